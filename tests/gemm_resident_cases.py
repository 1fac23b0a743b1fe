"""Cases of tests/test_gpu_gemm_resident.py, and the child process that runs them under one value of BBBP_GEMM_B_RESIDENT.

The GEMM knobs are read once per process, so the two forms of one product -- gemm_b3_kernel<1> (BBBP_GEMM_B_RESIDENT=2) and
gemm_b3r_kernel (=3), see GemmKnobs::b_resident in csrc/gemm.hip -- are run by two children of the test:

    BBBP_GEMM_B_RESIDENT=3 python tests/gemm_resident_cases.py out.npz
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORM_B3, FORM_RESIDENT = 2, 6          # bbbp_gemm_kernel_form (include/bbbp_hip.h)

# NN products the resident form takes: two row tiles, three (an odd count), a ragged last one; one and three column blocks; one, three
# and four k stages
MAIN = [(M, N, K) for M in (256, 384, 300) for N in (128, 384) for K in (32, 96, 128)]
# ... and products it must leave alone: K past the resident extent, N that is not whole column blocks, a single row tile, a batch
FALLBACK = [("k160", 256, 128, 160, 1), ("n200", 256, 200, 128, 1), ("m128", 128, 128, 128, 1), ("batch2", 256, 128, 128, 2)]
ENGINE_F, ENGINE_B = 64, 256           # the smallest batch with two row tiles; the image FC keeps N = 65536, K = 128


def operands(M, N, K, batch=1):
    """Standard normal, seeded; one row of A scaled by 1e4 and one column block of B by 1e-4, so that all three bf16 pieces of an
    element carry weight somewhere."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + batch)
    shape_a, shape_b = ((M, K), (K, N)) if batch == 1 else ((batch, M, K), (batch, K, N))
    a, b = torch.randn(*shape_a, generator=g), torch.randn(*shape_b, generator=g)
    a[..., 7, :] *= 1e4
    b[..., :, 32:64] *= 1e-4
    return a, b


def epilogue_operands(M, N):
    g = torch.Generator().manual_seed(5)
    return torch.randn(M, N, generator=g), torch.randn(M, N, generator=g), torch.randn(N, generator=g)      # residual, gate, bias


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_all(dev):
    import bbbp_amd
    from bbbp_amd import _lib, ops
    from helpers import synth_inputs
    L = _lib.lib()
    out = {}
    for M, N, K in MAIN:
        a, b = operands(M, N, K)
        out[f"main/{M}x{N}x{K}"] = ops.gemm(a.to(dev), b.to(dev)).cpu().numpy()
        out[f"form/{M}x{N}x{K}"] = np.int64(L.bbbp_gemm_kernel_form(0, 0, M, N, K, 1))
    for name, M, N, K, batch in FALLBACK:
        a, b = operands(M, N, K, batch)
        out[f"fallback/{name}"] = ops.gemm(a.to(dev), b.to(dev)).cpu().numpy()
        out[f"form/{name}"] = np.int64(L.bbbp_gemm_kernel_form(0, 0, M, N, K, batch))
    M, N, K = 300, 384, 128
    a, b = (t.to(dev) for t in operands(M, N, K))
    res, gate, bias = (t.to(dev) for t in epilogue_operands(M, N))
    out["epilogue/residual"] = ops.gemm(a, b, alpha=0.5, residual=res).cpu().numpy()
    out["epilogue/gate"] = ops.gemm(a, b, gate=gate, gate_scale=1.25).cpu().numpy()
    out["epilogue/gate_after_residual"] = ops.gemm(a, b, gate=gate, gate_scale=1.25, residual=res, gate_after_residual=True).cpu().numpy()
    out["epilogue/bias_relu"] = ops.gemm(a, b, alpha=0.5, bias=bias, act="relu").cpu().numpy()
    # one training step of the flagship model
    torch.manual_seed(3)
    model = bbbp_amd.MixedInputModel(ENGINE_F, 128).to(dev).train()
    fp, img, y = (t.to(dev) for t in synth_inputs(11, ENGINE_B, ENGINE_F, 49152))
    torch.manual_seed(99)                                   # the dropout seeds
    pred = model(fp, img)
    loss = bbbp_amd.MSELoss()(pred.squeeze(), y)
    loss.backward()
    torch.cuda.synchronize()
    names = ["output"] + [n for n, _ in model.named_parameters()]
    tensors = [pred] + [p.grad for _, p in model.named_parameters()]
    assert all(t is not None for t in tensors)
    out["engine/names"] = np.array(names)
    out["engine/digests"] = np.array([digest(t) for t in tensors])
    out["engine/sums"] = np.array([float(t.double().abs().sum()) for t in tensors])
    out["form/engine"] = np.int64(L.bbbp_gemm_kernel_form(0, 0, ENGINE_B, 65536, 128, 1))
    return out


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    np.savez(sys.argv[1], **run_all(torch.device("cuda:0")))
