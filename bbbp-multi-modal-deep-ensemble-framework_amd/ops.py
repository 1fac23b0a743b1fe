"""torch-tensor front end of the C ABI: one thin function per entry point of include/bbbp_hip.h.

torch supplies device memory and the current HIP stream; all arithmetic happens in libbbbp_hip.so.
Every function raises on non-CUDA / non-fp32 / non-contiguous operands, exactly like a torch op
would, and there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import ctypes
import threading

import torch

from . import _lib

ACT = {None: 0, "none": 0, "relu": 1, "tanh": 2, 0: 0, 1: 1, 2: 2}


_SEED_BASE = 0                  # device address of a 64-bit step counter the dropout streams are keyed from (training.GraphedTrainStep), or 0
_tls = threading.local()


def set_seed_base(ptr: int) -> int:
    """Key every seeded op's dropout stream from the 64-bit integer at device address ``ptr`` (``bbbp_set_seed_base``); 0 restores the
    default.  Process-wide on the Python side -- the library's setting is per thread and autograd runs backward nodes on its own
    threads, so every op call re-applies it for the thread it runs on (``_stream``).  Returns the previous address."""
    global _SEED_BASE
    prev, _SEED_BASE = _SEED_BASE, int(ptr or 0)
    return prev


def _stream() -> int:
    # every op passes here exactly once before it launches: the place to bring the calling thread's seed base up to date
    if _SEED_BASE or getattr(_tls, "applied", 0):
        _lib.check(_lib.lib().bbbp_set_seed_base(_SEED_BASE or None), "bbbp_set_seed_base")
        _tls.applied = _SEED_BASE
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA (HIP) tensor, got device {t.device}; the BBBP hot path has no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _rowmajor_2d(t: torch.Tensor, name: str) -> Tuple[int, int, int]:
    """(rows, cols, ld) of a 2-D tensor whose last dim is contiguous (column slices allowed)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{name}: expected a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    return t.shape[0], t.shape[1], ld


def _gemm_desc(a, b, trans_a, trans_b, alpha, bias, residual, act, out, gate, gate_scale, gate_after_residual=False, dropout_p=0.0,
               dropout_seed=0):
    """Validate one product and describe it as a bbbp_gemm_desc; returns (desc, out, split-K workspace bytes)."""
    _chk(a, "a"); _chk(b, "b")
    batched = a.dim() == 3
    if batched:
        if not (a.is_contiguous() and b.is_contiguous()):
            raise RuntimeError("batched gemm: operands must be contiguous")
        nb = a.shape[0]
        ar, ac = a.shape[1], a.shape[2]
        br, bc = b.shape[1], b.shape[2]
        lda, ldb = ac, bc
        sa, sb = ar * ac, br * bc
    else:
        nb = 1
        ar, ac, lda = _rowmajor_2d(a, "a")
        br, bc, ldb = _rowmajor_2d(b, "b")
        sa = sb = 0
    M, K = (ac, ar) if trans_a else (ar, ac)
    K2, N = (bc, br) if trans_b else (br, bc)
    if K != K2:
        raise RuntimeError(f"gemm: inner dimensions differ ({K} vs {K2})")
    if out is None:
        out = torch.empty((nb, M, N) if batched else (M, N), device=a.device, dtype=torch.float32)
    _chk(out, "out")
    ldc = N if batched else _rowmajor_2d(out, "out")[2]
    sc = M * N if batched else 0
    ldr, sr = 0, 0
    if residual is not None:
        _chk(residual, "residual")
        ldr = N if batched else _rowmajor_2d(residual, "residual")[2]
        sr = M * N if batched else 0
    ldg, sg = 0, 0
    if gate is not None:
        _chk(gate, "gate")
        if tuple(gate.shape) != tuple(out.shape):
            raise RuntimeError(f"gemm: gate shape {tuple(gate.shape)} != output shape {tuple(out.shape)}")
        ldg = N if batched else _rowmajor_2d(gate, "gate")[2]
        sg = M * N if batched else 0
    if bias is not None:
        _chk(bias, "bias")
        if bias.numel() != N:
            raise RuntimeError(f"gemm: bias has {bias.numel()} elements, expected {N}")
    d = _lib.GemmDesc(int(trans_a), int(trans_b), M, N, K, float(alpha), a.data_ptr(), lda, b.data_ptr(), ldb,
                      out.data_ptr(), ldc, _p(bias), _p(residual), ldr, ACT[act], _p(gate), ldg, float(gate_scale), nb,
                      sa, sb, sc, sr, sg, int(bool(gate_after_residual)), None, float(dropout_p), int(dropout_seed))
    return d, out, _lib.lib().bbbp_gemm_workspace_bytes(M, N, K, nb)


def gemm(a: torch.Tensor, b: torch.Tensor, *, trans_a: bool = False, trans_b: bool = False, alpha: float = 1.0,
         bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act=None,
         out: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, gate_scale: float = 1.0,
         gate_after_residual: bool = False) -> torch.Tensor:
    """out = gate_mask(act(alpha * op(a) @ op(b) + bias)) + residual  (2-D; or 3-D batched with equal batch dims).

    gate: optional tensor of the output's shape; the result is multiplied by gate_scale where gate > 0, by 0 elsewhere
    (before the residual is added, or after it with gate_after_residual)."""
    if gate is not None:
        return gemm_grouped([dict(a=a, b=b, trans_a=trans_a, trans_b=trans_b, alpha=alpha, bias=bias, residual=residual,
                                  act=act, out=out, gate=gate, gate_scale=gate_scale, gate_after_residual=gate_after_residual)])[0]
    d, out, wsb = _gemm_desc(a, b, trans_a, trans_b, alpha, bias, residual, act, out, None, 1.0)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=a.device)
    _lib.check(_lib.lib().bbbp_gemm_f32(_stream(), d.transA, d.transB, d.M, d.N, d.K, d.alpha, d.A, d.lda, d.B, d.ldb,
                                        d.C, d.ldc, d.bias, d.residual, d.ldr, d.act, d.batch, d.strideA, d.strideB,
                                        d.strideC, d.strideR, ws.data_ptr(), wsb), "bbbp_gemm_f32")
    return out


def gemm_grouped(problems) -> list:
    """Independent products (dicts of gemm()'s arguments); neighbours that are small enough share one launch."""
    keys = ("trans_a", "trans_b", "alpha", "bias", "residual", "act", "out", "gate", "gate_scale", "gate_after_residual", "dropout_p",
            "dropout_seed")
    defaults = dict(trans_a=False, trans_b=False, alpha=1.0, bias=None, residual=None, act=None, out=None, gate=None,
                    gate_scale=1.0, gate_after_residual=False, dropout_p=0.0, dropout_seed=0)
    descs, outs, wsb = [], [], 0
    for pr in problems:
        kw = {k: pr.get(k, defaults[k]) for k in keys}
        d, out, w = _gemm_desc(pr["a"], pr["b"], kw["trans_a"], kw["trans_b"], kw["alpha"], kw["bias"], kw["residual"],
                               kw["act"], kw["out"], kw["gate"], kw["gate_scale"], kw["gate_after_residual"], kw["dropout_p"],
                               kw["dropout_seed"])
        descs.append(d); outs.append(out); wsb = max(wsb, w)
    if not descs:
        return []
    arr = (_lib.GemmDesc * len(descs))(*descs)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=outs[0].device)
    _lib.check(_lib.lib().bbbp_gemm_f32_grouped(_stream(), arr, len(descs), ws.data_ptr(), wsb), "bbbp_gemm_f32_grouped")
    return outs


def linear_weight_bias_grad(dy: torch.Tensor, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dW = dy^T x and db = column sums of dy for a Linear (2-D).  When the product takes the small-GEMM path both come out of
    ONE launch: the bias gradient rides through the same MFMAs as a virtual all-ones column of x (bbbp_gemm_desc.asum)."""
    M, N = dy.shape
    K = x.shape[1]
    L = _lib.lib()
    if not L.bbbp_gemm_folds_asum(N, K, M, 1):
        return gemm(dy, x, trans_a=True), dy.sum(dim=0)
    d, dw, wsb = _gemm_desc(dy, x, True, False, 1.0, None, None, None, None, None, 1.0)
    db = torch.empty(N, device=dy.device, dtype=torch.float32)
    d.asum = db.data_ptr()
    arr = (_lib.GemmDesc * 1)(d)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dy.device)
    _lib.check(L.bbbp_gemm_f32_grouped(_stream(), arr, 1, ws.data_ptr(), wsb), "bbbp_gemm_f32_grouped")
    return dw, db


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear (+activation, +residual) on the MFMA GEMM."""
    return gemm(x, weight, trans_b=True, bias=bias, act=act, residual=residual, out=out)


def conv3x3_relu_pool_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, keep_mask: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``keep_mask=False``: a forward-only call -- no pooling decisions are written (the C entry takes a null mask) and None is returned
    in their place."""
    _chk(x, "x"); _chk(w, "weight"); _chk(b, "bias")
    if not (x.is_contiguous() and w.is_contiguous() and b.is_contiguous()):
        raise RuntimeError("conv3x3_relu_pool: operands must be contiguous (NCHW)")
    B, cin, H, W = x.shape
    cout = w.shape[0]
    if tuple(w.shape) != (cout, cin, 3, 3):
        raise RuntimeError(f"conv3x3_relu_pool: weight shape {tuple(w.shape)} does not match input channels {cin}")
    y = torch.empty((B, cout, H // 2, W // 2), device=x.device, dtype=torch.float32)
    mask = torch.empty((B, cout, H // 2, W // 2), device=x.device, dtype=torch.uint8) if keep_mask else None
    L = _lib.lib()
    wsb = L.bbbp_conv3x3_workspace_bytes(B, cin, cout, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    _lib.check(L.bbbp_conv3x3_relu_pool_fwd(_stream(), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                            mask.data_ptr() if keep_mask else None, B, cin, cout, H, W, ws.data_ptr(), wsb),
               "bbbp_conv3x3_relu_pool_fwd")
    return y, mask


def _conv_bwd_check(what: str, gy: torch.Tensor, mask: torch.Tensor, x: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None) -> None:
    """The shapes a conv backward op reads must fit each other: the kernels index ``mask`` like ``gy`` and ``x`` / ``w`` by the stage's
    channel counts, so a short or strided operand is read out of bounds or silently mixes channels."""
    if gy.dim() != 4:
        raise RuntimeError(f"{what}: gy must be [B, cout, H/2, W/2], got shape {tuple(gy.shape)}")
    if tuple(mask.shape) != tuple(gy.shape):
        raise RuntimeError(f"{what}: mask shape {tuple(mask.shape)} != gy shape {tuple(gy.shape)}")
    if not mask.is_contiguous():
        raise RuntimeError(f"{what}: mask must be contiguous, got shape {tuple(mask.shape)} strides {mask.stride()}")
    B, cout, Hp, Wp = gy.shape
    if x is not None:
        if x.dim() != 4 or not x.is_contiguous():
            raise RuntimeError(f"{what}: x must be contiguous NCHW, got shape {tuple(x.shape)} strides {x.stride()}")
        if x.shape[2] % 2 or x.shape[3] % 2:
            raise RuntimeError(f"{what}: x has an odd height or width, shape {tuple(x.shape)}")
        if (x.shape[0], x.shape[2] // 2, x.shape[3] // 2) != (B, Hp, Wp):
            raise RuntimeError(f"{what}: gy shape {tuple(gy.shape)} does not match x shape {tuple(x.shape)} (batch, H/2, W/2)")
    if w is not None:
        if not w.is_contiguous():
            raise RuntimeError(f"{what}: weight must be contiguous, got shape {tuple(w.shape)} strides {w.stride()}")
        if w.dim() != 4 or tuple(w.shape) != (cout, w.shape[1], 3, 3):
            raise RuntimeError(f"{what}: weight shape {tuple(w.shape)} is not ({cout}, cin, 3, 3) for gy shape {tuple(gy.shape)}")


def conv3x3_relu_pool_bwd_data(gy: torch.Tensor, mask: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    _chk(gy, "gy"); _chk(mask, "mask", torch.uint8); _chk(w, "weight")
    _conv_bwd_check("conv3x3_relu_pool_bwd_data", gy, mask, w=w)
    gy = gy.contiguous()
    B, cout, Hp, Wp = gy.shape
    cin = w.shape[1]
    H, W = 2 * Hp, 2 * Wp
    dx = torch.empty((B, cin, H, W), device=gy.device, dtype=torch.float32)
    L = _lib.lib()
    wsb = L.bbbp_conv3x3_workspace_bytes(B, cin, cout, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=gy.device)
    _lib.check(L.bbbp_conv3x3_relu_pool_bwd_data(_stream(), gy.data_ptr(), mask.data_ptr(), w.data_ptr(), dx.data_ptr(),
                                                 B, cin, cout, H, W, ws.data_ptr(), wsb), "bbbp_conv3x3_relu_pool_bwd_data")
    return dx


def conv3x3_relu_pool_bwd_weight(x: torch.Tensor, gy: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _chk(x, "x"); _chk(gy, "gy"); _chk(mask, "mask", torch.uint8)
    _conv_bwd_check("conv3x3_relu_pool_bwd_weight", gy, mask, x=x)
    gy = gy.contiguous()
    B, cin, H, W = x.shape
    cout = gy.shape[1]
    dw = torch.empty((cout, cin, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.empty((cout,), device=x.device, dtype=torch.float32)
    L = _lib.lib()
    wsb = L.bbbp_conv3x3_workspace_bytes(B, cin, cout, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    _lib.check(L.bbbp_conv3x3_relu_pool_bwd_weight(_stream(), x.data_ptr(), gy.data_ptr(), mask.data_ptr(), dw.data_ptr(),
                                                   db.data_ptr(), B, cin, cout, H, W, ws.data_ptr(), wsb),
               "bbbp_conv3x3_relu_pool_bwd_weight")
    return dw, db


def layernorm_fwd(x: torch.Tensor, residual: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                  eps: float = 1e-5, dropout_p: float = 0.0, seed: int = 0):
    """Returns (y, z, mean, rstd) with z = dropout(x) + residual (x is NOT modified: it is cloned)."""
    _chk(x, "x")
    z = x.contiguous().clone()
    rows, cols = z.shape
    y = torch.empty_like(z)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().bbbp_layernorm_fwd(_stream(), z.data_ptr(), _p(residual), y.data_ptr(), gamma.data_ptr(),
                                             beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, cols, eps,
                                             dropout_p, seed), "bbbp_layernorm_fwd")
    return y, z, mean, rstd


def linear_layernorm_fwd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor],
                         gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, dropout_p: float = 0.0, seed: int = 0):
    """y = LayerNorm(dropout(x @ weight.T + bias) + residual) in ONE launch (narrow outputs: weight [N <= 256, K]).
    Returns (y, z, mean, rstd) like ``layernorm_fwd``."""
    _chk(x, "x"); _chk(weight, "weight")
    x = x.contiguous(); weight = weight.contiguous()
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise RuntimeError("linear_layernorm_fwd: inner dimensions differ")
    z = torch.empty((M, N), device=x.device, dtype=torch.float32)
    y = torch.empty_like(z)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    res = residual.contiguous() if residual is not None else None
    _lib.check(_lib.lib().bbbp_linear_layernorm_fwd(_stream(), x.data_ptr(), K, weight.data_ptr(), _p(bias), _p(res), N, z.data_ptr(), N,
                                                    y.data_ptr(), N, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                    M, N, K, eps, dropout_p, seed), "bbbp_linear_layernorm_fwd")
    return y, z, mean, rstd


def layernorm_linear_fwd(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                         act: int = 0, eps: float = 1e-5, dropout_p: float = 0.0, seed: int = 0):
    """out = dropout(act(LayerNorm(z) @ weight.T + bias)) with the LayerNorm absorbed by the product (ONE launch; K = z.shape[1] <= 192).
    Returns (out [M, N], y = LayerNorm(z) [M, K], mean [M], rstd [M])."""
    _chk(z, "z"); _chk(weight, "weight"); _chk(gamma, "gamma"); _chk(beta, "beta")
    z = z.contiguous(); weight = weight.contiguous()
    M, K = z.shape
    N = weight.shape[0]
    if weight.shape[1] != K or gamma.numel() != K or beta.numel() != K:
        raise RuntimeError("layernorm_linear_fwd: inner dimensions differ")
    L = _lib.lib()
    if not L.bbbp_layernorm_linear_supported(M, N, K):
        raise RuntimeError(f"layernorm_linear_fwd: shape M={M} N={N} K={K} is not supported (K <= 192)")
    out = torch.empty((M, N), device=z.device, dtype=torch.float32)
    y = torch.empty_like(z)
    mean = torch.empty(M, device=z.device, dtype=torch.float32)
    rstd = torch.empty(M, device=z.device, dtype=torch.float32)
    _lib.check(L.bbbp_layernorm_linear_fwd(_stream(), z.data_ptr(), K, gamma.data_ptr(), beta.data_ptr(), eps, weight.data_ptr(), _p(bias),
                                           out.data_ptr(), N, act, dropout_p, seed, y.data_ptr(), K, mean.data_ptr(), rstd.data_ptr(), M, N, K),
               "bbbp_layernorm_linear_fwd")
    return out, y, mean, rstd


def layernorm_bwd(dy, z, gamma, mean, rstd, dropout_p: float = 0.0, seed: int = 0):
    """Returns (dz, dx, dgamma, dbeta); dx is dz when dropout_p == 0."""
    rows, cols = z.shape
    dz = torch.empty_like(z)
    dx = torch.empty_like(z) if dropout_p > 0 else None
    dg = torch.empty(cols, device=z.device, dtype=torch.float32)
    db = torch.empty(cols, device=z.device, dtype=torch.float32)
    _lib.check(_lib.lib().bbbp_layernorm_bwd(_stream(), dy.contiguous().data_ptr(), z.data_ptr(), gamma.data_ptr(),
                                             mean.data_ptr(), rstd.data_ptr(), dz.data_ptr(), _p(dx), dg.data_ptr(),
                                             db.data_ptr(), rows, cols, dropout_p, seed), "bbbp_layernorm_bwd")
    return dz, (dx if dx is not None else dz), dg, db


def softmax_fwd(x: torch.Tensor, dropout_p: float = 0.0, seed: int = 0):
    """Row softmax over the last dim of a contiguous tensor. Returns (prob, dropped_prob)."""
    p = _chk(x, "x").contiguous().clone()
    cols = p.shape[-1]
    rows = p.numel() // cols
    pd = torch.empty_like(p) if dropout_p > 0 else None
    _lib.check(_lib.lib().bbbp_softmax_fwd(_stream(), p.data_ptr(), _p(pd), rows, cols, dropout_p, seed), "bbbp_softmax_fwd")
    return p, (pd if pd is not None else p)


def softmax_bwd(dprob: torch.Tensor, prob: torch.Tensor, dropout_p: float = 0.0, seed: int = 0) -> torch.Tensor:
    d = _chk(dprob, "dprob").contiguous().clone()
    prob = _chk(prob, "prob")
    if prob.shape != d.shape or not prob.is_contiguous():
        raise RuntimeError(f"softmax_bwd: prob must be contiguous and shaped like dprob, got {tuple(prob.shape)} vs {tuple(d.shape)}")
    cols = d.shape[-1]
    _lib.check(_lib.lib().bbbp_softmax_bwd(_stream(), d.data_ptr(), prob.data_ptr(), d.numel() // cols, cols, dropout_p, seed),
               "bbbp_softmax_bwd")
    return d


def _attention_shape(qkv: torch.Tensor, nhead: int, what: str) -> Tuple[int, int, int]:
    """(B, F, head_dim) of a contiguous qkv [B, 3F] = Q | K | V with F = nhead * head_dim."""
    _chk(qkv, "qkv")
    if qkv.dim() != 2 or not qkv.is_contiguous() or nhead < 1 or qkv.shape[0] < 1 or qkv.shape[1] % (3 * nhead) != 0 or qkv.shape[1] == 0:
        raise RuntimeError(f"{what}: qkv must be a contiguous [B, 3 * nhead * head_dim] tensor, got shape {tuple(qkv.shape)} for nhead={nhead}")
    B, F = qkv.shape[0], qkv.shape[1] // 3
    return B, F, F // nhead


def attention_fwd(qkv: torch.Tensor, nhead: int, scale: Optional[float] = None, dropout_p: float = 0.0, seed: int = 0,
                  keep_mask: bool = False):
    """Fused self-attention over the rows of qkv [B, 3F] (``bbbp_attention_fwd``; small-head or wide-head kernels by shape).  Returns
    (ctx [B, F], lse [nhead, B], keep): ``keep`` holds the dropout decisions for ``attention_bwd`` when ``keep_mask`` and the shape's
    kernels save them (``bbbp_attention_keep_bytes`` > 0), else None.  ``scale`` defaults to head_dim ** -0.5."""
    B, F, D = _attention_shape(qkv, nhead, "attention_fwd")
    L = _lib.lib()
    ctx = torch.empty((B, F), device=qkv.device, dtype=torch.float32)
    lse = torch.empty((nhead, B), device=qkv.device, dtype=torch.float32)
    kb = L.bbbp_attention_keep_bytes(B, nhead, D) if keep_mask else 0
    keep = torch.empty(kb, device=qkv.device, dtype=torch.uint8) if kb else None
    _lib.check(L.bbbp_attention_fwd(_stream(), qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, F, nhead,
                                    D ** -0.5 if scale is None else scale, dropout_p, seed, _p(keep)), "bbbp_attention_fwd")
    return ctx, lse, keep


def attention_bwd(qkv: torch.Tensor, ctx: torch.Tensor, lse: torch.Tensor, dctx: torch.Tensor, nhead: int, scale: Optional[float] = None,
                  dropout_p: float = 0.0, seed: int = 0, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dqkv [B, 3F] from the forward call's operands and results (``bbbp_attention_bwd``); ``keep``: the forward call's decisions, or None
    to draw the stream again."""
    B, F, D = _attention_shape(qkv, nhead, "attention_bwd")
    for t, n, shape in ((ctx, "ctx", (B, F)), (lse, "lse", (nhead, B)), (dctx, "dctx", (B, F))):
        if tuple(_chk(t, n).shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"attention_bwd: {n} must be contiguous and shaped {shape}, got {tuple(t.shape)} strides {t.stride()}")
    L = _lib.lib()
    if keep is not None and (_chk(keep, "keep", torch.uint8).numel() != L.bbbp_attention_keep_bytes(B, nhead, D) or not keep.is_contiguous()):
        raise RuntimeError(f"attention_bwd: keep must hold {L.bbbp_attention_keep_bytes(B, nhead, D)} contiguous bytes, got {keep.numel()}")
    dqkv = torch.empty((B, 3 * F), device=qkv.device, dtype=torch.float32)
    _lib.check(L.bbbp_attention_bwd(_stream(), qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(), B, F, nhead,
                                    D ** -0.5 if scale is None else scale, dropout_p, seed, _p(keep)), "bbbp_attention_bwd")
    return dqkv


def attention_b3_fwd(qkv: torch.Tensor, nhead: int, scale: Optional[float] = None) -> torch.Tensor:
    """Forward-only self-attention of wide heads on the bf16 matrix pipe with split float32 operands (``bbbp_attention_b3_fwd``): ctx [B, F]."""
    B, F, D = _attention_shape(qkv, nhead, "attention_b3_fwd")
    L = _lib.lib()
    ctx = torch.empty((B, F), device=qkv.device, dtype=torch.float32)
    wsb = L.bbbp_attention_b3_workspace_bytes(B, nhead, D)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=qkv.device)
    _lib.check(L.bbbp_attention_b3_fwd(_stream(), qkv.data_ptr(), ctx.data_ptr(), B, F, nhead, D ** -0.5 if scale is None else scale,
                                       ws.data_ptr(), wsb), "bbbp_attention_b3_fwd")
    return ctx


def _dense(t: torch.Tensor, name: str, shape) -> int:
    """Device address of a contiguous float32 tensor of exactly ``shape``."""
    if tuple(_chk(t, name).shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor of shape {tuple(shape)}, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr()


def _outputs(out: Optional[dict], shapes: dict, device) -> dict:
    """The named outputs of an op: ``out[name]`` where the caller placed one (contiguous, of the op's shape), else a new tensor."""
    given = out or {}
    unknown = set(given) - set(shapes)
    if unknown:
        raise RuntimeError(f"out: unknown output name(s) {sorted(unknown)}; this op writes {sorted(shapes)}")
    o = {}
    for name, shape in shapes.items():
        if name in given:
            _dense(given[name], name, shape)
            o[name] = given[name]
        else:
            o[name] = torch.empty(shape, device=device, dtype=torch.float32)
    return o


def _output_lists(out: Optional[dict], shapes: dict, count: int, device) -> dict:
    """``_outputs`` for ops that write one tensor of every name per layer / norm: lists of ``count`` tensors."""
    given = out or {}
    unknown = set(given) - set(shapes)
    if unknown:
        raise RuntimeError(f"out: unknown output name(s) {sorted(unknown)}; this op writes {sorted(shapes)}")
    o = {}
    for name, shape in shapes.items():
        if name in given:
            if len(given[name]) != count:
                raise RuntimeError(f"out: {name} must list {count} tensors, got {len(given[name])}")
            for i, t in enumerate(given[name]):
                _dense(t, f"{name}[{i}]", shape)
            o[name] = list(given[name])
        else:
            o[name] = [torch.empty(shape, device=device, dtype=torch.float32) for _ in range(count)]
    return o


def outproj_fold_fwd(win, bin, wo, bo=None, out: Optional[dict] = None) -> dict:
    """out_proj folded into the value projection of one-head encoder layers (``bbbp_outproj_fold_fwd``), all layers in one launch.
    ``win`` [3F, F], ``bin`` [3F], ``wo`` [F, F] and (optional) ``bo`` [F]: lists with one tensor per layer.  Returns lists by name:
    wf [3F, F] = Wq; Wk; Wo Wv, bf [3F] = bq; bk; Wo bv (+ bo), wvt [F + 1, F] = [Wv | bv]^T.  ``out``: lists of tensors to write instead."""
    layers = len(win)
    if layers < 1 or not (len(bin) == len(wo) == layers) or (bo is not None and len(bo) != layers):
        raise RuntimeError("outproj_fold_fwd: win, bin, wo (and bo) must list one tensor per layer, at least one")
    F = _chk(wo[0], "wo[0]").shape[-1]
    L = _lib.lib()
    if not L.bbbp_outproj_fold_supported(F, 1, layers):
        raise RuntimeError(f"outproj_fold_fwd: F {F} with {layers} layers is not supported")
    ptrs = [[_dense(t, f"{n}[{i}]", shape) for i, t in enumerate(ts)]
            for n, ts, shape in (("win", win, (3 * F, F)), ("bin", bin, (3 * F,)), ("wo", wo, (F, F)))]
    bo_arr = None if bo is None else _lib.ptr_array([_dense(t, f"bo[{i}]", (F,)) for i, t in enumerate(bo)])
    o = _output_lists(out, {"wf": (3 * F, F), "bf": (3 * F,), "wvt": (F + 1, F)}, layers, wo[0].device)
    _lib.check(L.bbbp_outproj_fold_fwd(_stream(), layers, F, *[_lib.ptr_array(p) for p in ptrs], bo_arr,
                                       *[_lib.ptr_array([t.data_ptr() for t in o[n]]) for n in ("wf", "bf", "wvt")]), "bbbp_outproj_fold_fwd")
    return o


def outproj_fold_bwd(tdw: torch.Tensor, tdb: torch.Tensor, wo: torch.Tensor, wvt: torch.Tensor, dz: torch.Tensor,
                     out: Optional[dict] = None) -> dict:
    """The gradients of a folded layer unfolded (``bbbp_outproj_fold_bwd``): from ``tdw`` [F, F] = dW', ``tdb`` [F] = db', ``wo`` [F, F],
    ``wvt`` [F + 1, F] and ``dz`` [B, F] (rows may be padded) returns g_outw [F, F], g_outb [F], g_inw_v [F, F], g_inb_v [F] by name."""
    B, F, lddz = _rowmajor_2d(_chk(dz, "dz"), "dz")
    L = _lib.lib()
    if B < 1 or not L.bbbp_outproj_fold_supported(F, 1, 1):
        raise RuntimeError(f"outproj_fold_bwd: dz of shape {tuple(dz.shape)} is not supported")
    ins = [_dense(tdw, "tdw", (F, F)), _dense(tdb, "tdb", (F,)), _dense(wo, "wo", (F, F)), _dense(wvt, "wvt", (F + 1, F))]
    o = _outputs(out, {"g_outw": (F, F), "g_outb": (F,), "g_inw_v": (F, F), "g_inb_v": (F,)}, dz.device)
    _lib.check(L.bbbp_outproj_fold_bwd(_stream(), F, B, *ins, dz.data_ptr(), lddz, *[t.data_ptr() for t in o.values()]), "bbbp_outproj_fold_bwd")
    return o


def ln_param_grad(dy, z, mean, rstd, out: Optional[dict] = None) -> dict:
    """LayerNorm weight / bias gradients of n norms over [rows, cols] tensors (``bbbp_ln_param_grad``): ``dy``, ``z`` list [rows, cols]
    tensors, ``mean``, ``rstd`` [rows] tensors, one per norm.  Returns dgamma, dbeta: lists of n [cols] tensors."""
    n = len(dy)
    if n < 1 or not (len(z) == len(mean) == len(rstd) == n):
        raise RuntimeError("ln_param_grad: dy, z, mean and rstd must list one tensor per norm, at least one")
    if _chk(dy[0], "dy[0]").dim() != 2 or dy[0].shape[0] < 1 or dy[0].shape[1] < 1:
        raise RuntimeError(f"ln_param_grad: dy[0] must be a non-empty [rows, cols] tensor, got shape {tuple(dy[0].shape)}")
    rows, cols = dy[0].shape
    ptrs = [[_dense(t, f"{name}[{i}]", shape) for i, t in enumerate(ts)]
            for name, ts, shape in (("dy", dy, (rows, cols)), ("z", z, (rows, cols)), ("mean", mean, (rows,)), ("rstd", rstd, (rows,)))]
    o = _output_lists(out, {"dgamma": (cols,), "dbeta": (cols,)}, n, dy[0].device)
    _lib.check(_lib.lib().bbbp_ln_param_grad(_stream(), n, *[_lib.ptr_array(p) for p in ptrs],
                                             *[_lib.ptr_array([t.data_ptr() for t in o[k]]) for k in ("dgamma", "dbeta")], rows, cols),
               "bbbp_ln_param_grad")
    return o


def _encoder_rows_shapes(F: int, DFF: int) -> dict:
    return {"wo": (F, F), "bo": (F,), "g1": (F,), "be1": (F,), "w1": (DFF, F), "b1": (DFF,), "w2": (F, DFF), "b2": (F,), "g2": (F,), "be2": (F,)}


def encoder_rows_fwd(ctx: torch.Tensor, xin: torch.Tensor, weights: dict, p: float = 0.0, seeds=(0, 0, 0), nxt: Optional[dict] = None,
                     out: Optional[dict] = None) -> dict:
    """The row-local stretch of a post-norm encoder layer, forward, as one launch (``bbbp_encoder_rows_fwd``).  ``ctx``, ``xin`` [B, F];
    ``weights``: wo, bo, g1, be1, w1 [DFF, F], b1, w2 [F, DFF], b2, g2, be2; ``seeds``: the dropout streams of the three sites.  ``nxt``
    (optional): the next projection, dict(wn [nn, F], bn [nn], act (None or "relu"), outn (optional [B, nn] tensor, which may be a column
    slice of a wider buffer)).  Returns z1, y1, hff, z2, y2, mean1, rstd1, mean2, rstd2 and outn (None without ``nxt``) by name."""
    if _chk(ctx, "ctx").dim() != 2 or ctx.shape[0] < 1:
        raise RuntimeError(f"encoder_rows_fwd: ctx must be a non-empty [B, F] tensor, got shape {tuple(ctx.shape)}")
    B, F = ctx.shape
    DFF = _chk(weights["w1"], "w1").shape[0]
    L = _lib.lib()
    if not L.bbbp_encoder_rows_supported(F, 1, DFF):
        raise RuntimeError(f"encoder_rows_fwd: F {F}, DFF {DFF} is not supported")
    d = _lib.EncoderRowsFwdDesc(B=B, F=F, DFF=DFF, dropout_p=float(p), seed1=int(seeds[0]), seed2=int(seeds[1]), seed3=int(seeds[2]),
                                ctx=_dense(ctx, "ctx", (B, F)), xin=_dense(xin, "xin", (B, F)))
    for name, shape in _encoder_rows_shapes(F, DFF).items():
        setattr(d, name, _dense(weights[name], name, shape))
    out = dict(out or {})
    outn = out.pop("outn", None)
    if nxt is not None:
        nn = _chk(nxt["wn"], "wn").shape[0]
        d.wn, d.bn, d.nn, d.actn = _dense(nxt["wn"], "wn", (nn, F)), _dense(nxt["bn"], "bn", (nn,)), nn, ACT[nxt.get("act")]
        outn = nxt.get("outn", outn)
        if outn is None:
            outn = torch.empty((B, nn), device=ctx.device, dtype=torch.float32)
        rows, cols, ldn = _rowmajor_2d(_chk(outn, "outn"), "outn")
        if (rows, cols) != (B, nn):
            raise RuntimeError(f"encoder_rows_fwd: outn must be shaped {(B, nn)}, got {tuple(outn.shape)}")
        d.outn, d.ldn = outn.data_ptr(), ldn
    elif outn is not None:
        raise RuntimeError("encoder_rows_fwd: outn given without a next projection")
    o = _outputs(out, {"z1": (B, F), "y1": (B, F), "hff": (B, DFF), "z2": (B, F), "y2": (B, F), "mean1": (B,), "rstd1": (B,),
                       "mean2": (B,), "rstd2": (B,)}, ctx.device)
    for name, t in o.items():
        setattr(d, name, t.data_ptr())
    _lib.check(L.bbbp_encoder_rows_fwd(_stream(), ctypes.byref(d)), "bbbp_encoder_rows_fwd")
    o["outn"] = outn
    return o


def encoder_rows_bwd(saved: dict, weights: dict, dyout: Optional[torch.Tensor] = None, up: Optional[dict] = None, p: float = 0.0,
                     seeds=(0, 0), out: Optional[dict] = None) -> dict:
    """The row-local stretch of a post-norm encoder layer, backward, as one launch (``bbbp_encoder_rows_bwd``).  ``saved``: z1, z2, hff,
    mean1, rstd1, mean2, rstd2 as ``encoder_rows_fwd`` returns them (taken as given); ``weights``: g1, g2, w1, w2, wo; ``seeds``: the streams
    of sites 1 and 3.  Either ``dyout`` [B, F], the gradient of the layer's output, or ``up`` = dict(dqkv_up [B, 3F], win_up [3F, F],
    dz1_up [B, F]) of the layer above, from which stage 0 forms it (into ``out["dyout"]`` or a new tensor).  Returns dyout, dz2, dff, dhff,
    dy1, dz1, dsa, dctx by name."""
    if _chk(saved["z1"], "z1").dim() != 2 or saved["z1"].shape[0] < 1:
        raise RuntimeError(f"encoder_rows_bwd: z1 must be a non-empty [B, F] tensor, got shape {tuple(saved['z1'].shape)}")
    B, F = saved["z1"].shape
    DFF = _chk(weights["w1"], "w1").shape[0]
    L = _lib.lib()
    if not L.bbbp_encoder_rows_supported(F, 1, DFF):
        raise RuntimeError(f"encoder_rows_bwd: F {F}, DFF {DFF} is not supported")
    if (dyout is None) == (up is None):
        raise RuntimeError("encoder_rows_bwd: pass either dyout or up (dqkv_up, win_up, dz1_up)")
    d = _lib.EncoderRowsBwdDesc(B=B, F=F, DFF=DFF, dropout_p=float(p), seed1=int(seeds[0]), seed3=int(seeds[1]))
    for name, shape in (("z1", (B, F)), ("z2", (B, F)), ("hff", (B, DFF)), ("mean1", (B,)), ("rstd1", (B,)), ("mean2", (B,)), ("rstd2", (B,))):
        setattr(d, name, _dense(saved[name], name, shape))
    shapes = _encoder_rows_shapes(F, DFF)
    for name in ("g1", "g2", "w1", "w2", "wo"):
        setattr(d, name, _dense(weights[name], name, shapes[name]))
    outs = {"dz2": (B, F), "dff": (B, F), "dhff": (B, DFF), "dy1": (B, F), "dz1": (B, F), "dsa": (B, F), "dctx": (B, F)}
    if up is not None:
        d.dqkv_up, d.win_up, d.dz1_up = (_dense(up["dqkv_up"], "dqkv_up", (B, 3 * F)), _dense(up["win_up"], "win_up", (3 * F, F)),
                                         _dense(up["dz1_up"], "dz1_up", (B, F)))
        outs = {"dyout": (B, F), **outs}
        o = _outputs(out, outs, saved["z1"].device)
    else:
        o = {"dyout": dyout, **_outputs(out, outs, saved["z1"].device)}
        _dense(dyout, "dyout", (B, F))
    for name, t in o.items():
        setattr(d, name, t.data_ptr())
    _lib.check(L.bbbp_encoder_rows_bwd(_stream(), ctypes.byref(d)), "bbbp_encoder_rows_bwd")
    return o


def dropout(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    x = _chk(x, "x").contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.lib().bbbp_dropout(_stream(), x.data_ptr(), y.data_ptr(), x.numel(), p, seed), "bbbp_dropout")
    return y


def _column_vectors(what: str, cols: int, **vectors) -> None:
    """The per-column operands of a BatchNorm call: float32 device tensors of ``cols`` contiguous elements (the kernels index them unchecked)."""
    for name, t in vectors.items():
        if _chk(t, name).numel() != cols or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must hold {cols} contiguous elements, got shape {tuple(t.shape)} strides {t.stride()}")


def batchnorm1d_fwd(x, gamma, beta, running_mean, running_var, training: bool, eps: float = 1e-5, momentum: float = 0.1):
    """Returns (y, save_mean, save_rstd); running stats are updated in place when training."""
    x = _chk(x, "x").contiguous()
    rows, cols = x.shape
    _column_vectors("batchnorm1d_fwd", cols, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var)
    y = torch.empty_like(x)
    sm = torch.empty(cols, device=x.device, dtype=torch.float32)
    sr = torch.empty(cols, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().bbbp_batchnorm1d_fwd(_stream(), x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                               running_mean.data_ptr(), running_var.data_ptr(), sm.data_ptr(), sr.data_ptr(),
                                               rows, cols, eps, momentum, int(training)), "bbbp_batchnorm1d_fwd")
    return y, sm, sr


def batchnorm1d_bwd(dy, x, gamma, save_mean, save_rstd, training: bool):
    x = _chk(x, "x").contiguous(); dy = _chk(dy, "dy").contiguous()
    if x.dim() != 2 or dy.shape != x.shape:
        raise RuntimeError(f"batchnorm1d_bwd: dy and x must be 2-D and shaped alike, got {tuple(dy.shape)} vs {tuple(x.shape)}")
    rows, cols = x.shape
    _column_vectors("batchnorm1d_bwd", cols, gamma=gamma, save_mean=save_mean, save_rstd=save_rstd)
    dx = torch.empty_like(x)
    dg = torch.empty(cols, device=x.device, dtype=torch.float32)
    db = torch.empty(cols, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().bbbp_batchnorm1d_bwd(_stream(), dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), save_mean.data_ptr(),
                                               save_rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, cols,
                                               int(training)), "bbbp_batchnorm1d_bwd")
    return dx, dg, db


def bias_act_bwd(dy: torch.Tensor, y: Optional[torch.Tensor], act=None, scale: float = 1.0):
    """In place: dy *= act'(y) * scale.  Returns the column sums (bias gradient)."""
    rows, cols, lddy = _rowmajor_2d(_chk(dy, "dy"), "dy")
    ldy = 0
    if y is not None:
        ldy = _rowmajor_2d(_chk(y, "y"), "y")[2]
        if y.shape != dy.shape:
            raise RuntimeError(f"bias_act_bwd: y must be shaped like dy, got {tuple(y.shape)} vs {tuple(dy.shape)}")
    db = torch.empty(cols, device=dy.device, dtype=torch.float32)
    _lib.check(_lib.lib().bbbp_bias_act_bwd(_stream(), dy.data_ptr(), lddy, _p(y), ldy, db.data_ptr(), rows, cols, ACT[act],
                                            scale), "bbbp_bias_act_bwd")
    return db


# parameters of the fusion block and the head as ops.head_fwd / head_bwd take them: name -> shape; fw1 .. fb2 are lists of four tensors
HEAD_PARAM_SHAPES = {"fw1": (128, 256), "fb1": (128,), "fw2": (128,), "fb2": (1,), "w0": (256, 256), "b0": (256,), "gamma": (256,),
                     "beta": (256,), "w3": (128, 256), "b3": (128,), "w5": (64, 128), "b5": (64,), "w7": (64,), "b7": (1,)}
_HEAD_PER_HEAD = ("fw1", "fb1", "fw2", "fb2")


def _head_operand(t: torch.Tensor, name: str, shape) -> int:
    """Device address of a contiguous float32 tensor of ``shape`` (any shape with as many elements: the kernels index it flat)."""
    numel = 1
    for s in shape:
        numel *= s
    if _chk(t, name).numel() != numel or not t.is_contiguous():
        raise RuntimeError(f"head: {name} must hold {numel} contiguous elements ({shape}), got shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr()


def _head_params(params, names, what: str):
    """ctypes arguments of the named parameters, in order: a pointer array per fusion-block entry, an address per head entry."""
    args = []
    for n in names:
        if n in _HEAD_PER_HEAD:
            if len(params[n]) != 4:
                raise RuntimeError(f"{what}: {n} must list the four fusion heads' tensors, got {len(params[n])}")
            args.append(_lib.ptr_array([_head_operand(t, f"{n}[{i}]", HEAD_PARAM_SHAPES[n]) for i, t in enumerate(params[n])]))
        else:
            args.append(_head_operand(params[n], n, HEAD_PARAM_SHAPES[n]))
    return args


def _head_partial(partial, B: int, world: int, device, what: str) -> torch.Tensor:
    need = max(world, 1) * ((B + 15) // 16) * 2 * 256
    if partial is None:
        return torch.empty(need, device=device, dtype=torch.float32)
    if _chk(partial, "partial").numel() < need or not partial.is_contiguous():
        raise RuntimeError(f"{what}: partial must hold at least {need} contiguous floats, got {partial.numel()}")
    return partial


def head_fwd(comb: torch.Tensor, params: dict, running_mean: torch.Tensor, running_var: torch.Tensor, training: bool, concat: bool = False,
             world: int = 1, rank: int = 0, partial: Optional[torch.Tensor] = None, fusion_out=None) -> dict:
    """Fusion block + regression head, forward (``bbbp_head_fwd``).  ``params``: HEAD_PARAM_SHAPES (the fusion entries may be missing when
    ``concat``).  Returns every tensor the kernels write, by name: hid, attn, fused (None when ``concat``, unless ``fusion_out`` hands in
    three buffers, which must then stay untouched), h, hb, bn_mean, bn_rstd, h2, h3, out; the running statistics are updated in place when
    training.  ``partial``: the block-partial workspace, shared between the ranks' calls when ``world`` > 1."""
    if _chk(comb, "comb").dim() != 2 or comb.shape[1] != 256 or not comb.is_contiguous():
        raise RuntimeError(f"head_fwd: comb must be a contiguous [B, 256] tensor, got shape {tuple(comb.shape)} strides {comb.stride()}")
    B, dev = comb.shape[0], comb.device
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    fusion = [None] * 4 if concat else _head_params(params, _HEAD_PER_HEAD, "head_fwd")
    head = _head_params(params, ("w0", "b0", "gamma", "beta"), "head_fwd") + [_head_operand(running_mean, "running_mean", (256,)),
                                                                               _head_operand(running_var, "running_var", (256,))]
    head += _head_params(params, ("w3", "b3", "w5", "b5", "w7", "b7"), "head_fwd")
    o = {}
    if fusion_out is not None:
        o["hid"], o["attn"], o["fused"] = fusion_out
        for n, shape in (("hid", (4, B, 128)), ("attn", (B, 4)), ("fused", (B, 256))):
            _head_operand(o[n], n, shape)
    elif concat:
        o["hid"] = o["attn"] = o["fused"] = None
    else:
        o["hid"], o["attn"], o["fused"] = new(4, B, 128), new(B, 4), new(B, 256)
    o.update(h=new(B, 256), hb=new(B, 256), bn_mean=new(256), bn_rstd=new(256), h2=new(B, 128), h3=new(B, 64), out=new(B))
    partial = _head_partial(partial, B, world, dev, "head_fwd")
    _lib.check(_lib.lib().bbbp_head_fwd(_stream(), comb.data_ptr(), *fusion, *head, *[_p(o[n]) for n in (
        "hid", "attn", "fused", "h", "hb", "bn_mean", "bn_rstd", "h2", "h3", "out")], partial.data_ptr(), B, int(training), int(concat),
        world, rank), "bbbp_head_fwd")
    return o


def head_bwd(dout: torch.Tensor, comb: torch.Tensor, saved: dict, params: dict, training: bool, world: int = 1, rank: int = 0,
             partial: Optional[torch.Tensor] = None) -> dict:
    """Input-gradient chain of the fusion block + head (``bbbp_head_bwd``).  ``saved``: hid, attn, h, h2, h3, bn_mean, bn_rstd as
    ``head_fwd`` returns them -- or any tensors of those shapes: they are taken as given.  Returns dh3, dh2, dhb, dh, dlogit [4, B],
    dpre [4, B, 128], dcomb, dgamma, dbeta by name."""
    if _chk(comb, "comb").dim() != 2 or comb.shape[1] != 256 or not comb.is_contiguous():
        raise RuntimeError(f"head_bwd: comb must be a contiguous [B, 256] tensor, got shape {tuple(comb.shape)} strides {comb.stride()}")
    B, dev = comb.shape[0], comb.device
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    ins = [_head_operand(dout, "dout", (B,)), comb.data_ptr()]
    ins += [_head_operand(saved[n], n, shape) for n, shape in (("hid", (4, B, 128)), ("attn", (B, 4)), ("h", (B, 256)), ("h2", (B, 128)),
                                                                ("h3", (B, 64)), ("bn_mean", (256,)), ("bn_rstd", (256,)))]
    ins += _head_params(params, ("gamma", "fw1", "fw2", "w0", "w3", "w5", "w7"), "head_bwd")
    o = dict(dh3=new(B, 64), dh2=new(B, 128), dhb=new(B, 256), dh=new(B, 256), dlogit=new(4, B), dpre=new(4, B, 128), dcomb=new(B, 256),
             dgamma=new(256), dbeta=new(256))
    partial = _head_partial(partial, B, world, dev, "head_bwd")
    _lib.check(_lib.lib().bbbp_head_bwd(_stream(), *ins, *[t.data_ptr() for t in o.values()], partial.data_ptr(), B, int(training), world,
                                        rank), "bbbp_head_bwd")
    return o


def mse(pred: torch.Tensor, target: torch.Tensor, grad_scale: float = 1.0):
    """Returns (loss[1], dpred) for loss = mean((pred - target)^2)."""
    pred = _chk(pred, "pred").contiguous().view(-1)
    target = _chk(target, "target").contiguous().view(-1)
    if target.numel() != pred.numel():
        raise RuntimeError(f"mse: pred has {pred.numel()} elements, target {target.numel()}")
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred)
    _lib.check(_lib.lib().bbbp_mse(_stream(), pred.data_ptr(), target.data_ptr(), loss.data_ptr(), dpred.data_ptr(),
                                   pred.numel(), grad_scale), "bbbp_mse")
    return loss, dpred


def adamw_step_(param, grad, exp_avg, exp_avg_sq, step: int, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5,
                grad_scale: float = 1.0) -> None:
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, n)
        if not t.is_contiguous():
            raise RuntimeError(f"adamw: {n} must be contiguous")
    _lib.check(_lib.lib().bbbp_adamw_step(_stream(), param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
                                          exp_avg_sq.data_ptr(), param.numel(), lr, betas[0], betas[1], eps, weight_decay,
                                          step, grad_scale), "bbbp_adamw_step")


def adamw_step_deferred_(param, grad, exp_avg, exp_avg_sq, step: int, lo: int, hi: int, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5,
                         grad_scale: float = 1.0) -> None:
    """``adamw_step_`` with elements [lo, hi) of the flat buffers updated on a library-owned side stream (``bbbp_adamw_step_deferred``):
    the next ``MixedInputModel`` forward waits for that slice right before it reads it; ``param_sync()`` orders anything else."""
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, n)
        if not t.is_contiguous():
            raise RuntimeError(f"adamw: {n} must be contiguous")
    _lib.check(_lib.lib().bbbp_adamw_step_deferred(_stream(), param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                                   param.numel(), lo, hi, lr, betas[0], betas[1], eps, weight_decay, step, grad_scale),
               "bbbp_adamw_step_deferred")
    # torch's caching allocator is stream-ordered: the gradient buffer is usually freed (zero_grad(set_to_none=True)) while the side stream may
    # still read it -- tell the allocator, or the block could be handed to the next allocation on the current stream too early
    h = _lib.lib().bbbp_param_stream()
    if h:
        side = torch.cuda.ExternalStream(int(h), device=param.device)
        grad.record_stream(side)                 # (parameters and moments live as long as the optimizer)


def adamw_hyper_store_(hyper, step: int, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, grad_scale: float = 1.0) -> None:
    """Store the eight derived floats the AdamW kernels compute with into the 8-float device tensor ``hyper``, in stream order
    (``bbbp_adamw_hyper_store``)."""
    _chk(hyper, "hyper")
    if hyper.numel() != 8 or not hyper.is_contiguous():
        raise RuntimeError("adamw_hyper_store: hyper must be 8 contiguous float32 values")
    _lib.check(_lib.lib().bbbp_adamw_hyper_store(_stream(), hyper.data_ptr(), lr, betas[0], betas[1], eps, weight_decay, step, grad_scale),
               "bbbp_adamw_hyper_store")


def adamw_step_multi_(param, exp_avg, exp_avg_sq, table, n_tensors: int, step: int, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5,
                      grad_scale: float = 1.0, hyper=None) -> None:
    """One launch over a flat parameter / moment buffer whose gradients are ``n_tensors`` separate tensors (``bbbp_adamw_step_multi``).
    ``table``: int64 device tensor, ``n_tensors + 1`` element offsets followed by ``n_tensors`` gradient addresses.  ``hyper``: optional
    8-float device tensor (``adamw_hyper_store_``) read by the kernel instead of the scalar arguments."""
    for t, n in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, n)
        if not t.is_contiguous():
            raise RuntimeError(f"adamw: {n} must be contiguous")
    if table.dtype != torch.int64 or not table.is_cuda or table.numel() != 2 * n_tensors + 1 or not table.is_contiguous():
        raise RuntimeError("adamw_multi: table must be a contiguous int64 CUDA tensor of 2 * n_tensors + 1 entries")
    if hyper is not None and (hyper.dtype != torch.float32 or not hyper.is_cuda or hyper.numel() != 8):
        raise RuntimeError("adamw_multi: hyper must be 8 float32 values on the device")
    _lib.check(_lib.lib().bbbp_adamw_step_multi(_stream(), param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.numel(),
                                                table.data_ptr(), n_tensors, lr, betas[0], betas[1], eps, weight_decay, step, grad_scale,
                                                hyper.data_ptr() if hyper is not None else None), "bbbp_adamw_step_multi")


def param_sync() -> None:
    """Order the current stream behind a deferred optimizer slice (no-op when none is pending)."""
    _lib.check(_lib.lib().bbbp_param_sync(_stream()), "bbbp_param_sync")
