"""GPU: the six kernel families of csrc/attention.hip and csrc/attention_b3.hip, called directly (ops.attention_fwd / attention_bwd /
attention_b3_fwd) and compared element-wise with the float64 oracle of tests/attention_oracle.py: ctx, logsumexp and every element of dqkv.

Which kernel a shape reaches (``small_dispatch`` restates the launcher's rules; the tests that exist for one branch assert it):
  * head_dim 8 / 16, nhead > 1: attn_small_fwd_kernel<2 / 4> on nhead x fwd_parts work-groups; backward on attn_small_bwd1_kernel (one
    work-group per head) when head_parts == 1, B <= 512 and (p == 0 or the keep bytes are passed), else attn_small_bwd_kernel (two sweeps)
    on nhead x head_parts work-groups;
  * head_dim 161 .. 176, nhead <= 8: attn_wide_fwd_kernel / attn_wide_bwd_kernel;
  * attention_b3_fwd: attn_b3_fwd_kernel, plus attn_b3_merge_kernel when the key axis is split (workspace bytes > 0).
Ordinary inputs meet the project's bound for float32 kernels against float64; the large-logit regimes are held to what float32 can give
on the same input (helpers.assert_close_or_as_accurate_as_fp32 against the oracle's float32 evaluation)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attention_oracle as A
from bbbp_amd import _lib, ops
from helpers import assert_close, assert_close_or_as_accurate_as_fp32

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol_frac=2e-5)          # float32 kernels against float64, as _conv_case / _layernorm_case
HIGH_SEED = 2 ** 32 + 5


def small_dispatch(nhead, D, B, p=0.0, keep=False):
    """(fwd_parts, head_parts, single-sweep backward?) as csrc/attention.hip's launcher decides them with its knobs at their defaults."""
    blocks = (B + 15) // 16
    per = (blocks + 7) // 8
    head_parts = max(1, min(256 // nhead, per, 16))
    fwd_parts = max(1, min(512 // nhead, per, 16))
    bwd1_lds = (4 * blocks * 16 * (D + 1) + 2 * blocks * 16 + 2 * 8 * 256) * 4
    return fwd_parts, head_parts, (p == 0 or keep) and head_parts == 1 and blocks <= 32 and bwd1_lds <= 160 * 1024


@functools.lru_cache(maxsize=None)
def reference(nhead, D, B, regime="ordinary", p=0.0, seed=0, base=None, f32=False, backward=True):
    """Inputs and float64 results of one case (computed once, shared, read-only); ``f32``: the float32 evaluation too."""
    qkv, dctx = A.inputs(nhead, D, B, regime)
    r = SimpleNamespace(qkv=qkv, dctx=dctx, nhead=nhead, D=D, B=B, F=nhead * D, p=p, seed=seed, base=base,
                        what=f"nhead={nhead} head_dim={D} B={B} {regime} p={p}")
    r.ctx, r.lse, _, _ = A.forward(qkv, nhead, p=p, seed=seed, base=base, full=False)
    r.dqkv = A.backward(qkv, dctx, nhead, p=p, seed=seed, base=base) if backward else None
    if f32:
        r.ctx32, r.lse32, _, _ = A.forward(qkv, nhead, p=p, seed=seed, base=base, dtype=np.float32, full=False)
        r.dqkv32 = A.backward(qkv, dctx, nhead, p=p, seed=seed, base=base, dtype=np.float32) if backward else None
    for v in vars(r).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def T(a, dev):
    return torch.tensor(a).to(dev)           # a copy: the cached references are read-only


def N(t):
    return t.detach().cpu().numpy()


def run(dev, r, keep_mask=False, bwd_keep=True, backward=True):
    """(ctx, lse, dqkv, keep) of the device ops on a case's inputs, as torch tensors; ``bwd_keep=False``: backward redraws the stream."""
    qkv, dctx = T(r.qkv, dev), T(r.dctx, dev)
    ctx, lse, keep = ops.attention_fwd(qkv, r.nhead, dropout_p=r.p, seed=r.seed, keep_mask=keep_mask)
    dqkv = ops.attention_bwd(qkv, ctx, lse, dctx, r.nhead, dropout_p=r.p, seed=r.seed, keep=keep if bwd_keep else None) if backward else None
    return ctx, lse, dqkv, keep


def thirds(dqkv, F):
    return (("dQ", dqkv[:, :F]), ("dK", dqkv[:, F:2 * F]), ("dV", dqkv[:, 2 * F:]))


def check_ordinary(r, ctx, lse, dqkv):
    assert_close(N(ctx), r.ctx, what=r.what + " ctx", **TOL)
    assert_close(N(lse), r.lse, what=r.what + " lse", **TOL)
    if dqkv is not None:
        # one tensor, one floor: at B = 1 dQ and dK are exactly 0 and float32 leaves rounding residue of dP - delta there
        assert_close(N(dqkv), r.dqkv, what=r.what + " dqkv", **TOL)


def as_accurate_as_fp32(got, want64, want32, what):
    """Finite, and within the float64 oracle's tolerance or no worse than 2 x the float32 evaluation of the same input; prints both errors."""
    got = np.asarray(got, dtype=np.float64)
    err, ref = float(np.abs(got - want64).max()), float(np.abs(want32.astype(np.float64) - want64).max())
    print(f"[fp32-yardstick] {what}: kernel {err:.3e} float32 {ref:.3e} ratio {err / ref if ref else float('inf'):.2f} "
          f"scale {np.abs(want64).max():.3e}")
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements are not finite"
    assert_close_or_as_accurate_as_fp32(got, want64, want32, what=what)


def check_large(r, ctx, lse, dqkv):
    as_accurate_as_fp32(N(ctx), r.ctx, r.ctx32, r.what + " ctx")
    as_accurate_as_fp32(N(lse), r.lse, r.lse32, r.what + " lse")
    if dqkv is not None:
        # dqkv as ONE tensor, as in check_ordinary.  dS = P o (dP - delta) is a difference of O(|dP|) terms, and dQ = dS K sums it against key
        # rows that share a large component in the offset regimes: what float32 leaves in dQ and dK scales with |dP| |K|, i.e. with dqkv as a
        # whole, not with their own size -- which is ~1e-15 for one-hot rows, where only an evaluation that takes delta from the very same
        # dP array (the oracle's; the kernels take it from dO . O, flash-style) cancels exactly.  The thirds are printed for the record.
        got = N(dqkv)
        for (name, g), (_, want), (_, want32) in zip(thirds(got, r.F), thirds(r.dqkv, r.F), thirds(r.dqkv32, r.F)):
            print(f"[thirds] {r.what} {name}: kernel {np.abs(g - want).max():.3e} float32 {np.abs(want32 - want).max():.3e} scale {np.abs(want).max():.3e}")
        as_accurate_as_fp32(got, r.dqkv, r.dqkv32, r.what + " dqkv")


# ---- small heads ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 37, 128, 129, 200])
@pytest.mark.parametrize("nhead,D", [(2, 8), (8, 8), (2, 16), (8, 16)])
def test_small_head_kernels_against_float64(dev, nhead, D, B):
    """B <= 128: one forward chunk, single-sweep backward; B = 129: a second forward chunk of one key and a head split over two work-groups
    (two-sweep backward); B = 200: two work-groups per head, 13 tiles."""
    r = reference(nhead, D, B)
    fwd_parts, head_parts, bwd1 = small_dispatch(nhead, D, B)
    assert bwd1 == (B <= 128) and head_parts == fwd_parts == (1 if B <= 128 else 2)
    check_ordinary(r, *run(dev, r)[:3])


@pytest.mark.parametrize("nhead,D,B,bwd1", [(256, 8, 129, True), (256, 8, 512, True), (256, 8, 513, False), (256, 16, 200, True)])
def test_many_small_heads_against_float64(dev, nhead, D, B, bwd1):
    """256 heads (the F = 2048 encoder): the single-sweep backward with more than eight key tiles -- waves own 1 and 2 tiles at B = 129, 4 at
    B = 512 -- and B = 513, the first batch that falls back to the two-sweep kernel."""
    assert small_dispatch(nhead, D, B) == (min(2, (B + 127) // 128), 1, bwd1)
    r = reference(nhead, D, B)
    check_ordinary(r, *run(dev, r)[:3])


def test_small_head_support_limit(dev):
    """(2, 8) at B = 960: the largest LDS request (bwd_lds = 159.5 of 160 KB, on 2 x 8 work-groups); one row more is refused before any launch."""
    L = _lib.lib()
    assert [L.bbbp_attention_supported(B, 2, 8) for B in (960, 961)] == [1, 0]
    assert [L.bbbp_attention_supported(B, 2, 16) for B in (512, 513)] == [1, 0]
    r = reference(2, 8, 960)
    check_ordinary(r, *run(dev, r)[:3])
    for nhead, D, B in ((2, 8, 961), (2, 16, 513), (2, 12, 37), (9, 167, 37), (1, 8, 37)):
        qkv = torch.zeros(B, 3 * nhead * D, device=dev)
        with pytest.raises(RuntimeError, match="not supported"):
            ops.attention_fwd(qkv, nhead)
        with pytest.raises(RuntimeError, match="not supported"):
            ops.attention_bwd(qkv, qkv[:, :nhead * D].contiguous(), torch.zeros(nhead, B, device=dev), qkv[:, :nhead * D].contiguous(), nhead)
    for nhead, D in ((1, 96), (1, 193), (17, 100)):
        with pytest.raises(RuntimeError, match="not supported"):
            ops.attention_b3_fwd(torch.zeros(37, 3 * nhead * D, device=dev), nhead)
    torch.cuda.synchronize()


# ---- wide heads -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16, 17, 37, 129, 200])
@pytest.mark.parametrize("nhead,D", [(1, 167), (1, 161), (1, 176), (2, 167), (3, 164), (8, 167)])
def test_wide_head_kernels_against_float64(dev, nhead, D, B):
    """Both ends of the head_dim range, and nhead > 1: heads at odd float offsets h * 167 of a row."""
    assert _lib.lib().bbbp_attention_supported(B, nhead, D) & 3 == 2
    r = reference(nhead, D, B)
    check_ordinary(r, *run(dev, r)[:3])


# ---- split-bf16 forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 128, 129, 257, 600])
@pytest.mark.parametrize("nhead,D", [(1, 167), (1, 97), (1, 128), (1, 192), (2, 167), (16, 100)])
def test_b3_forward_against_float64_and_the_float32_kernel(dev, nhead, D, B):
    """B = 257: two key ranges, the second ragged (97 keys); B = 600: three -- the merge kernel runs."""
    L = _lib.lib()
    assert L.bbbp_attention_supported(B, nhead, D) & 4
    wsb = L.bbbp_attention_b3_workspace_bytes(B, nhead, D)
    assert (wsb > 0) == (B > 256)
    r = reference(nhead, D, B, f32=True, backward=False)
    qkv = T(r.qkv, dev)
    ctx = ops.attention_b3_fwd(qkv, nhead)
    assert_close(N(ctx), r.ctx, what=r.what + " b3 ctx", **TOL)
    if L.bbbp_attention_supported(B, nhead, D) & 2:
        f32 = N(ops.attention_fwd(qkv, nhead)[0]).astype(np.float64)
        # two float32 results: apart by no more than the float32 evaluation is from float64 (the helper's yardstick, moved onto the kernel)
        as_accurate_as_fp32(N(ctx), f32, f32 + (r.ctx32 - r.ctx), r.what + " b3 ctx against attention_fwd")


# ---- logit regimes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", A.LARGE)
@pytest.mark.parametrize("B", A.REGIME_BS)
@pytest.mark.parametrize("nhead,D", A.REGIME_HEADS["small"])
def test_small_head_kernels_in_the_large_logit_regimes(dev, nhead, D, B, regime):
    """p = 0: forward and the single-sweep backward at B = 32 (full tiles) and 37 (ragged), the two-sweep backward at B = 129."""
    assert small_dispatch(nhead, D, B)[2] == (B < 129)
    r = reference(nhead, D, B, regime, f32=True)
    check_large(r, *run(dev, r)[:3])


@pytest.mark.parametrize("regime", A.LARGE)
@pytest.mark.parametrize("B", A.REGIME_BS[:2])
@pytest.mark.parametrize("nhead,D", A.REGIME_HEADS["small"])
def test_two_sweep_backward_in_the_large_logit_regimes(dev, nhead, D, B, regime):
    """At these batches the two-sweep kernel is reached through dropout without saved decisions (the oracle applies the exact mask)."""
    assert not small_dispatch(nhead, D, B, p=0.1, keep=False)[2]
    r = reference(nhead, D, B, regime, p=0.1, seed=11, f32=True)
    check_large(r, *run(dev, r, keep_mask=False)[:3])


@pytest.mark.parametrize("regime", ["neg95", "pos95", "max_last"])
def test_single_sweep_backward_with_a_ragged_second_tile_in_the_large_logit_regimes(dev, regime):
    """256 heads at B = 129: the ragged last key tile is tile 8, the second tile of wave 0."""
    nhead, D, B = A.REGIME_MANY_HEADS
    assert small_dispatch(nhead, D, B)[2]
    r = reference(nhead, D, B, regime, f32=True)
    check_large(r, *run(dev, r)[:3])


@pytest.mark.parametrize("regime", A.LARGE)
@pytest.mark.parametrize("B", A.REGIME_BS)
@pytest.mark.parametrize("nhead,D", A.REGIME_HEADS["wide"])
def test_wide_head_kernels_in_the_large_logit_regimes(dev, nhead, D, B, regime):
    r = reference(nhead, D, B, regime, f32=True)
    check_large(r, *run(dev, r)[:3])


@pytest.mark.parametrize("regime", A.LARGE)
@pytest.mark.parametrize("B", A.REGIME_BS)
@pytest.mark.parametrize("nhead,D", A.REGIME_HEADS["b3"])
def test_b3_forward_in_the_large_logit_regimes(dev, nhead, D, B, regime):
    r = reference(nhead, D, B, regime, f32=True, backward=False)
    as_accurate_as_fp32(N(ops.attention_b3_fwd(T(r.qkv, dev), nhead)), r.ctx, r.ctx32, r.what + " b3 ctx")


# ---- dropout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, HIGH_SEED])
@pytest.mark.parametrize("B", [36, 37])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("nhead,D", [(2, 8), (2, 16), (1, 167), (2, 167)])
def test_dropout_is_the_oracles_stream(dev, nhead, D, p, B, seed):
    """Element (h B + q) B + k of the Philox stream: rows start at multiples of 4 at B = 36 (one block per keep4) and anywhere at B = 37 (two).
    Every element of ctx and dqkv against the oracle under the exact mask; the saved decisions are the oracle's mask bit for bit; backward
    from the saved bytes (single sweep) and from the redrawn stream (two sweeps) agree."""
    r = reference(nhead, D, B, p=p, seed=seed)
    ctx, lse, dqkv, keep = run(dev, r, keep_mask=True)
    check_ordinary(r, ctx, lse, dqkv)
    redrawn = run(dev, r, keep_mask=False)
    assert torch.equal(redrawn[0], ctx) and torch.equal(redrawn[1], lse)
    check_ordinary(r, *redrawn[:3])
    if D <= 16:
        assert small_dispatch(nhead, D, B, p, keep=True)[2] and not small_dispatch(nhead, D, B, p, keep=False)[2]
        _, _, _, mask = A.forward(r.qkv, nhead, p=p, seed=seed)
        assert keep.numel() == _lib.lib().bbbp_attention_keep_bytes(B, nhead, D) > 0
        assert np.array_equal(A.decode_keep(N(keep), nhead, B), mask != 0)
        assert 0.5 * p < 1 - (mask != 0).mean() < 1.5 * p
        assert_close(N(redrawn[2]), N(dqkv), what=r.what + " dqkv: redrawn stream against saved decisions", **TOL)
    else:
        assert keep is None and torch.equal(redrawn[2], dqkv)          # the wide kernels always redraw


@pytest.mark.parametrize("nhead,D", [(2, 8), (1, 167)])
def test_dropout_under_a_seed_base(dev, nhead, D):
    B, p, seed, base = 37, 0.1, HIGH_SEED, 2 ** 40 + 7
    r = reference(nhead, D, B, p=p, seed=seed, base=base)
    base_t = torch.full((1,), base, dtype=torch.int64, device=dev)
    ops.set_seed_base(base_t.data_ptr())
    try:
        ctx, lse, dqkv, keep = run(dev, r, keep_mask=True)
        redrawn = run(dev, r, keep_mask=False)
    finally:
        ops.set_seed_base(0)
    check_ordinary(r, ctx, lse, dqkv)
    check_ordinary(r, *redrawn[:3])
    if keep is not None:
        assert np.array_equal(A.decode_keep(N(keep), nhead, B), A.forward(r.qkv, nhead, p=p, seed=seed, base=base)[3] != 0)
    plain = reference(nhead, D, B, p=p, seed=seed)                     # restored: no base
    check_ordinary(plain, *run(dev, plain)[:3])


@pytest.mark.parametrize("nhead,D,B", [(2, 8, 37), (2, 16, 36)])
def test_no_dropout_with_a_keep_pointer_behaves_as_with_none(dev, nhead, D, B):
    r = reference(nhead, D, B)
    with_keep, without = run(dev, r, keep_mask=True), run(dev, r, keep_mask=False)
    assert with_keep[3] is not None and without[3] is None
    for a, b in zip(with_keep[:3], without[:3]):
        assert torch.equal(a, b)
    check_ordinary(r, *with_keep[:3])


# ---- determinism --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhead,D,B,p,keep_mask", [(2, 8, 37, 0.0, False), (2, 8, 37, 0.1, True), (2, 8, 37, 0.1, False), (8, 16, 200, 0.0, False),
                                                   (256, 8, 129, 0.0, False), (2, 167, 37, 0.0, False), (1, 167, 200, 0.1, False)])
def test_two_calls_are_bit_identical(dev, nhead, D, B, p, keep_mask):
    """No atomics, a fixed summation order: every family returns the same bits twice (forward, both backward kernels, wide)."""
    r = reference(nhead, D, B, p=p, seed=3)
    first, second = run(dev, r, keep_mask=keep_mask), run(dev, r, keep_mask=keep_mask)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("nhead,D,B", [(1, 167, 37), (1, 167, 257), (16, 100, 600)])
def test_two_b3_calls_are_bit_identical(dev, nhead, D, B):
    """... and the split-bf16 forward with its merge pass (ranges summed in range order)."""
    qkv = T(reference(nhead, D, B, backward=False).qkv, dev)
    assert torch.equal(ops.attention_b3_fwd(qkv, nhead), ops.attention_b3_fwd(qkv, nhead))
