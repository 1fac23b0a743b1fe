"""GPU: ops.attention_fwd / attention_bwd / attention_b3_fwd with every output, the keep bytes and the split-bf16 workspace allocated from
poisoned, guarded pools (tests/poison.py) and the operands inside moats at an odd base: one ragged shape per kernel family.  Under each fill
the results are bit-equal to the run on ordinary allocations -- a difference is a read of memory the call does not own, or of an output
element it never wrote -- every guard band and moat is intact, and the results still meet the float64 oracle."""
import pytest
import torch

from bbbp_amd import _lib, ops
from poison import moated, poisoned_allocations
from helpers import assert_close
from test_gpu_attention import N, TOL, check_ordinary, reference
from test_gpu_poison_ops import RUNS, same_bits

pytestmark = pytest.mark.gpu


def _fwd_bwd(r, qkv, dctx, keep_mask):
    """(ctx, lse, keep, dqkv from the saved decisions, dqkv from the redrawn stream)"""
    ctx, lse, keep = ops.attention_fwd(qkv, r.nhead, dropout_p=r.p, seed=r.seed, keep_mask=keep_mask)
    saved = ops.attention_bwd(qkv, ctx, lse, dctx, r.nhead, dropout_p=r.p, seed=r.seed, keep=keep)
    redrawn = ops.attention_bwd(qkv, ctx, lse, dctx, r.nhead, dropout_p=r.p, seed=r.seed, keep=None)
    torch.cuda.synchronize()
    return ctx, lse, (keep if r.p > 0 else None), saved, redrawn           # without dropout the keep bytes are passed along, never written


def _under_every_fill(dev, monkeypatch, host_operands, call, what):
    """``call(*device operands)`` on ordinary allocations, then under each fill with the operands moated one element off a 256-byte boundary."""
    plain = call(*(t.to(dev) for t in host_operands))
    for name, fill in RUNS:
        held = [moated(t, fill, offset=1, device=dev) for t in host_operands]
        with poisoned_allocations(monkeypatch, fill) as pa:
            outs = call(*(view for view, _ in held))
        assert pa.check() >= len([t for t in outs if t is not None]), f"{what}: an output did not come from the pools"
        for _, check in held:
            check()
        for i, (a, b) in enumerate(zip(plain, outs)):
            assert (a is None) == (b is None)
            if a is not None:
                assert same_bits(a, b), f"{what}: returned tensor {i} under {name} differs from the run on ordinary allocations"
                assert a.dtype == torch.uint8 or bool(b.isfinite().all()), f"{what}: returned tensor {i} is not finite under {name}"
        pa.release()
    return plain


@pytest.mark.parametrize("nhead,D,p", [(2, 8, 0.0), (2, 8, 0.1), (1, 167, 0.0), (1, 167, 0.1)], ids=["small", "small-dropout", "wide", "wide-dropout"])
def test_attention_fwd_bwd_under_poison(dev, monkeypatch, nhead, D, p):
    """B = 37: two full tiles and a ragged one.  Small heads: the single-sweep backward (saved decisions) and the two-sweep backward (redrawn)."""
    r = reference(nhead, D, 37, p=p, seed=9)
    keep_mask = D <= 16
    ctx, lse, keep, saved, redrawn = _under_every_fill(dev, monkeypatch, (torch.tensor(r.qkv), torch.tensor(r.dctx)),
                                                       lambda qkv, dctx: _fwd_bwd(r, qkv, dctx, keep_mask), r.what)
    assert (keep is not None) == (keep_mask and p > 0) and (keep is None or keep.numel() == _lib.lib().bbbp_attention_keep_bytes(37, nhead, D))
    check_ordinary(r, ctx, lse, saved)
    check_ordinary(r, ctx, lse, redrawn)


def test_attention_b3_fwd_under_poison(dev, monkeypatch):
    """(1, 167) at B = 257: two key ranges, the second ragged; the partial (O, max, sum) triples live in a poisoned workspace."""
    r = reference(1, 167, 257, backward=False)
    assert _lib.lib().bbbp_attention_b3_workspace_bytes(257, 1, 167) > 0

    def call(qkv):
        out = ops.attention_b3_fwd(qkv, 1)
        torch.cuda.synchronize()
        return (out,)
    ctx, = _under_every_fill(dev, monkeypatch, (torch.tensor(r.qkv),), call, r.what + " b3")
    assert_close(N(ctx), r.ctx, what=r.what + " b3 ctx", **TOL)
