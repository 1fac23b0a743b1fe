"""CPU: tests/attention_oracle.py pinned to torch -- the yardstick of tests/test_gpu_attention.py must itself be right -- and the host-side
argument checks of the attention entry points (no launch is reached)."""
import ctypes

import numpy as np
import pytest
import torch

import attention_oracle as A
import rowops_oracle as R
from bbbp_amd import _lib

PINNED = [(2, 8, 37), (8, 16, 17), (3, 164, 17), (1, 97, 33), (2, 8, 1)]


def _torch_heads(qkv, nhead):
    B, F, D = A.shape_of(qkv, nhead)
    t = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    q, k, v = (t[:, i * F:(i + 1) * F].reshape(B, nhead, D).transpose(0, 1) for i in range(3))       # [nhead, B, D]
    return t, q, k, v


@pytest.mark.parametrize("nhead,D,B", PINNED)
def test_oracle_matches_torch_sdpa_and_autograd(nhead, D, B):
    qkv, dctx = A.inputs(nhead, D, B)
    t, q, k, v = _torch_heads(qkv, nhead)
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v)                                    # default scale D ** -0.5
    ctx_t = out.transpose(0, 1).reshape(B, nhead * D)
    ctx_t.backward(torch.from_numpy(dctx.astype(np.float64)))
    lse_t = torch.logsumexp(q @ k.transpose(1, 2) * D ** -0.5, dim=2)
    ctx, lse, prob, keep = A.forward(qkv, nhead)
    assert keep is None and prob.shape == (nhead, B, B)
    np.testing.assert_allclose(prob.sum(axis=2), 1.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(ctx, ctx_t.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(lse, lse_t.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(A.backward(qkv, dctx, nhead), t.grad.numpy(), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("nhead,D,B", PINNED[:4])
@pytest.mark.parametrize("p,seed,base", [(0.1, 7, None), (0.5, 2 ** 32 + 5, 2 ** 40 + 7)])
def test_oracle_dropout_matches_a_masked_softmax_in_torch(nhead, D, B, p, seed, base):
    """The mask of a [nhead, B, B] probability tensor as rowops_oracle states it for any contiguous tensor (element i draws word i): the
    same stream position as (h B + q) B + k."""
    qkv, dctx = A.inputs(nhead, D, B, seed=1)
    keep_t = R.keep_scale_like(np.empty((nhead, B, B), np.float32), p, seed, base)
    t, q, k, v = _torch_heads(qkv, nhead)
    pd = torch.softmax(q @ k.transpose(1, 2) * D ** -0.5, dim=2) * torch.from_numpy(keep_t.astype(np.float64))
    ctx_t = (pd @ v).transpose(0, 1).reshape(B, nhead * D)
    ctx_t.backward(torch.from_numpy(dctx.astype(np.float64)))
    ctx, _, _, keep = A.forward(qkv, nhead, p=p, seed=seed, base=base)
    assert keep.dtype == np.float32 and np.array_equal(keep, keep_t)
    assert set(np.unique(keep)) <= {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    np.testing.assert_allclose(ctx, ctx_t.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(A.backward(qkv, dctx, nhead, p=p, seed=seed, base=base), t.grad.numpy(), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("nhead,D,B", A.REGIME_SHAPES)
@pytest.mark.parametrize("regime", A.LARGE)
def test_large_logit_inputs_have_the_range_they_claim(nhead, D, B, regime):
    qkv, _ = A.inputs(nhead, D, B, regime)
    _, lse, prob, _ = A.forward(qkv, nhead)
    F = nhead * D
    q, k = (qkv[:, i * F:(i + 1) * F].astype(np.float64).reshape(B, nhead, D).transpose(1, 0, 2) for i in range(2))
    s = q @ k.transpose(0, 2, 1) * D ** -0.5
    if regime == "neg95":
        assert s.max() <= -95 and lse.max() <= -95
    elif regime == "pos95":
        assert s.min() >= 95 and lse.min() >= 95
    elif regime == "std30":
        assert 24 <= s.std() <= 36
        assert np.median(prob.max(axis=2)) > 0.9                    # near-one-hot rows
    else:
        at = B - 1 if regime == "max_last" else 0
        rest = np.delete(s, at, axis=2)
        assert (s.argmax(axis=2) == at).all()
        if B > 1:
            assert (s[:, :, at] - rest.max(axis=2)).min() >= 20       # whatever came before it is rescaled by exp(-20) at the most


@pytest.mark.parametrize("nhead,D,B", A.REGIME_SHAPES)
@pytest.mark.parametrize("regime", A.LARGE)
def test_float32_yardstick_is_finite_and_within_its_stated_error(nhead, D, B, regime):
    qkv, dctx = A.inputs(nhead, D, B, regime)
    ctx, lse, _, _ = A.forward(qkv, nhead, full=False)
    ctx32, lse32, _, _ = A.forward(qkv, nhead, dtype=np.float32, full=False)
    d32 = A.backward(qkv, dctx, nhead, dtype=np.float32)
    assert ctx32.dtype == lse32.dtype == d32.dtype == np.float32
    assert np.isfinite(ctx32).all() and np.isfinite(lse32).all() and np.isfinite(d32).all()
    ctx_b, lse_b = A.fp32_error_bound(qkv, nhead)
    assert np.abs(ctx32 - ctx).max() <= ctx_b, (np.abs(ctx32 - ctx).max(), ctx_b)
    assert np.abs(lse32 - lse).max() <= lse_b, (np.abs(lse32 - lse).max(), lse_b)
    assert ctx_b <= 0.01 * np.abs(qkv[:, 2 * nhead * D:]).max()        # a worst-case bound, but not a vacuous one: 1 % of max |V|


@pytest.mark.parametrize("nhead,B", [(1, 1), (2, 16), (3, 37), (2, 129)])
def test_keep_byte_decoder_against_a_brute_force_loop(nhead, B):
    nt = (B + 15) // 16
    raw = np.random.default_rng(B).integers(0, 16, size=nhead * nt * nt * 64, dtype=np.uint8)
    got = A.decode_keep(raw, nhead, B)
    assert got.shape == (nhead, B, B) and got.dtype == bool
    for h in range(nhead):
        for query in range(B):
            for key in range(B):
                qb, q, kt, kq, r = query // 16, query % 16, key // 16, (key % 16) // 4, key % 4
                byte = raw[((h * nt + qb) * nt + kt) * 64 + 16 * kq + q]
                assert got[h, query, key] == bool((byte >> r) & 1)


def test_supported_shapes_and_argument_errors_without_a_gpu():
    """bbbp_attention_supported follows bwd_lds <= 160 KB for the small-head kernels and the head_dim ranges of the other two; every
    unsupported or malformed call returns BBBP_ERR_ARG before anything is launched (the pointers here are never dereferenced)."""
    L = _lib.lib()
    sup = L.bbbp_attention_supported
    assert [sup(B, 2, 8) for B in (1, 960, 961)] == [1, 1, 0]
    assert [sup(B, 2, 16) for B in (512, 513)] == [1, 0]
    assert sup(37, 1, 8) == 0 and sup(37, 2, 12) == 0                                       # one head is never "small"; head_dim 8 or 16 only
    assert [sup(37, 1, D) for D in (96, 97, 160, 161, 167, 176, 177, 192, 193)] == [0, 4, 4, 6, 6, 6, 4, 4, 0]
    assert [sup(37, n, 167) for n in (8, 9, 16, 17)] == [6, 4, 4, 0]
    assert L.bbbp_attention_keep_bytes(37, 2, 8) == 2 * 3 * 3 * 64 and L.bbbp_attention_keep_bytes(37, 1, 167) == 0
    ERR_ARG, fake = 1, ctypes.c_void_p(4096)
    for B, F, nhead in ((961, 16, 2), (513, 32, 2), (37, 24, 2), (37, 9 * 167, 9), (37, 17, 2), (0, 16, 2), (37, 16, 0)):
        assert L.bbbp_attention_fwd(None, fake, fake, fake, B, F, nhead, 1.0, 0.0, 0, None) == ERR_ARG, (B, F, nhead)
        assert L.bbbp_attention_bwd(None, fake, fake, fake, fake, fake, B, F, nhead, 1.0, 0.0, 0, None) == ERR_ARG, (B, F, nhead)
    assert L.bbbp_attention_fwd(None, fake, fake, fake, 37, 16, 2, 1.0, 1.0, 0, None) == ERR_ARG and b"dropout_p" in L.bbbp_last_error()
    assert L.bbbp_attention_fwd(None, fake, None, fake, 37, 16, 2, 1.0, 0.0, 0, None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_attention_bwd(None, fake, fake, fake, fake, None, 37, 16, 2, 1.0, 0.0, 0, None) == ERR_ARG and b"null" in L.bbbp_last_error()
    for B, F, nhead in ((37, 96, 1), (37, 193, 1), (37, 17 * 100, 17), (37, 201, 2)):
        assert L.bbbp_attention_b3_fwd(None, fake, fake, B, F, nhead, 1.0, None, 0) == ERR_ARG, (B, F, nhead)
    assert L.bbbp_attention_b3_fwd(None, None, fake, 37, 167, 1, 1.0, None, 0) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_attention_b3_workspace_bytes(37, 1, 96) == 0
