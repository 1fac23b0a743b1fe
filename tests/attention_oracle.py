"""numpy oracle of the fused self-attention kernels in csrc/attention.hip and csrc/attention_b3.hip.

* ``forward`` / ``backward``: softmax(scale Q K^T) with dropout, times V, and its gradient in closed form, head by head (one [B, B]
  matrix alive at a time).  float64 by default -- the yardstick; ``dtype=np.float32`` evaluates the SAME formulas in float32, which is
  what float32 arithmetic can give on an input (``fp32_error_bound`` states how far that may be from float64).
* the dropout decisions are those of tests/rowops_oracle.py's exact Philox stream: element (h B + q) B + k.
* ``decode_keep``: the keep-byte layout the small-head forward kernel leaves for its backward pass.
* ``inputs``: the seeded operands of tests/test_gpu_attention.py per logit regime, here so that tests/test_attention_cpu.py can pin the
  oracle, and the logsumexp range every regime claims, without a GPU.
"""
import numpy as np

import rowops_oracle as R

REGIMES = ("ordinary", "std30", "max_last", "max_first", "neg95", "pos95")
LARGE = REGIMES[1:]


def shape_of(qkv, nhead):
    B, F3 = qkv.shape
    assert F3 % (3 * nhead) == 0
    return B, F3 // 3, F3 // 3 // nhead


def default_scale(head_dim):
    return float(head_dim) ** -0.5


def keep_scale_head(h, B, p, seed, base=None):
    """[B, B] float32: 0 or 1 / (1 - p) for (query, key) of head ``h`` -- element (h B + q) B + k of the stream; None when p == 0."""
    if p == 0:
        return None
    q = np.arange(B, dtype=np.uint64)
    idx = ((np.uint64(h * B) + q)[:, None] * np.uint64(B) + q[None, :]).ravel()
    return R.keep_scale(R.effective_seed(seed, base), idx, p).reshape(B, B)


def _head(qkv, F, D, h, dtype):
    return tuple(np.ascontiguousarray(qkv[:, t * F + h * D: t * F + (h + 1) * D], dtype=dtype) for t in range(3))


def _softmax(q, k, scale, dtype):
    s = (q @ k.T) * dtype(scale)
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(axis=1, keepdims=True)
    return e / l, (m + np.log(l))[:, 0]


def forward(qkv, nhead, scale=None, p=0.0, seed=0, base=None, dtype=np.float64, full=True):
    """(ctx [B, F], lse [nhead, B], prob [nhead, B, B], keep_scale [nhead, B, B] or None).  ``full=False``: prob and keep_scale are not
    collected (None), for the many-head shapes."""
    B, F, D = shape_of(qkv, nhead)
    scale = default_scale(D) if scale is None else scale
    ctx, lse = np.empty((B, F), dtype), np.empty((nhead, B), dtype)
    probs, keeps = [], []
    for h in range(nhead):
        q, k, v = _head(qkv, F, D, h, dtype)
        prob, lse[h] = _softmax(q, k, scale, dtype)
        ks = keep_scale_head(h, B, p, seed, base)
        ctx[:, h * D:(h + 1) * D] = (prob if ks is None else prob * ks.astype(dtype)) @ v
        if full:
            probs.append(prob); keeps.append(ks)
    if not full:
        return ctx, lse, None, None
    return ctx, lse, np.stack(probs), (None if p == 0 else np.stack(keeps))


def backward(qkv, dctx, nhead, scale=None, p=0.0, seed=0, base=None, dtype=np.float64):
    """dqkv [B, 3F]: dV = Pd^T dO, dP = dO V^T o keep, dS = P o (dP - rowsum(dP o P)) scale, dQ = dS K, dK = dS^T Q."""
    B, F, D = shape_of(qkv, nhead)
    scale = default_scale(D) if scale is None else scale
    dqkv = np.empty((B, 3 * F), dtype)
    for h in range(nhead):
        q, k, v = _head(qkv, F, D, h, dtype)
        do = np.ascontiguousarray(dctx[:, h * D:(h + 1) * D], dtype=dtype)
        prob, _ = _softmax(q, k, scale, dtype)
        ks = keep_scale_head(h, B, p, seed, base)
        ks = None if ks is None else ks.astype(dtype)
        dp = do @ v.T
        if ks is not None:
            dp = dp * ks
        ds = prob * (dp - (dp * prob).sum(axis=1, keepdims=True)) * dtype(scale)
        dqkv[:, h * D:(h + 1) * D] = ds @ k
        dqkv[:, F + h * D: F + (h + 1) * D] = ds.T @ q
        dqkv[:, 2 * F + h * D: 2 * F + (h + 1) * D] = (prob if ks is None else prob * ks).T @ do
    return dqkv


def fp32_error_bound(qkv, nhead, scale=None):
    """(ctx bound, lse bound): how far the float32 evaluation of ``forward`` (p = 0) may be from float64.  A score of D products, the
    scale and the subtraction of the row maximum round to within delta = (D + 3) 2^-24 scale max_qk sum_d |q_d k_d|; the exponentials
    and the two sums over B keys add (B + D + 16) roundings; a probability moves by at most the factor exp(2 delta)."""
    B, F, D = shape_of(qkv, nhead)
    scale = default_scale(D) if scale is None else scale
    u = 2.0 ** -24
    ctx_b = lse_b = 0.0
    for h in range(nhead):
        q, k, v = _head(qkv, F, D, h, np.float64)
        delta = (D + 3) * u * abs(scale) * float((np.abs(q) @ np.abs(k).T).max())
        lse_abs = abs(scale) * float(np.abs(q @ k.T).max()) + np.log(B)
        ctx_b = max(ctx_b, (np.expm1(2 * delta) * 1.25 + (B + D + 16) * u) * float(np.abs(v).max()))
        lse_b = max(lse_b, 1.5 * delta + (B + 16) * u + 4 * u * lse_abs)
    return ctx_b, lse_b


def decode_keep(keep, nhead, B):
    """bool [nhead, B, B] from the bytes [nhead][ceil(B/16)][ceil(B/16)][64]: byte (h, qb, kt, lane = 16 kq + q), bit r <-> query
    16 qb + q keeps key 16 kt + 4 kq + r."""
    nt = (B + 15) // 16
    a = np.asarray(keep, dtype=np.uint8).reshape(nhead, nt, nt, 4, 16)                  # h, qb, kt, kq, q
    bits = (a[..., None] >> np.arange(4, dtype=np.uint8)) & 1                            # h, qb, kt, kq, q, r
    return bits.transpose(0, 1, 4, 2, 3, 5).reshape(nhead, nt * 16, nt * 16)[:, :B, :B].astype(bool)


# ---- the large-logit cases of tests/test_gpu_attention.py: (nhead, head_dim) per kernel family, at a full, a ragged and a two-chunk batch -----
REGIME_BS = (32, 37, 129)
REGIME_HEADS = {"small": [(2, 8), (2, 16)], "wide": [(1, 167), (2, 167)], "b3": [(1, 167), (2, 128)]}
REGIME_MANY_HEADS = (256, 8, 129)          # single-sweep backward whose ragged last key tile is a wave's SECOND tile
REGIME_SHAPES = sorted({(n, d, b) for heads in REGIME_HEADS.values() for n, d in heads for b in REGIME_BS} | {REGIME_MANY_HEADS})


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def inputs(nhead, D, B, regime="ordinary", seed=0):
    """(qkv [B, 3F] float32, dctx [B, F] float32) for the default scale D ** -0.5.

    ordinary : standard normal Q, K, V: scores of standard deviation 1.
    std30    : Q, K of variance 30: scores of standard deviation 30, near-one-hot rows.
    max_last : every query's maximum is the LAST key, 60 above the typical score (the online softmax meets it after everything else and
               rescales what it has by exp(-60)); max_first: the first key.
    neg95    : Q rows a u + noise, K rows -a u + noise with scale a^2 = 120: every score, hence every logsumexp, below -95.
    pos95    : K rows +a u + noise: every score and logsumexp above +95.
    """
    assert regime in REGIMES
    rng = np.random.default_rng([seed, nhead, D, B, REGIMES.index(regime)])
    scale = default_scale(D)
    q, k, v = (rng.standard_normal((B, nhead, D)) for _ in range(3))
    u = rng.standard_normal((nhead, D))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if regime == "std30":
        q *= np.sqrt(30.0); k *= np.sqrt(30.0)
    elif regime in ("max_last", "max_first"):
        a = np.sqrt(60.0 / scale)
        q += a * u
        k[B - 1 if regime == "max_last" else 0] += a * u
    elif regime in ("neg95", "pos95"):
        a = np.sqrt(120.0 / scale)
        q = a * u + 0.1 * q
        k = (a if regime == "pos95" else -a) * u + 0.1 * k
    qkv = np.concatenate([t.reshape(B, nhead * D) for t in (q, k, v)], axis=1).astype(np.float32)
    return qkv, rng.standard_normal((B, nhead * D)).astype(np.float32)
