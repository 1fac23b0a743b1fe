"""numpy oracle of the row / column kernels in csrc/rowops.hip and of the dropout stream in csrc/common.h.

Three layers:

* the Philox-4x32-10 stream and the keep decision in the integer / float32 arithmetic the kernels use -- exact, so the GPU tests compare
  with ``==``;
* float64 references (from float32 inputs) of softmax, BatchNorm1d, the sharded-BatchNorm pieces, bias_act_bwd, MSE and the attention
  fusion combine -- the yardstick of every tolerant comparison;
* float32 restatements of the BatchNorm and softmax kernels in the kernels' own order of operations -- what float32 can give at a
  shape.  Where a case does not hold at the tolerances of tests/test_gpu_ops.py, its bound is 4 x the restatement's own deviation from
  float64 (``S``), never a figure taken from the kernel.

The case lists of tests/test_gpu_rowops.py live here too, so that tests/test_rowops_cpu.py can pin the references to torch on the same
cases without a GPU.
"""
import numpy as np

# ---- Philox-4x32-10 ------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32, _S8, _S2 = np.uint64(32), np.uint64(8), np.uint64(2)
CTR2, CTR3 = 0x9E3779B9, 0xBB67AE85            # the constant upper half of the project's counter (common.h:philox4)
SEED_MUL = 0x9E3779B97F4A7C15                  # common.h:effective_seed


def _u32(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox-4x32 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words; returns the four output words."""
    shape = np.broadcast(*(np.asarray(v) for v in (c0, c1, c2, c3, k0, k1))).shape
    c0, c1, c2, c3, k0, k1 = (np.broadcast_to(_u32(v), shape or (1,)).copy() for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                          # 32 x 32 -> 64 bits: no wrap in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return tuple(w.reshape(shape) for w in (c0, c1, c2, c3))


def stream_words(seed, idx):
    """Word ``idx`` of dropout stream ``seed``: component ``idx & 3`` of the block at counter ``idx >> 2``, key (lo32, hi32) of seed."""
    seed = int(seed) & (2 ** 64 - 1)
    i = np.asarray(idx, dtype=np.uint64)
    blk = i >> _S2
    words = np.stack(philox4x32_10(blk & _M32, blk >> _S32, CTR2, CTR3, seed & 0xFFFFFFFF, seed >> 32))
    sel = (i & np.uint64(3)).astype(np.int64)
    return np.take_along_axis(words, sel[None], axis=0)[0]


def keep_scale(seed, idx, p):
    """0 or 1 / (1 - p) for element ``idx``, in the kernels' float32 arithmetic (common.h:dropout_scale)."""
    p = np.float32(p)
    u = (stream_words(seed, idx) >> _S8).astype(np.float32) * np.float32(2.0 ** -24)
    inv_keep = np.float32(1) / (np.float32(1) - p)
    return np.where(u >= p, inv_keep, np.float32(0)).astype(np.float32)


def effective_seed(seed, base=None):
    """The stream a seeded kernel draws when the library's seed base points at the 64-bit value ``base`` (None: no base set)."""
    seed = int(seed) & (2 ** 64 - 1)
    return seed if base is None else ((int(base) & (2 ** 64 - 1)) * SEED_MUL + seed) & (2 ** 64 - 1)


def keep_scale_like(x, p, seed, base=None):
    """keep_scale for every element of a contiguous tensor shaped like ``x`` (element i of the flattened tensor draws word i)."""
    x = np.asarray(x)
    return keep_scale(effective_seed(seed, base), np.arange(x.size, dtype=np.uint64), p).reshape(x.shape)


def dropout(x, p, seed, base=None):
    x = np.asarray(x, dtype=np.float32)
    if p == 0:
        return x.copy()
    return x * keep_scale_like(x, p, seed, base)


# ---- float64 references --------------------------------------------------------------------------------------------------------
def _f64(*a):
    return [None if v is None else np.asarray(v, dtype=np.float64) for v in a]


def softmax_fwd(x):
    x, = _f64(x)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_bwd(dpd, prob, scale=None):
    """ds = P * (dP - sum(dP * P)), dP = dpd * keep-scale."""
    dpd, prob, scale = _f64(dpd, prob, scale)
    dp = dpd if scale is None else dpd * scale
    return prob * (dp - (dp * prob).sum(axis=-1, keepdims=True))


def batchnorm_fwd(x, gamma, beta, running_mean, running_var, training, eps=1e-5, momentum=0.1):
    """Returns (y, save_mean, save_rstd, running_mean', running_var')."""
    x, gamma, beta, rm, rv = _f64(x, gamma, beta, running_mean, running_var)
    rows = x.shape[0]
    if training:
        mean = x.mean(axis=0)
        var = ((x - mean) ** 2).mean(axis=0)                      # biased, for y
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * (rows / (rows - 1))
    else:
        mean, var = rm, rv
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean) * rstd * gamma + beta, mean, rstd, rm, rv


def batchnorm_bwd(dy, x, gamma, save_mean, save_rstd, training, relu_gate=False):
    """Returns (dx, dgamma, dbeta).  ``relu_gate``: x is the output of a ReLU whose backward rides along (dx = 0 where x <= 0);
    dgamma / dbeta are the BatchNorm's own and are not gated."""
    dy, x, gamma, mu, rs = _f64(dy, x, gamma, save_mean, save_rstd)
    rows = x.shape[0]
    xhat = (x - mu) * rs
    dgamma, dbeta = (dy * xhat).sum(axis=0), dy.sum(axis=0)
    dx = gamma * rs * (dy - dbeta / rows - xhat * dgamma / rows) if training else dy * gamma * rs
    if relu_gate:
        dx = np.where(x > 0, dx, 0.0)
    return dx, dgamma, dbeta


def column_moments(x, centre=None):
    x, centre = _f64(x, centre)
    d = x if centre is None else x - centre
    return d.sum(axis=0), (d * d).sum(axis=0)


def batchnorm_bwd_apply(dy, x, gamma, mean, rstd, sum_dy, sum_dy_xhat, n):
    dy, x, gamma, mean, rstd, sum_dy, sum_dy_xhat = _f64(dy, x, gamma, mean, rstd, sum_dy, sum_dy_xhat)
    xhat = (x - mean) * rstd
    return gamma * rstd * (dy - sum_dy / n - xhat * sum_dy_xhat / n)


def bias_act_bwd(dy, y, act, scale=1.0):
    """(dy', db): dy' = dy * act'(y) * scale for act 1 (relu: y > 0) and 2 (tanh: 1 - y^2); act 0 leaves dy alone -- the kernel
    applies ``scale`` only together with an activation -- and db holds the column sums of dy'."""
    dy, y = _f64(dy, y)
    if act == 1:
        dy = np.where(y > 0, dy * scale, 0.0)
    elif act == 2:
        dy = dy * (1.0 - y * y) * scale
    return dy, dy.sum(axis=0)


def mse(pred, target, grad_scale=1.0):
    pred, target = _f64(pred, target)
    d = pred.ravel() - target.ravel()
    return (d * d).mean(), 2.0 * d / d.size * grad_scale


def fusion_combine_fwd(combined, hid, w2, b2):
    """hid [nh, rows, hd], w2 [nh, hd], b2 [nh].  Returns (logits [rows, nh], attn [rows, nh], out [rows, dim])."""
    combined, hid, w2, b2 = _f64(combined, hid, w2, b2)
    logits = np.einsum("hrc,hc->rh", hid, w2) + b2
    attn = softmax_fwd(logits)
    return logits, attn, combined * attn.sum(axis=1, keepdims=True)


# ---- float32 restatements in the kernels' order of operations ---------------------------------------------------------------------
_F = np.float32


def _lane_sums32(a, lanes):
    """Sums of float32 ``a`` over axis 0 as a kernel does them: ``lanes`` accumulators striding the axis, each sequential.  Returns
    the [lanes, ...] partial sums."""
    n = a.shape[0]
    pad = (-n) % lanes
    if pad:
        a = np.concatenate([a, np.zeros((pad,) + a.shape[1:], _F)])
    a = a.reshape((-1, lanes) + a.shape[1:])
    acc = np.zeros(a.shape[1:], _F)
    for i in range(a.shape[0]):
        acc = acc + a[i]
    return acc


def _seq_sum32(parts):
    t = np.zeros(parts.shape[1:], _F)
    for i in range(parts.shape[0]):
        t = t + parts[i]
    return t


def _butterfly32(parts, op=np.add):
    """wave_sum / wave_max: xor-shuffle butterfly over the 64 lanes on axis 0."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        parts = op(parts, parts[lanes ^ o])
    return parts[0]


def softmax_fwd32(x):
    """softmax_fwd_kernel: one wave per row, lane-strided maximum and sum, butterfly reductions, e * (1 / sum)."""
    x = np.asarray(x, dtype=_F)
    xt = x.T                                                       # [cols, rows]: the reduced axis first
    with np.errstate(invalid="ignore"):
        m = xt.max(axis=0)                                         # a maximum is exact in any order
        e = np.exp((xt - m).astype(_F)).astype(_F)
    s = _butterfly32(_lane_sums32(e, 64))
    inv = _F(1) / s
    return (e * inv).T.astype(_F)


def batchnorm_fwd32(x, gamma, beta, running_mean, running_var, training, eps=1e-5, momentum=0.1):
    """batchnorm_fwd_kernel: 16 row lanes per column, a sequential tree over the 16 partial sums, two passes."""
    x, gamma, beta, rm, rv = (np.asarray(v, dtype=_F) for v in (x, gamma, beta, running_mean, running_var))
    rows = x.shape[0]
    eps, momentum = _F(eps), _F(momentum)
    if training:
        mu = _seq_sum32(_lane_sums32(x, 16)) / _F(rows)
        d = x - mu
        var = _seq_sum32(_lane_sums32(d * d, 16)) / _F(rows)
        rm = (_F(1) - momentum) * rm + momentum * mu
        rv = (_F(1) - momentum) * rv + momentum * var * (_F(rows) / _F(rows - 1))
    else:
        mu, var = rm, rv
    rstd = _F(1) / np.sqrt(var + eps)
    return (x - mu) * rstd * gamma + beta, mu, rstd, rm, rv


def batchnorm_bwd32(dy, x, gamma, save_mean, save_rstd, training, relu_gate=False):
    """batchnorm_bwd_kernel in float32, same lane structure."""
    dy, x, gamma, mu, rs = (np.asarray(v, dtype=_F) for v in (dy, x, gamma, save_mean, save_rstd))
    rows = x.shape[0]
    dgamma = _seq_sum32(_lane_sums32(dy * (x - mu) * rs, 16))
    dbeta = _seq_sum32(_lane_sums32(dy, 16))
    sa, sb = dgamma / _F(rows), dbeta / _F(rows)
    dx = gamma * rs * (dy - sb - (x - mu) * rs * sa) if training else dy * gamma * rs
    if relu_gate:
        dx = np.where(x > 0, dx, _F(0))
    return dx, dgamma, dbeta


def deviation(a, ref):
    """Largest |a - ref|: the S of a float32 restatement against its float64 reference."""
    a, ref = _f64(a, ref)
    return float(np.abs(a - ref).max()) if a.size else 0.0


# ---- inputs and case lists shared by the CPU and GPU tests --------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


DROPOUT_LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 70001]
DROPOUT_PS = [0.1, 0.25, 0.5, 0.9]
DROPOUT_SEEDS = [0, 5, 2 ** 32 - 1, 2 ** 32, 0x9E3779B97F4A7C15, 2 ** 60 + 12345]
SEED_BASES = [0, 1, 2, 2 ** 40 + 7, 2 ** 63 + 1]

SOFTMAX_ROWS = [1, 3, 4, 5, 9]
SOFTMAX_COLS = [1, 2, 63, 64, 65, 167, 4097]
SOFTMAX_DROPOUT = [(0.0, 0), (0.3, 777), (0.3, 2 ** 60 + 12345)]          # (p, seed): below and above 2^32


def softmax_inputs(rows, cols):
    return rnd(rows, cols, seed=1000 * rows + cols, scale=3.0), rnd(rows, cols, seed=1000 * rows + cols + 500000)


def softmax_special_rows(cols=167):
    """name -> [1, cols] rows: a large common offset, some -inf entries, one dominant entry."""
    base = rnd(1, cols, seed=4242, scale=3.0)
    masked = base.copy()
    masked[0, ::3] = -np.inf
    dominant = base.copy()
    dominant[0, cols // 2] += 300.0
    return {"offset-1e4": base + np.float32(1e4), "neg-inf": masked, "dominant": dominant}


BN_ROWS = [2, 15, 16, 17, 33, 512]
BN_COLS = [1, 63, 64, 65, 130]
BN_MOMENTA = [0.1, 0.3]
BN_SHIFTED = (33, 130)                      # the case with a third of its columns shifted by 30 standard deviations


def batchnorm_inputs(rows, cols, shifted=False):
    """(x, gamma, beta, running_mean, running_var, dy) with non-trivial running statistics."""
    s = 7000 * rows + 10 * cols
    x = rnd(rows, cols, seed=s)
    if shifted:
        x[:, : max(1, cols // 3)] += np.float32(30.0)
    gamma, beta = (1 + 0.2 * rnd(cols, seed=s + 1)).astype(np.float32), rnd(cols, seed=s + 2, scale=0.3)
    rm, rv = rnd(cols, seed=s + 3, scale=0.5), (np.abs(rnd(cols, seed=s + 4)) + np.float32(0.5)).astype(np.float32)
    return x, gamma, beta, rm, rv, rnd(rows, cols, seed=s + 5)


SHARD_ROWS = (16, 17)
SHARD_COLS = [5, 16, 17]

BIAS_ACT_ROWS = [1, 31, 32, 33, 100]
BIAS_ACT_COLS = [1, 15, 16, 17, 70]
BIAS_ACT_SCALES = [1.0, 1.25]

MSE_NS = [1, 2, 255, 256, 257, 1000]
MSE_SCALES = [1.0, 0.5]

FUSION_HEADS = [1, 3, 8]
FUSION_HIDDEN = [1, 64, 65, 128]
FUSION_DIMS = [1, 64, 256 + 3]
FUSION_ROWS = [1, 4, 5]


def fusion_inputs(nh, hd, dim, rows):
    """(combined [rows, dim], hid [nh, rows, hd] = tanh(randn), w2 [nh, hd], b2 [nh], dout [rows, dim])."""
    s = ((nh * 131 + hd) * 307 + dim) * 11 + rows
    return (rnd(rows, dim, seed=s), np.tanh(rnd(nh, rows, hd, seed=s + 1)).astype(np.float32), rnd(nh, hd, seed=s + 2, scale=0.5),
            rnd(nh, seed=s + 3, scale=0.5), rnd(rows, dim, seed=s + 4))
