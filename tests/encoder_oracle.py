"""numpy oracle of the encoder layer outside attention: the out_proj fold of csrc/fold.hip, the LayerNorm parameter gradients and the
row-fused stretches of csrc/encoder.hip (nn.TransformerEncoderLayer, post-norm, ReLU, eps = 1e-5).

Plain formulas in ``dtype`` (float64: the yardstick; float32: what float32 gives on the same input).  The dropout keep-scales are the exact
ones of tests/rowops_oracle.py: site 1 (after out_proj) and site 3 (after linear2) draw element ``row * F + col`` of their streams, site 2
(the hidden activation) element ``row * DFF + col``.  tests/test_encoder_oracle_cpu.py pins every function to float64 torch autograd.

The input generators and case lists of tests/test_gpu_encoder_rows.py and tests/test_gpu_fold_ops.py live here too.
"""
import numpy as np

import rowops_oracle as R

EPS = 1e-5
FWD_NAMES = ("z1", "y1", "hff", "z2", "y2", "mean1", "rstd1", "mean2", "rstd2")
BWD_NAMES = ("dyout", "dz2", "dff", "dhff", "dy1", "dz1", "dsa", "dctx")
SAVED_NAMES = ("z1", "z2", "hff", "mean1", "rstd1", "mean2", "rstd2")
WEIGHT_NAMES = ("wo", "bo", "g1", "be1", "w1", "b1", "w2", "b2", "g2", "be2")


def _cast(dtype, *a):
    return [None if v is None else np.asarray(v, dtype=dtype) for v in a]


# ---- out_proj folded into the value projection ---------------------------------------------------------------------------------------------
def fold(win, bin, wo, bo=None, dtype=np.float64):
    """(wf [3F, F], bf [3F], wvt [F + 1, F]): wf = Wq; Wk; Wo Wv, bf = bq; bk; Wo bv (+ bo), wvt = [Wv | bv]^T."""
    win, bin, wo, bo = _cast(dtype, win, bin, wo, bo)
    F = wo.shape[0]
    wv, bv = win[2 * F:], bin[2 * F:]
    bp = wo @ bv
    if bo is not None:
        bp = bp + bo
    return np.concatenate([win[:2 * F], wo @ wv]), np.concatenate([bin[:2 * F], bp]), np.concatenate([wv, bv[:, None]], axis=1).T.copy()


def unfold(tdw, tdb, wo, wvt, dz, dtype=np.float64):
    """(dWo, dbo, d(Wv rows), d(bv)) from dW' = tdw, db' = tdb:  dWo = dW' Wv^T + db' bv^T, dbo = column sums of dz, d[Wv | bv] = Wo^T [dW' | db']."""
    tdw, tdb, wo, wvt, dz = _cast(dtype, tdw, tdb, wo, wvt, dz)
    F = wo.shape[0]
    wv, bv = wvt[:F].T, wvt[F]
    return tdw @ wv.T + np.outer(tdb, bv), dz.sum(axis=0), wo.T @ tdw, wo.T @ tdb


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def ln_param_grad(dy, z, mean, rstd, dtype=np.float64):
    """(dgamma, dbeta) = (sum_rows dy * xhat, sum_rows dy), xhat = (z - mean) * rstd."""
    dy, z, mean, rstd = _cast(dtype, dy, z, mean, rstd)
    return (dy * (z - mean[:, None]) * rstd[:, None]).sum(axis=0), dy.sum(axis=0)


def _ln_fwd(z, gamma, beta):
    mean = z.mean(axis=1)
    d = z - mean[:, None]
    rstd = 1 / np.sqrt((d * d).mean(axis=1) + z.dtype.type(EPS))
    return d * rstd[:, None] * gamma + beta, mean, rstd


def _ln_bwd(dy, z, gamma, mean, rstd):
    g = dy * gamma
    xhat = (z - mean[:, None]) * rstd[:, None]
    return rstd[:, None] * (g - g.mean(axis=1, keepdims=True) - xhat * (g * xhat).mean(axis=1, keepdims=True))


# ---- the row-fused stretches ----------------------------------------------------------------------------------------------------------------
def keep_scales(B, F, DFF, p, seeds, base=None):
    """The keep-scales (float32: 0 or 1 / (1 - p)) of the three dropout sites: [B, F], [B, DFF], [B, F]; all ones when p == 0."""
    shapes = ((B, F), (B, DFF), (B, F))
    if p == 0:
        return tuple(np.ones(s, np.float32) for s in shapes)
    return tuple(R.keep_scale_like(np.empty(s, np.float32), p, seed, base) for s, seed in zip(shapes, seeds))


def rows_fwd(ctx, xin, weights, p=0.0, seeds=(0, 0, 0), base=None, next=None, dtype=np.float64, masks=None):
    """out_proj (+ bias, dropout, + x) -> LayerNorm1 -> linear1 (+ bias, ReLU, dropout) -> linear2 (+ bias, dropout, + y1) -> LayerNorm2 ->
    the next projection ``next`` = dict(wn, bn, act).  Returns a dict: z1, y1, hff, z2, y2, mean1, rstd1, mean2, rstd2, outn (None without
    ``next``), and for the tests ``pre`` (linear1's output before the ReLU) and ``masks`` (the three keep-scales; ``masks=`` overrides)."""
    ctx, xin = _cast(dtype, ctx, xin)
    w = dict(zip(WEIGHT_NAMES, _cast(dtype, *[weights[n] for n in WEIGHT_NAMES])))
    B, F = ctx.shape
    DFF = w["w1"].shape[0]
    masks = keep_scales(B, F, DFF, p, seeds, base) if masks is None else masks
    k1, k2, k3 = _cast(dtype, *masks)
    o = {}
    o["z1"] = (ctx @ w["wo"].T + w["bo"]) * k1 + xin
    o["y1"], o["mean1"], o["rstd1"] = _ln_fwd(o["z1"], w["g1"], w["be1"])
    o["pre"] = o["y1"] @ w["w1"].T + w["b1"]
    o["hff"] = np.maximum(o["pre"], 0) * k2
    o["z2"] = (o["hff"] @ w["w2"].T + w["b2"]) * k3 + o["y1"]
    o["y2"], o["mean2"], o["rstd2"] = _ln_fwd(o["z2"], w["g2"], w["be2"])
    o["outn"] = None
    if next is not None:
        wn, bn = _cast(dtype, next["wn"], next["bn"])
        v = o["y2"] @ wn.T + bn
        o["outn"] = np.maximum(v, 0) if next.get("act") else v
    o["masks"] = masks
    return o


def rows_bwd(saved, weights, dyout=None, up=None, p=0.0, seeds=(0, 0), base=None, dtype=np.float64, masks=None):
    """The backward of ``rows_fwd`` from ``saved`` (z1, z2, hff, mean1, rstd1, mean2, rstd2, taken as given) and the gradient of y2: ``dyout``,
    or ``up`` = dict(dqkv_up, win_up, dz1_up) -> dyout = dqkv_up Win_up + dz1_up.  ``seeds``: the streams of sites 1 and 3 (``masks``: the
    two keep-scales instead).  The ReLU / dropout gate of the hidden site is ``hff > 0``, scaled by the float32 1 / (1 - p), as the kernel
    takes it.  Returns a dict: dyout, dz2, dff, dhff, dy1, dz1, dsa, dctx."""
    s = dict(zip(SAVED_NAMES, _cast(dtype, *[saved[n] for n in SAVED_NAMES])))
    w = {n: np.asarray(weights[n], dtype=dtype) for n in ("g1", "g2", "w1", "w2", "wo")}
    B, F = s["z1"].shape
    if masks is None:
        k1, _, k3 = keep_scales(B, F, 1, p, (seeds[0], 0, seeds[1]), base)
    else:
        k1, k3 = masks
    k1, k3 = _cast(dtype, k1, k3)
    inv_keep = dtype(np.float32(1) / (np.float32(1) - np.float32(p))) if p > 0 else dtype(1)
    o = {}
    if up is not None:
        dqkv_up, win_up, dz1_up = _cast(dtype, up["dqkv_up"], up["win_up"], up["dz1_up"])
        o["dyout"] = dqkv_up @ win_up + dz1_up
    else:
        o["dyout"], = _cast(dtype, dyout)
    o["dz2"] = _ln_bwd(o["dyout"], s["z2"], w["g2"], s["mean2"], s["rstd2"])
    o["dff"] = o["dz2"] * k3
    o["dhff"] = np.where(s["hff"] > 0, (o["dff"] @ w["w2"]) * inv_keep, 0)
    o["dy1"] = o["dhff"] @ w["w1"] + o["dz2"]
    o["dz1"] = _ln_bwd(o["dy1"], s["z1"], w["g1"], s["mean1"], s["rstd1"])
    o["dsa"] = o["dz1"] * k1
    o["dctx"] = o["dsa"] @ w["wo"]
    return o


# ---- inputs and case lists shared by the CPU and GPU tests ---------------------------------------------------------------------------------
ROW_BS = [1, 16, 17, 37]
ROW_FS = [4, 15, 16, 17, 64, 167, 192]
ROW_DFFS = [16, 18, 70, 272]                   # 2048 runs with F = 167 at B = 37 only
ROW_PS = [0.0, 0.1]
ROW_SEEDS = (11, 12, 13)
HIGH_SEEDS = (2 ** 32 + 5, 2 ** 60 + 12345, 2 ** 63 + 1)
SEED_BASE = 2 ** 40 + 7
NEXT_KINDS = ("none", "in_proj", "fc")         # absent; nn = 3F, ldn = 3F, no activation; nn = 128, ldn = 256, ReLU

FOLD_FS = [1, 3, 4, 5, 63, 64, 65, 167, 255]
FOLD_LAYERS = [(F, 1) for F in FOLD_FS] + [(5, 6), (167, 6), (5, 32)]
UNFOLD_BS = [1, 15, 16, 17, 100]

# (n, rows, cols): every n, rows and cols value with at least two values of the other axes; n = 13 and 25 with ragged rows and cols
LN_GRAD_CASES = [(1, 1, 1), (1, 33, 17), (1, 100, 167), (2, 31, 15), (2, 32, 16), (2, 1, 167), (2, 100, 1), (12, 32, 16), (12, 33, 15), (12, 31, 17),
                 (13, 33, 17), (13, 31, 167), (13, 100, 15), (25, 33, 17), (25, 31, 15), (25, 1, 16), (2, 100, 167), (1, 32, 1), (12, 100, 16)]


def rnd(*shape, seed=0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def next_projection(kind, F, seed=0):
    """The next projection of a case: None, in_proj of the next layer, or fingerprint_fc + ReLU."""
    if kind == "none":
        return None
    nn = 3 * F if kind == "in_proj" else 128
    return dict(wn=rnd(nn, F, seed=seed + 50, scale=F ** -0.5), bn=rnd(nn, seed=seed + 51, scale=0.3), act="relu" if kind == "fc" else None)


def row_inputs(B, F, DFF, shifted=False):
    """float32 inputs of one row case: ctx, xin, the ten weights, and for the backward dyout and the layer above's (dqkv_up, win_up, dz1_up).
    ``shifted``: a third of the rows of x carry a mean of 30, far above their spread."""
    s = (B * 1009 + F) * 4099 + DFF
    ctx, xin = rnd(B, F, seed=s), rnd(B, F, seed=s + 1)
    if shifted:
        xin[: max(1, B // 3)] += np.float32(30.0)
    w = dict(wo=rnd(F, F, seed=s + 2, scale=F ** -0.5), bo=rnd(F, seed=s + 3, scale=0.3),
             g1=(1 + 0.2 * rnd(F, seed=s + 4)).astype(np.float32), be1=rnd(F, seed=s + 5, scale=0.3),
             w1=rnd(DFF, F, seed=s + 6, scale=F ** -0.5), b1=rnd(DFF, seed=s + 7, scale=0.3),
             w2=rnd(F, DFF, seed=s + 8, scale=DFF ** -0.5), b2=rnd(F, seed=s + 9, scale=0.3),
             g2=(1 + 0.2 * rnd(F, seed=s + 10)).astype(np.float32), be2=rnd(F, seed=s + 11, scale=0.3))
    up = dict(dqkv_up=rnd(B, 3 * F, seed=s + 12), win_up=rnd(3 * F, F, seed=s + 13, scale=F ** -0.5), dz1_up=rnd(B, F, seed=s + 14))
    return ctx, xin, w, rnd(B, F, seed=s + 15), up


def fold_inputs(F, layers):
    """Per layer: win [3F, F], bin [3F], wo [F, F], bo [F] (float32)."""
    s = 70000 * layers + 13 * F
    return ([rnd(3 * F, F, seed=s + 4 * l, scale=F ** -0.5) for l in range(layers)], [rnd(3 * F, seed=s + 4 * l + 1, scale=0.3) for l in range(layers)],
            [rnd(F, F, seed=s + 4 * l + 2, scale=F ** -0.5) for l in range(layers)], [rnd(F, seed=s + 4 * l + 3, scale=0.3) for l in range(layers)])


def unfold_inputs(F, B):
    """tdw [F, F], tdb [F], wo [F, F], wvt [F + 1, F], dz [B, F] (float32)."""
    s = 90000 * B + 17 * F
    return rnd(F, F, seed=s), rnd(F, seed=s + 1), rnd(F, F, seed=s + 2, scale=F ** -0.5), rnd(F + 1, F, seed=s + 3, scale=F ** -0.5), rnd(B, F, seed=s + 4)


def ln_grad_inputs(n, rows, cols):
    """n distinct (dy, z, mean, rstd): z with per-row offsets, mean and rstd its float32 statistics."""
    out = []
    for i in range(n):
        s = ((n * 131 + rows) * 257 + cols) * 31 + i
        dy = rnd(rows, cols, seed=s)
        z = (rnd(rows, cols, seed=s + 1000003, scale=1.0 + 0.1 * i) + rnd(rows, 1, seed=s + 2000003)).astype(np.float32)
        z64 = z.astype(np.float64)
        mean = z64.mean(axis=1)
        rstd = 1 / np.sqrt(((z64 - mean[:, None]) ** 2).mean(axis=1) + EPS)
        out.append((dy, z, mean.astype(np.float32), rstd.astype(np.float32)))
    return out
