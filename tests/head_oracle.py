"""numpy oracle of the fused fusion-block + head kernels in csrc/head.hip (ops.head_fwd / ops.head_bwd).

* ``forward``: combined [B, 256] -> 4 x (Linear(256,128) -> Tanh -> Linear(128,1)) -> softmax over the heads -> sum_h a_h combined ->
  Linear(256,256)+ReLU -> BatchNorm1d (eps 1e-5, momentum 0.1, unbiased running variance) -> Linear(256,128)+ReLU -> Linear(128,64)+ReLU
  -> Linear(64,1); every tensor the kernels write, and the updated running statistics.
* ``backward``: the input-gradient chain as a composition of per-stage VJPs over SAVED tensors taken as given -- nothing is recomputed
  from ``comb``, so attn rows need not sum to 1 and hid need not be the Tanh of anything (the off-manifold cases: on real activations
  the fusion block's gradient is analytically zero, sum_h a_h = 1, and only there does it have magnitude).
* float64 by default -- the yardstick; ``dtype=np.float32`` evaluates the SAME formulas in float32: what float32 arithmetic can give.
* ``make_params`` / ``make_comb`` / ``off_manifold``: the seeded operands of tests/test_gpu_head.py, here so that tests/test_head_cpu.py
  can pin what each case claims (dead columns, saturated rows, ties) without a GPU.
Parameters travel as a dict: fw1, fb1, fw2, fb2 lists of four arrays ([128, 256], [128], [128], [1]); w0 [256, 256], b0, gamma, beta [256],
w3 [128, 256], b3, w5 [64, 128], b5, w7 [64], b7 [1] (Linear weights [out, in]) -- the names of bbbp_amd.ops.HEAD_PARAM_SHAPES.
"""
import numpy as np

NHEADS, COMB, FHID, H1, H2, H3 = 4, 256, 128, 256, 128, 64
EPS, MOMENTUM = 1e-5, 0.1
PER_HEAD = ("fw1", "fb1", "fw2", "fb2")
FORWARD_OUT = ("hid", "attn", "fused", "h", "hb", "bn_mean", "bn_rstd", "h2", "h3", "out")
SAVED = ("hid", "attn", "h", "h2", "h3", "bn_mean", "bn_rstd")
BACKWARD_OUT = ("dh3", "dh2", "dhb", "dh", "dlogit", "dpre", "dcomb", "dgamma", "dbeta")


def cast(params, dtype):
    return {k: ([np.asarray(a, dtype=dtype) for a in v] if k in PER_HEAD else np.asarray(v, dtype=dtype)) for k, v in params.items()}


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def softmax_rows(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def batchnorm(x, gamma, beta, running_mean, running_var, training, dtype=np.float64):
    """(y, mean, rstd, new running_mean, new running_var): batch statistics (biased variance, two passes) when training."""
    n = x.shape[0]
    if training:
        assert n > 1, "Expected more than 1 value per channel when training"
        mean = x.mean(axis=0)
        var = ((x - mean) ** 2).mean(axis=0)
        m = dtype(MOMENTUM)
        running_mean = (1 - m) * running_mean + m * mean
        running_var = (1 - m) * running_var + m * (var * dtype(n / (n - 1)))
    else:
        mean, var = running_mean, running_var
    rstd = 1 / np.sqrt(var + dtype(EPS))
    return (x - mean) * rstd * gamma + beta, mean, rstd, running_mean, running_var


def forward(comb, params, running, training, concat=False, dtype=np.float64):
    """dict of FORWARD_OUT (hid [4, B, 128], attn [B, 4], out [B]; hid / attn None and fused = comb when ``concat``), the logits [B, 4] and
    the running statistics after the call (the given ones in eval).  ``running``: (running_mean, running_var)."""
    P, x = cast(params, dtype), np.asarray(comb, dtype=dtype)
    rm, rv = (np.asarray(r, dtype=dtype) for r in running)
    o = {}
    if concat:
        o["hid"] = o["attn"] = o["logit"] = None
        o["fused"] = x
    else:
        o["hid"] = np.stack([np.tanh(x @ P["fw1"][h].T + P["fb1"][h]) for h in range(NHEADS)])
        o["logit"] = np.stack([o["hid"][h] @ P["fw2"][h] + P["fb2"][h][0] for h in range(NHEADS)], axis=1)
        o["attn"] = softmax_rows(o["logit"])
        o["fused"] = (o["attn"][:, :, None] * x[:, None, :]).sum(axis=1)
    o["h"] = np.maximum(o["fused"] @ P["w0"].T + P["b0"], 0)
    o["hb"], o["bn_mean"], o["bn_rstd"], o["running_mean"], o["running_var"] = batchnorm(o["h"], P["gamma"], P["beta"], rm, rv, training, dtype)
    o["h2"] = np.maximum(o["hb"] @ P["w3"].T + P["b3"], 0)
    o["h3"] = np.maximum(o["h2"] @ P["w5"].T + P["b5"], 0)
    o["out"] = o["h3"] @ P["w7"] + P["b7"][0]
    return o


# ---- backward: one VJP per stage, each over the saved OUTPUT of its stage ------------------------------------------------------------------
def relu_vjp(dy, y):
    return dy * (y > 0)


def tanh_vjp(dy, y):
    return dy * (1 - y * y)


def softmax_vjp(da, a):
    """Gradient at the logits from the gradient at the probabilities, with ``a`` whatever was saved (rows need not sum to 1)."""
    return a * (da - (da * a).sum(axis=1, keepdims=True))


def batchnorm_vjp(dy, x, gamma, mean, rstd, training):
    """(dx, dgamma, dbeta) with the saved mean / rstd taken as given; eval: the statistics are constants."""
    n = x.shape[0]
    xhat = (x - mean) * rstd
    dgamma, dbeta = (dy * xhat).sum(axis=0), dy.sum(axis=0)
    if training:
        return gamma * rstd * (dy - dbeta / n - xhat * (dgamma / n)), dgamma, dbeta
    return dy * gamma * rstd, dgamma, dbeta


def fusion_vjp(dfused, comb, attn):
    """fused = sum_h a_h comb: (dcomb through the product, da [B, 4]) -- da is the same t = dfused . comb for every head."""
    t = (dfused * comb).sum(axis=1)
    return dfused * attn.sum(axis=1, keepdims=True), np.repeat(t[:, None], NHEADS, axis=1)


def backward(dout, saved, params, training, dtype=np.float64):
    """dict of BACKWARD_OUT (dlogit [4, B], dpre [4, B, 128]; dcomb masked by comb > 0), plus dfused and t = dfused . comb.
    ``saved``: comb and SAVED, as the forward pass wrote them or anything else of those shapes."""
    P = cast(params, dtype)
    s = {k: np.asarray(saved[k], dtype=dtype) for k in ("comb",) + SAVED}
    dout = np.asarray(dout, dtype=dtype)
    o = {}
    o["dh3"] = relu_vjp(dout[:, None] * P["w7"][None, :], s["h3"])
    o["dh2"] = relu_vjp(o["dh3"] @ P["w5"], s["h2"])
    o["dhb"] = o["dh2"] @ P["w3"]
    dx, o["dgamma"], o["dbeta"] = batchnorm_vjp(o["dhb"], s["h"], P["gamma"], s["bn_mean"], s["bn_rstd"], training)
    o["dh"] = relu_vjp(dx, s["h"])
    o["dfused"] = o["dh"] @ P["w0"]
    dcomb, da = fusion_vjp(o["dfused"], s["comb"], s["attn"])
    o["t"] = da[:, 0]
    dlogit = softmax_vjp(da, s["attn"])                                        # [B, 4]
    o["dlogit"] = np.ascontiguousarray(dlogit.T)
    o["dpre"] = np.stack([tanh_vjp(dlogit[:, h, None] * P["fw2"][h][None, :], s["hid"][h]) for h in range(NHEADS)])
    for h in range(NHEADS):
        dcomb = dcomb + o["dpre"][h] @ P["fw1"][h]
    o["dcomb"] = relu_vjp(dcomb, s["comb"])
    return o


def fusion_noise_floor(dout, saved, params, training):
    """Bounds (dlogit [4, B], dpre [4, B, 128]) on what a float32 evaluation leaves of the fusion block's gradient when the saved attn rows
    ARE float32 softmax rows: dlogit_h = a_h (t - t s) with s = fl(sum_h a_h).  Each a_h is a quotient rounded to a few units in the last
    place and three additions follow, so |1 - s| <= 4 eps32; t s and the difference round once more: |dlogit_h| <= 8 eps32 a_h |t'|, t'
    the float32 t.  t' itself is two chained 256-term float32 sums (dfused = dh W0, t = dfused . comb) of float32 inputs, within
    512 eps32 of the sums of absolute values (which also covers what the float32 chain in front leaves in dh):
    |t'| <= |t| + 512 eps32 sum_c (sum_k |dh_k W0_kc|) |comb_c|.  dpre_h = dlogit_h w2_h (1 - hid^2): times |w2_h|."""
    eps32 = float(np.finfo(np.float32).eps)
    o = backward(dout, saved, params, training)
    P = cast(params, np.float64)
    a, comb = np.asarray(saved["attn"], np.float64), np.asarray(saved["comb"], np.float64)
    tmag = ((np.abs(o["dh"]) @ np.abs(P["w0"])) * np.abs(comb)).sum(axis=1)
    dl = 8 * eps32 * a.T * (np.abs(o["t"]) + 512 * eps32 * tmag)[None, :]
    return dl, dl[:, :, None] * np.abs(np.stack(P["fw2"]))[:, None, :] * (1 + 4 * eps32)


# ---- the operands of the tests -------------------------------------------------------------------------------------------------------------
DEAD_COLUMNS, OFFSET_COLUMNS = (3, 64, 255), (0, 100, 201)
SATURATING_SCALE = 200.0


def make_params(seed=0, case="ordinary"):
    """Float32 parameters at torch's initialisation scale (weights of standard deviation fan_in ** -0.5) and the running statistics.
    ``case``: "dead_offset": b0 = -50 in DEAD_COLUMNS (fc.0 never fires there: h = 0, variance 0) and +50 in OFFSET_COLUMNS (mean >> spread);
    "saturated": every fw2 times SATURATING_SCALE (logits tens apart: one head takes most rows, the others underflow to 0 in float32)
    and head 1 a copy of head 0 (their logits tie in every row)."""
    rng = np.random.default_rng([seed, 77])
    w = lambda o, i: (rng.standard_normal((o, i)) * i ** -0.5).astype(np.float32)
    b = lambda o: (0.1 * rng.standard_normal(o)).astype(np.float32)
    p = {"fw1": [w(FHID, COMB) for _ in range(NHEADS)], "fb1": [b(FHID) for _ in range(NHEADS)],
         "fw2": [w(1, FHID)[0] for _ in range(NHEADS)], "fb2": [b(1) for _ in range(NHEADS)],
         "w0": w(H1, COMB), "b0": b(H1), "gamma": (1 + 0.3 * rng.standard_normal(H1)).astype(np.float32), "beta": b(H1),
         "w3": w(H2, H1), "b3": b(H2), "w5": w(H3, H2), "b5": b(H3), "w7": w(1, H3)[0], "b7": b(1)}
    running = ((0.5 * rng.standard_normal(H1)).astype(np.float32), rng.uniform(0.5, 2.0, H1).astype(np.float32))
    if case == "dead_offset":
        p["b0"][list(DEAD_COLUMNS)] = -50.0
        p["b0"][list(OFFSET_COLUMNS)] = 50.0
    elif case == "saturated":
        p["fw2"] = [(SATURATING_SCALE * a).astype(np.float32) for a in p["fw2"]]
        for k in PER_HEAD:
            p[k][1] = p[k][0].copy()
    else:
        assert case == "ordinary"
    return p, running


def make_comb(B, seed=0):
    """relu(randn) [B, 256] float32: the real `combined` is a ReLU output, with exact zeros that the dcomb mask needs."""
    return np.maximum(np.random.default_rng([seed, B, 78]).standard_normal((B, COMB)), 0).astype(np.float32)


def make_dout(B, seed=0):
    return np.random.default_rng([seed, B, 79]).standard_normal(B).astype(np.float32)


def off_manifold(B, seed=0):
    """Saved tensors that no forward pass produces, so that every term of the fusion block's backward has full magnitude: attn positive with
    row sums in 0.5 .. 0.9, hid uniform in (-1, 1) and independent of comb, h / h2 / h3 half zeros, arbitrary bn_mean / bn_rstd."""
    rng = np.random.default_rng([seed, B, 80])
    half = lambda *s: np.where(rng.random(s) < 0.5, 0, np.abs(rng.standard_normal(s))).astype(np.float32)
    attn = rng.uniform(0.05, 1.0, (B, NHEADS))
    attn *= rng.uniform(0.5, 0.9, (B, 1)) / attn.sum(axis=1, keepdims=True)
    return {"comb": make_comb(B, seed + 1), "hid": rng.uniform(-0.999, 0.999, (NHEADS, B, FHID)).astype(np.float32),
            "attn": attn.astype(np.float32), "h": half(B, H1), "h2": half(B, H2), "h3": half(B, H3),
            "bn_mean": (0.3 * rng.standard_normal(H1)).astype(np.float32), "bn_rstd": rng.uniform(0.5, 3.0, H1).astype(np.float32)}
