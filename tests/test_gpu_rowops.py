"""GPU: the row / column kernels of csrc/rowops.hip and the dropout stream of csrc/common.h against tests/rowops_oracle.py.

The dropout stream is integer arithmetic and one float32 compare, so its comparisons are equalities: ``ops.dropout`` must give the
oracle's bits, and with it every test elsewhere that says "same stream as bbbp_dropout" becomes absolute.  Everything else is compared
with a float64 reference computed from the same float32 inputs, at the tolerances tests/test_gpu_ops.py applies to these ops: forward
values rtol 1e-5, gradients and column sums rtol 1e-4 with a floor of 2e-5 of the largest element.

Two-row BatchNorm batches are the one place where float32 itself cannot hold those: a column whose two values nearly coincide has a
variance of the order of eps and every result of it is a difference of nearly equal numbers.  There the bound is 4 x S, S being the
largest deviation from float64 of the oracle's float32 restatement of the kernel (same order of operations) on the same case.  Measured
S for the cases here: y of 2 x 63: 1.8e-5 (0.83 x the tolerance), dx of 2 x 64: 1.0e-3 (1.07 x), dx of 2 x 65: 7.8e-5 (0.61 x); every
other case of the file, the shifted columns, the 1e4 offset and 4097 columns included, stays below 0.25 x the tolerance in float32.
"""
import itertools

import numpy as np
import pytest
import torch

from bbbp_amd import _lib, functional, ops
from helpers import assert_close
import rowops_oracle as O

pytestmark = pytest.mark.gpu

FWD = dict(rtol=1e-5)                                   # forward values
GRAD = dict(rtol=1e-4, atol_frac=2e-5)                  # gradients and column sums
HIGH_SEED = 2 ** 60 + 12345


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def close_or_4s(actual, ref64, restated, what, **tol):
    """assert_close; for an ill-conditioned case (see the module docstring) alternatively within 4 x S of float64, S = the deviation
    of the float32 restatement ``restated`` -- a bound that never looks at the kernel's output."""
    try:
        assert_close(actual, ref64, what=what, **tol)
    except AssertionError:
        s = O.deviation(restated, ref64)
        err = O.deviation(actual, ref64)
        print(f"{what}: error {err:.3e}, S = {s:.3e}")
        assert err <= 4 * s, f"{what}: error {err:.3e} beyond the tolerance and beyond 4 x S = {4 * s:.3e}"


# ---- the dropout stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", O.DROPOUT_SEEDS, ids=[hex(s) for s in O.DROPOUT_SEEDS])
def test_dropout_stream_bit_for_bit(dev, seed):
    """Keep mask and values of bbbp_dropout == the numpy restatement of Philox-4x32-10 and the float32 keep decision: lane select,
    key schedule, round count, both key halves, the grid-stride loop (70001 > one pass only if the grid were capped)."""
    for n in O.DROPOUT_LENGTHS:
        x = O.rnd(n, seed=n)
        assert (x != 0).all()
        xd = T(x, dev)
        for p in O.DROPOUT_PS:
            got = N(ops.dropout(xd, p, seed))
            keep = O.keep_scale_like(x, p, seed) != 0
            assert np.array_equal(got != 0, keep), f"keep mask, n={n} p={p}: {int(((got != 0) != keep).sum())} decisions differ"
            assert np.array_equal(got, O.dropout(x, p, seed)), f"values, n={n} p={p}"
        assert np.array_equal(N(ops.dropout(xd, 0.0, seed)), x)                     # p = 0 is a copy


def test_seed_base_moves_the_stream_by_a_wrapping_multiply_add(dev):
    """effective_seed: with the library's seed base pointing at a 64-bit device value b, stream `seed` becomes b * 0x9E3779B97F4A7C15 +
    seed mod 2^64 -- what moves the dropout masks from replay to replay of a captured training step."""
    x = O.rnd(1023, seed=3)
    xd = T(x, dev)
    base_t = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.set_seed_base(base_t.data_ptr())
    try:
        for base in O.SEED_BASES:
            base_t.fill_(base - 2 ** 64 if base >= 2 ** 63 else base)
            for seed in (5, HIGH_SEED):
                assert np.array_equal(N(ops.dropout(xd, 0.25, seed)), O.dropout(x, 0.25, seed, base)), (base, seed)
    finally:
        ops.set_seed_base(0)
    assert np.array_equal(N(ops.dropout(xd, 0.25, 5)), O.dropout(x, 0.25, 5))       # restored: no base


@pytest.mark.parametrize("rows,cols,seed", [(5, 167, 777), (3, 1500, HIGH_SEED)], ids=["narrow", "wide"])
def test_layernorm_dropout_is_the_oracles(dev, rows, cols, seed):
    """z = dropout(x) + residual out of both LayerNorm forms (a wave per row; a work-group per row with one block per float4)."""
    x, r = O.rnd(rows, cols, seed=1), O.rnd(rows, cols, seed=2)
    gam, bet = O.rnd(cols, seed=3), O.rnd(cols, seed=4)
    _, z, _, _ = ops.layernorm_fwd(T(x, dev), T(r, dev), T(gam, dev), T(bet, dev), dropout_p=0.3, seed=seed)
    assert np.array_equal(N(z), O.dropout(x, 0.3, seed) + r)
    assert np.array_equal(N(z) - r == 0, O.keep_scale_like(x, 0.3, seed) == 0)


def test_gemm_epilogue_dropout_is_the_oracles(dev):
    """bbbp_gemm_desc.drop_p: element (m, n) of the product takes the keep decision of stream element m * N + n."""
    M, N_, K, p, seed = 37, 300, 64, 0.1, 987654321
    a, w, bias = T(O.rnd(M, K, seed=21), dev), T(O.rnd(N_, K, seed=22), dev), T(O.rnd(N_, seed=23), dev)
    plain = N(ops.gemm(a, w, trans_b=True, bias=bias, act="relu"))
    got = N(ops.gemm_grouped([dict(a=a, b=w, trans_b=True, bias=bias, act="relu", dropout_p=p, dropout_seed=seed)])[0])
    keep = O.keep_scale_like(plain, p, seed) != 0
    live = plain != 0                                                               # ReLU zeros say nothing about the mask
    assert 0.3 < live.mean() < 0.7
    assert np.array_equal((got != 0)[live], keep[live])
    assert (got[~live] == 0).all()
    assert np.array_equal(got, O.dropout(plain, p, seed))


# ---- softmax ----------------------------------------------------------------------------------------------------------------------
def _softmax_check(dev, x, dp, p, seed, what):
    prob, pd = ops.softmax_fwd(T(x, dev), p, seed)
    assert_close(N(prob), O.softmax_fwd(x), what=f"{what} prob", **FWD)
    scale = O.keep_scale_like(x, p, seed) if p > 0 else None
    if p > 0:
        assert np.array_equal(N(pd), N(prob) * scale), f"{what}: pd != prob * keep-scale"
    else:
        assert pd is prob
    ds = ops.softmax_bwd(T(dp, dev), prob, p, seed)
    assert_close(N(ds), O.softmax_bwd(dp, N(prob), scale), what=f"{what} ds", **GRAD)
    return N(prob)


@pytest.mark.parametrize("p,seed", O.SOFTMAX_DROPOUT, ids=["p0", "p0.3", "p0.3-high-seed"])
@pytest.mark.parametrize("cols", O.SOFTMAX_COLS)
def test_softmax(dev, cols, p, seed):
    """Around the 64-lane boundary, a single column, more than one work-group of four rows; with dropout the forward's dropped copy
    and the backward's dP = dpd * keep-scale use the oracle's mask."""
    for rows in O.SOFTMAX_ROWS:
        _softmax_check(dev, *O.softmax_inputs(rows, cols), p, seed, f"softmax {rows}x{cols} p={p}")


@pytest.mark.parametrize("name", ["offset-1e4", "neg-inf", "dominant"])
def test_softmax_special_rows(dev, name):
    x = O.softmax_special_rows()[name]
    dp = O.rnd(*x.shape, seed=9)
    for p, seed in O.SOFTMAX_DROPOUT:
        prob = _softmax_check(dev, x, dp, p, seed, f"softmax {name} p={p}")
        assert np.isfinite(prob).all() and abs(float(prob.astype(np.float64).sum()) - 1.0) <= 1e-5
        if name == "neg-inf":
            assert (prob[0, ::3] == 0).all() and (prob[0, 1::3] > 0).all()          # exactly 0 where the input is -inf
        if name == "dominant":
            assert prob[0, x.shape[1] // 2] == 1.0 and (np.delete(prob[0], x.shape[1] // 2) == 0).all()   # exp(-300 + ...) underflows


# ---- BatchNorm1d ------------------------------------------------------------------------------------------------------------------
def _bn_bwd_relu(dev, dy, x, gamma, sm, sr, training=True):
    rows, cols = x.shape
    dx, dg, db = torch.empty_like(x), torch.empty(cols, device=dev), torch.empty(cols, device=dev)
    _lib.check(_lib.lib().bbbp_batchnorm1d_bwd_relu(ops._stream(), dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), sm.data_ptr(), sr.data_ptr(),
                                                    dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, cols, int(training)), "bbbp_batchnorm1d_bwd_relu")
    return dx, dg, db


def _batchnorm_case(dev, rows, cols, shifted=False):
    x, gamma, beta, rm, rv, dy = O.batchnorm_inputs(rows, cols, shifted)
    xd, gd, bd, dyd = (T(v, dev) for v in (x, gamma, beta, dy))
    what = f"bn {rows}x{cols}{' shifted' if shifted else ''}"
    # two-row batches: see the module docstring
    check = close_or_4s if rows == 2 else (lambda a, e, restated, what, **tol: assert_close(a, e, what=what, **tol))
    for momentum in O.BN_MOMENTA:
        rmd, rvd = T(rm, dev), T(rv, dev)
        y, sm, sr = ops.batchnorm1d_fwd(xd, gd, bd, rmd, rvd, training=True, momentum=momentum)
        want = O.batchnorm_fwd(x, gamma, beta, rm, rv, True, 1e-5, momentum)
        f32 = O.batchnorm_fwd32(x, gamma, beta, rm, rv, True, 1e-5, momentum)
        for nm, got, w, r in zip(("y", "save_mean", "save_rstd", "running_mean", "running_var"), (y, sm, sr, rmd, rvd), want, f32):
            check(N(got), w, r, f"{what} m={momentum} {nm}", **FWD)
    # training backward with the kernel's own saved statistics
    got = ops.batchnorm1d_bwd(dyd, xd, gd, sm, sr, training=True)
    wantb = O.batchnorm_bwd(dy, x, gamma, want[1], want[2], True)
    f32b = O.batchnorm_bwd32(dy, x, gamma, f32[1], f32[2], True)
    for nm, g, w, r in zip(("dx", "dgamma", "dbeta"), got, wantb, f32b):
        check(N(g), w, r, f"{what} {nm}", **GRAD)
    # eval forward and backward with the given running statistics
    rmd, rvd = T(rm, dev), T(rv, dev)
    y, sm, sr = ops.batchnorm1d_fwd(xd, gd, bd, rmd, rvd, training=False)
    want = O.batchnorm_fwd(x, gamma, beta, rm, rv, False)
    assert np.array_equal(N(rmd), rm) and np.array_equal(N(rvd), rv) and np.array_equal(N(sm), rm)
    assert_close(N(y), want[0], what=f"{what} eval y", **FWD)
    assert_close(N(sr), want[2], what=f"{what} eval rstd", **FWD)
    got = ops.batchnorm1d_bwd(dyd, xd, gd, sm, sr, training=False)
    for nm, g, w in zip(("dx", "dgamma", "dbeta"), got, O.batchnorm_bwd(dy, x, gamma, want[1], want[2], False)):
        assert_close(N(g), w, what=f"{what} eval {nm}", **GRAD)
    # x = relu(pre): about half the entries are exactly 0 and the ReLU's backward rides along; dgamma / dbeta are not gated
    xa = np.maximum(x, 0)
    xad = T(xa, dev)
    _, sm, sr = ops.batchnorm1d_fwd(xad, gd, bd, T(rm, dev), T(rv, dev), training=True)
    want = O.batchnorm_fwd(xa, gamma, beta, rm, rv, True)
    f32 = O.batchnorm_fwd32(xa, gamma, beta, rm, rv, True)
    got = _bn_bwd_relu(dev, dyd, xad, gd, sm, sr)
    f32b = O.batchnorm_bwd32(dy, xa, gamma, f32[1], f32[2], True, relu_gate=True)
    for nm, g, w, r in zip(("dx", "dgamma", "dbeta"), got, O.batchnorm_bwd(dy, xa, gamma, want[1], want[2], True, relu_gate=True), f32b):
        check(N(g), w, r, f"{what} relu-gated {nm}", **GRAD)
    assert (N(got[0])[xa == 0] == 0).all()


@pytest.mark.parametrize("cols", O.BN_COLS)
@pytest.mark.parametrize("rows", O.BN_ROWS)
def test_batchnorm(dev, rows, cols):
    """Across the 64-column work-group boundary and the 16-row stride, in training mode: y, both saved and both running statistics
    (non-trivial starting values, two momenta), training / eval / ReLU-gated backward."""
    _batchnorm_case(dev, rows, cols)


def test_batchnorm_shifted_columns(dev):
    """A third of the columns carries a mean of 30 standard deviations."""
    _batchnorm_case(dev, *O.BN_SHIFTED, shifted=True)


@pytest.mark.parametrize("cols", O.SHARD_COLS)
def test_sharded_batchnorm_pieces_compose_to_batchnorm(dev, cols):
    """The exact-global-batch BatchNorm of distributed.py without torch.distributed: bbbp_column_moments per shard (no centre, then about
    the global mean), shard sums added on the host, bbbp_batchnorm1d_bwd_apply with the global sums == BatchNorm over the whole batch."""
    L = _lib.lib()
    n = sum(O.SHARD_ROWS)
    x, gamma, beta, rm, rv, dy = O.batchnorm_inputs(n, cols)
    cuts = np.cumsum((0,) + O.SHARD_ROWS)
    shards = [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    xs, dys, gd, bd = [T(x[s], dev) for s in shards], [T(dy[s], dev) for s in shards], T(gamma, dev), T(beta, dev)

    def moments(xd, centre):
        st = torch.empty((2, cols), device=dev)
        _lib.check(L.bbbp_column_moments(ops._stream(), xd.data_ptr(), None if centre is None else centre.data_ptr(), st[0].data_ptr(),
                                         st[1].data_ptr(), xd.shape[0], cols), "bbbp_column_moments")
        return N(st).astype(np.float64)

    s1 = np.zeros(cols)
    for xd, s in zip(xs, shards):
        m = moments(xd, None)
        assert_close(m[0], O.column_moments(x[s])[0], what="sum", **GRAD)
        assert_close(m[1], O.column_moments(x[s])[1], what="sum of squares", **GRAD)
        s1 += m[0]
    mean = T((s1 / n).astype(np.float32), dev)
    s2 = np.zeros(cols)
    for xd, s in zip(xs, shards):
        m = moments(xd, mean)
        assert_close(m[1], O.column_moments(x[s], N(mean))[1], what="centred sum of squares", **GRAD)
        s2 += m[1]
    var = T((s2 / n).astype(np.float32), dev)
    ys, stats = [], []
    for xd in xs:
        y, sm, sr = ops.batchnorm1d_fwd(xd, gd, bd, mean, var, training=False)
        ys.append(N(y)); stats.append((sm, sr))
    sums = np.zeros((2, cols))
    for xd, dyd, (sm, sr) in zip(xs, dys, stats):
        _, dg, db = ops.batchnorm1d_bwd(dyd, xd, gd, sm, sr, training=True)
        sums += np.stack([N(db), N(dg)]).astype(np.float64)
    sums_d = T(sums.astype(np.float32), dev)
    dxs = []
    for xd, dyd, (sm, sr) in zip(xs, dys, stats):
        dx = torch.empty_like(xd)
        _lib.check(L.bbbp_batchnorm1d_bwd_apply(ops._stream(), dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), sm.data_ptr(), sr.data_ptr(),
                                                sums_d[0].data_ptr(), sums_d[1].data_ptr(), dx.data_ptr(), xd.shape[0], cols, n), "bbbp_batchnorm1d_bwd_apply")
        dxs.append(N(dx))
    want = O.batchnorm_fwd(x, gamma, beta, rm, rv, True)
    wdx, wdg, wdb = O.batchnorm_bwd(dy, x, gamma, want[1], want[2], True)
    assert_close(np.concatenate(ys), want[0], what="sharded y", **FWD)
    assert_close(sums[1], wdg, what="sharded dgamma", **GRAD)
    assert_close(sums[0], wdb, what="sharded dbeta", **GRAD)
    assert_close(np.concatenate(dxs), wdx, what="sharded dx", **GRAD)


# ---- bias_act_bwd and mse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", O.BIAS_ACT_SCALES)
@pytest.mark.parametrize("act", [None, "relu", "tanh"])
def test_bias_act_bwd(dev, act, scale):
    """Column counts around the 16-column block, row counts around the 32 row lanes; dy and y are column slices of wider buffers whose
    other columns must stay untouched; without an activation dy is only summed."""
    code = ops.ACT[act]
    for rows, cols in itertools.product(O.BIAS_ACT_ROWS, O.BIAS_ACT_COLS):
        pre, dy = O.rnd(rows, cols, seed=rows + cols), O.rnd(rows, cols, seed=rows + cols + 1)
        y = np.maximum(pre, 0) if act == "relu" else np.tanh(pre).astype(np.float32)
        wide_dy, wide_y = T(O.rnd(rows, cols + 7, seed=5), dev), T(O.rnd(rows, cols + 5, seed=6), dev)
        wide_dy[:, 3:3 + cols] = T(dy, dev)
        wide_y[:, 2:2 + cols] = T(y, dev)
        before = wide_dy.clone()
        db = ops.bias_act_bwd(wide_dy[:, 3:3 + cols], wide_y[:, 2:2 + cols] if act else None, act=act, scale=scale)
        want, wdb = O.bias_act_bwd(dy, y, code, scale)
        what = f"bias_act_bwd {act} x{scale} {rows}x{cols}"
        assert torch.equal(wide_dy[:, :3], before[:, :3]) and torch.equal(wide_dy[:, 3 + cols:], before[:, 3 + cols:]), what
        if act is None:
            assert torch.equal(wide_dy, before), what
        assert_close(N(wide_dy[:, 3:3 + cols]), want, what=what, **FWD)
        assert_close(N(db), wdb, what=what + " db", **GRAD)


@pytest.mark.parametrize("gs", O.MSE_SCALES)
@pytest.mark.parametrize("n", O.MSE_NS)
def test_mse(dev, n, gs):
    """The stride-256 loop takes a second trip from n = 257 on, and every thread of the reduction tree holds a non-zero term."""
    pred, tgt = O.rnd(n, seed=n), O.rnd(n, seed=n + 1)
    loss, dpred = ops.mse(T(pred, dev), T(tgt, dev), gs)
    wl, wd = O.mse(pred, tgt, gs)
    assert_close(N(loss), [wl], what="mse", **FWD)
    assert_close(N(dpred), wd, what="dmse", **FWD)
    loss, dpred = ops.mse(T(pred, dev), T(pred, dev), gs)
    assert float(loss) == 0.0 and (N(dpred) == 0).all()


# ---- attention fusion combine -----------------------------------------------------------------------------------------------------
class _Ctx:
    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


@pytest.mark.parametrize("hd", O.FUSION_HIDDEN)
@pytest.mark.parametrize("nh", O.FUSION_HEADS)
def test_fusion_combine(dev, nh, hd):
    """functional._FusionCombine forward and backward.  out = combined * sum_h attn_h, so the true gradient of every scorer is 0 and the
    kernel's dlogit is rounding noise: the backward is held to its structure -- dcombined exactly, dlogit within the derived bound
    (|1 - asum| <= nh * 2^-24 and one rounding of t * asum, times two), dpre as the product it is defined as."""
    L = _lib.lib()
    worst = 0.0
    for dim, rows in itertools.product(O.FUSION_DIMS, O.FUSION_ROWS):
        what = f"fusion nh={nh} hd={hd} dim={dim} rows={rows}"
        comb, hid, w2, b2, dout = O.fusion_inputs(nh, hd, dim, rows)
        cd, hdv, dd = T(comb, dev), T(hid, dev), T(dout, dev)
        w2d, b2d = [T(w2[h][None], dev) for h in range(nh)], [T(b2[h:h + 1], dev) for h in range(nh)]
        ctx = _Ctx()
        out = functional._FusionCombine.forward(ctx, cd, hdv, *w2d, *b2d)
        attn = N(ctx.saved_tensors[2])
        _, want_attn, want_out = O.fusion_combine_fwd(comb, hid, w2, b2)
        assert_close(attn, want_attn, what=what + " attn", **FWD)
        assert_close(N(out), want_out, what=what + " out", **FWD)
        grads = functional._FusionCombine.backward(ctx, dd)
        assert len(grads) == 2 + 2 * nh
        dcomb, dpre = N(grads[0]), N(grads[1])
        # the same call once more, to see dlogit
        dcomb2, dlogit_d, dpre2 = torch.empty_like(cd), torch.empty((nh, rows), device=dev), torch.empty_like(hdv)
        _lib.check(L.bbbp_fusion_combine_bwd(ops._stream(), dd.data_ptr(), cd.data_ptr(), hdv.data_ptr(), ctx.saved_tensors[2].data_ptr(),
                                             _lib.ptr_array([w.data_ptr() for w in w2d]), dcomb2.data_ptr(), dlogit_d.data_ptr(), dpre2.data_ptr(),
                                             rows, dim, hd, nh), "bbbp_fusion_combine_bwd")
        dlogit = N(dlogit_d)
        assert np.array_equal(N(dcomb2), dcomb) and np.array_equal(N(dpre2), dpre), what
        asum = np.zeros(rows, np.float32)
        for h in range(nh):
            asum = asum + attn[:, h]                                                 # float32, head order
        assert np.array_equal(dcomb, dout * asum[:, None]), what + " dcombined"
        assert np.isfinite(dlogit).all(), what
        bound = attn.T.astype(np.float64) * np.abs(dout.astype(np.float64) * comb.astype(np.float64)).sum(axis=1) * (nh + 2) * 2.0 ** -23
        worst = max(worst, float((np.abs(dlogit) / np.maximum(bound, 1e-300)).max()))
        assert (np.abs(dlogit) <= bound).all(), f"{what}: dlogit up to {worst:.2f} x its bound"
        h64 = hid.astype(np.float64)
        assert_close(dpre, dlogit.astype(np.float64)[:, :, None] * w2.astype(np.float64)[:, None, :] * (1.0 - h64 * h64), rtol=1e-6, atol_frac=0.0,
                     what=what + " dpre")
        for h in range(nh):                          # the scorers' parameter gradients are sums over the rows of the same dlogit
            dl = dlogit[h].astype(np.float64)
            assert abs(float(grads[2 + nh + h]) - dl.sum()) <= 1e-6 * np.abs(dl).sum(), what + " db2"
            dw2 = N(grads[2 + h]).reshape(hd)
            assert (np.abs(dw2 - dl @ h64[h]) <= 2e-6 * (np.abs(dl) @ np.abs(h64[h]))).all(), what + " dw2"
    print(f"fusion nh={nh} hd={hd}: dlogit at most {worst:.3f} x its bound")


# ---- empties and refusals ---------------------------------------------------------------------------------------------------------
def test_empty_batches(dev):
    e = torch.empty((0, 5), device=dev)
    prob, pd = ops.softmax_fwd(e, 0.3, 7)
    assert prob.shape == pd.shape == (0, 5) and ops.softmax_bwd(e, prob, 0.3, 7).shape == (0, 5)
    assert ops.dropout(e, 0.3, 7).shape == (0, 5)
    g, b, rm, rv = (T(O.rnd(5, seed=i), dev) for i in range(4))
    rv = rv.abs() + 0.5
    y, sm, sr = ops.batchnorm1d_fwd(e, g, b, rm, rv, training=False)
    dx, dg, db = ops.batchnorm1d_bwd(e, e, g, sm, sr, training=False)
    assert y.shape == dx.shape == (0, 5) and (N(dg) == 0).all() and (N(db) == 0).all()
    for act in (None, "relu", "tanh"):
        db = ops.bias_act_bwd(e, e if act else None, act=act)
        assert (N(db) == 0).all()
    out = functional._FusionCombine.forward(_Ctx(), e, torch.empty((2, 0, 3), device=dev), *[T(O.rnd(1, 3, seed=h), dev) for h in range(2)],
                                            *[T(O.rnd(1, seed=h), dev) for h in range(2)])
    assert out.shape == (0, 5)


def test_refusals(dev):
    """Arguments a kernel would index unchecked are refused before any launch."""
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError):
        ops.mse(z(0), z(0))
    with pytest.raises(RuntimeError):
        ops.mse(z(8), z(7))
    with pytest.raises(RuntimeError):
        ops.dropout(z(8), 1.0, 3)
    nine = [z(1, 4) for _ in range(9)] + [z(1) for _ in range(9)]
    with pytest.raises(RuntimeError, match="num_heads"):
        functional._FusionCombine.forward(_Ctx(), z(2, 6), z(9, 2, 4), *nine)
    with pytest.raises(RuntimeError, match="num_heads"):
        _lib.check(_lib.lib().bbbp_fusion_combine_bwd(ops._stream(), z(2, 6).data_ptr(), z(2, 6).data_ptr(), z(9, 2, 4).data_ptr(), z(2, 9).data_ptr(),
                                                      _lib.ptr_array([w.data_ptr() for w in nine[:9]]), z(2, 6).data_ptr(), z(9, 2).data_ptr(),
                                                      z(9, 2, 4).data_ptr(), 2, 6, 4, 9), "bbbp_fusion_combine_bwd")
    x, v = z(4, 6), z(6)
    for bad in (dict(dy=z(3, 6)), dict(dy=z(4, 5)), dict(gamma=z(5)), dict(save_mean=z(7)), dict(save_rstd=z(6, 2)[:, 0]), dict(dy=torch.zeros(4, 6))):
        args = dict(dy=z(4, 6), x=x, gamma=v, save_mean=v, save_rstd=v)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.batchnorm1d_bwd(args["dy"], args["x"], args["gamma"], args["save_mean"], args["save_rstd"], training=True)
    for bad in (dict(gamma=z(5)), dict(beta=z(7)), dict(running_mean=z(5)), dict(running_var=z(12)[::2])):
        args = dict(gamma=v, beta=v, running_mean=v, running_var=z(6) + 1)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.batchnorm1d_fwd(x, args["gamma"], args["beta"], args["running_mean"], args["running_var"], training=False)
    with pytest.raises(RuntimeError):
        ops.softmax_bwd(z(4, 6), z(4, 5))
    with pytest.raises(RuntimeError):
        ops.softmax_bwd(z(4, 6), z(3, 6))
    with pytest.raises(RuntimeError):
        ops.bias_act_bwd(z(4, 6), z(3, 6), act="relu")
    with pytest.raises(RuntimeError):
        ops.bias_act_bwd(z(4, 6), z(4, 5), act="tanh")
