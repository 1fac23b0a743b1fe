"""GPU: the four kernels of csrc/head.hip (head_a / head_b forward, head_bwd_a / head_bwd_c backward), called directly through ops.head_fwd /
ops.head_bwd, every tensor they write compared element-wise with the float64 oracle of tests/head_oracle.py.

Batch sizes are the smallest that reach each branch of the 16-row blocking: 1 (eval only), 2 (n / (n - 1) = 2), 15 (one short block), 16
(exactly one), 17 (a block of one row), 33, 100, 530 (34 blocks, a 2-row tail: the merge loops).  The backward kernels take the saved
activations as arguments, so besides the forward pass's own outputs they are fed tensors no forward pass produces (``H.off_manifold``):
on real activations sum_h a_h = 1 makes the fusion block's gradient -- dlogit, dpre, the product sum_h dpre_h W1_h -- rounding noise,
and only off that manifold does a wrong head index or stride in it change anything.
Bound: the project's for float32 kernels against float64 (TOL), in every regime -- the offset columns (mean >> spread), ill-conditioned
in float32 by construction, meet it too (worst ratio 0.10 of the bound, hb at B = 2), so no case is held to a float32 yardstick.
Worst error / bound measured on the MI355X: forward hid 0.01, attn 0.13 (saturated), fused 0.002, h 0.01, hb 0.10, bn_mean 0.002,
bn_rstd 0.14 (B = 2), h2 0.04, h3 0.05, out 0.05, running statistics 0.001; backward dh3 0 (one rounding), dh2 0.005, dhb 0.01, dh 0.02,
dcomb 0.01, dgamma 0.01, dbeta 0.01; off the manifold dlogit 0.02, dpre 0.02, dcomb 0.01; on it |dlogit|, |dpre| <= 0.13 of their floor."""
import functools

import numpy as np
import pytest
import torch

import head_oracle as H
import poison
from bbbp_amd import ops
from helpers import assert_close

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol_frac=2e-5)          # float32 kernels against float64, as test_gpu_attention.py / _conv_case / _layernorm_case
BATCHES = (2, 15, 16, 17, 33, 100, 530)
FWD_CASES = [(1, False)] + [(B, training) for B in BATCHES for training in (True, False)]
STATS = ("running_mean", "running_var")
GRADS = ("dh3", "dh2", "dhb", "dh", "dcomb", "dgamma", "dbeta")


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
def T(a, dev):
    return torch.tensor(a).to(dev)             # a copy: the cached references are read-only


def N(t):
    return t.detach().cpu().numpy()


def to_dev(p, dev):
    return {k: ([T(a, dev) for a in v] if k in H.PER_HEAD else T(v, dev)) for k, v in p.items()}


def freeze(d):
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def operands(case="ordinary"):
    p, running = H.make_params(case=case)
    freeze(p)
    for r in running:
        r.setflags(write=False)
    return p, running


@functools.lru_cache(maxsize=None)
def forward_reference(case, B, training, concat=False):
    """Float64 oracle results of one forward case: computed once, shared, read-only."""
    p, running = operands(case)
    return freeze(H.forward(H.make_comb(B), p, running, training, concat=concat))


def run_forward(dev, case, B, training, **kw):
    """The op on a case's operands: (outputs as numpy by name, running statistics after the call included; the device tensors)."""
    p, running = operands(case)
    rm, rv = T(running[0], dev), T(running[1], dev)
    o = ops.head_fwd(T(H.make_comb(B), dev), to_dev(p, dev), rm, rv, training, **kw)
    got = {k: (None if v is None else N(v)) for k, v in o.items()}
    got["running_mean"], got["running_var"] = N(rm), N(rv)
    return got, o


def ratio(got, want, rtol, atol_frac):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float((err / (rtol * np.abs(want) + atol_frac * np.abs(want).max() + 1e-30)).max())


def close(got, want, what):
    """assert_close at TOL; prints the worst error ratio first (1.0 = at the bound)."""
    print(f"[head] {what}: worst ratio {ratio(got, want, **TOL):.3f} scale {np.abs(want).max():.3e}")
    assert np.isfinite(got).all(), f"{what}: not finite"
    assert_close(got, want, what=what, **TOL)


def saved_of(fwd, comb):
    return dict({k: fwd[k] for k in H.SAVED}, comb=comb)


def run_backward(dev, dout, saved, p, training, **kw):
    s = {k: T(v, dev) for k, v in saved.items()}
    return {k: N(v) for k, v in ops.head_bwd(T(dout, dev), s["comb"], s, to_dev(p, dev), training, **kw).items()}


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,training", FWD_CASES)
def test_forward_against_float64(dev, B, training):
    want = forward_reference("ordinary", B, training)
    got, _ = run_forward(dev, "ordinary", B, training)
    for k in H.FORWARD_OUT + STATS:
        close(got[k], want[k], f"fwd B={B} training={training} {k}")
    if not training:
        running = operands()[1]
        assert np.array_equal(got["running_mean"], running[0]) and np.array_equal(got["running_var"], running[1])
    assert (got["attn"] > 0).all() and np.abs(got["attn"].astype(np.float64).sum(axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("B,training", [(B, True) for B in BATCHES] + [(17, False), (530, False)])
def test_forward_with_dead_and_offset_columns(dev, B, training):
    """b0 = -50: fc.0 never fires in that column, h = 0 in every row, variance exactly 0, rstd = eps ** -0.5 = 316, hb = beta bit for bit.
    b0 = +50: the column's mean is tens of its spread, where a one-pass variance would cancel; per-block (mean, M2) and Chan's merge do not."""
    want = forward_reference("dead_offset", B, training)
    got, _ = run_forward(dev, "dead_offset", B, training)
    for k in H.FORWARD_OUT + STATS:
        close(got[k], want[k], f"dead/offset B={B} training={training} {k}")
    dead = list(H.DEAD_COLUMNS)
    beta = operands("dead_offset")[0]["beta"]
    assert (got["h"][:, dead] == 0).all()
    if training:
        assert (got["bn_mean"][dead] == 0).all() and np.allclose(got["bn_rstd"][dead], H.EPS ** -0.5, rtol=1e-6)
        assert np.array_equal(got["hb"][:, dead], np.broadcast_to(beta[dead], (B, len(dead))))


@pytest.mark.parametrize("B", [17, 100])
def test_forward_with_a_saturated_head_softmax(dev, B):
    """Logits tens to hundreds apart: rows that one head takes alone (the others underflow to 0) and, heads 0 and 1 being copies, rows where
    two logits tie at the maximum."""
    want = forward_reference("saturated", B, True)
    got, _ = run_forward(dev, "saturated", B, True)
    a = got["attn"]
    assert np.isfinite(a).all() and np.abs(a.astype(np.float64).sum(axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps
    assert ((a == 0).sum(axis=1) == 3).any() and np.array_equal(a[:, 0], a[:, 1]) and (a[:, 0] == 0.5).any()
    for k in H.FORWARD_OUT + STATS:
        close(got[k], want[k], f"saturated B={B} {k}")


@pytest.mark.parametrize("B,training", [(17, True), (100, True), (100, False)])
def test_forward_concat_skips_the_fusion_block(dev, monkeypatch, B, training):
    """concat = 1: fused IS combined.  h .. out against the oracle, the same bits with and without fusion buffers, and buffers that are
    handed in keep their poison."""
    want = forward_reference("ordinary", B, training, concat=True)
    plain, _ = run_forward(dev, "ordinary", B, training, concat=True)
    assert plain["hid"] is None and plain["attn"] is None and plain["fused"] is None
    for k in H.FORWARD_OUT[3:] + STATS:
        close(plain[k], want[k], f"concat B={B} training={training} {k}")
    for fill in poison.FILLS:
        with poison.poisoned_allocations(monkeypatch, fill) as pa:
            bufs = [torch.empty(shape, device=dev, dtype=torch.float32) for shape in ((4, B, 128), (B, 4), (B, 256))]
            got, _ = run_forward(dev, "ordinary", B, training, concat=True, fusion_out=bufs)
            torch.cuda.synchronize()
            pa.check()
            for b in bufs:
                assert bool((b.view(torch.uint8) == fill).all()), "the skipped fusion block wrote one of its outputs"
        for k in H.FORWARD_OUT[3:] + STATS:
            assert np.array_equal(got[k], plain[k]), k


# ---- backward --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,training", [("ordinary", B, t) for B in BATCHES for t in (True, False)] + [("ordinary", 1, False)]
                         + [("dead_offset", 17, True), ("dead_offset", 100, True), ("dead_offset", 100, False)])
def test_backward_on_the_forward_ops_own_outputs(dev, case, B, training):
    """Saved tensors = what ops.head_fwd wrote; the oracle is evaluated on those same float32 tensors, so the ReLU gates are inputs and no
    near-tie can fall on two sides.  The fusion block's gradient is noise here: bounded by its derived floor, not compared."""
    p = operands(case)[0]
    comb, dout = H.make_comb(B), H.make_dout(B)
    fwd, _ = run_forward(dev, case, B, training)
    saved = saved_of(fwd, comb)
    want = H.backward(dout, saved, p, training)
    got = run_backward(dev, dout, saved, p, training)
    for k in GRADS:
        close(got[k], want[k], f"bwd {case} B={B} training={training} {k}")
    dl_floor, dpre_floor = H.fusion_noise_floor(dout, saved, p, training)
    for k, floor in (("dlogit", dl_floor), ("dpre", dpre_floor)):
        print(f"[head] bwd {case} B={B} training={training} {k}: worst |value| / floor {(np.abs(got[k]) / (floor + 1e-300)).max():.3f}")
        assert np.isfinite(got[k]).all() and (np.abs(got[k]) <= floor).all(), k
    if case == "dead_offset":
        dead = list(H.DEAD_COLUMNS)
        assert (got["dh"][:, dead] == 0).all() and (not training or (got["dgamma"][dead] == 0).all())      # eval: xhat = -running_mean rstd


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", [17, 100])
def test_backward_off_the_manifold(dev, B, training):
    """attn rows that sum to 0.5 .. 0.9, hid independent of comb, half-zero h / h2 / h3, arbitrary statistics, a distinct fw1 / fw2 per
    head: dlogit, dpre and the W1 product in dcomb at full magnitude, against the same chain-rule formulas in float64."""
    p = operands()[0]
    saved, dout = H.off_manifold(B), H.make_dout(B)
    want = H.backward(dout, saved, p, training)
    got = run_backward(dev, dout, saved, p, training)
    for k in H.BACKWARD_OUT:
        close(got[k], want[k], f"off-manifold B={B} training={training} {k}")
    assert np.abs(want["dlogit"]).max() > 1e-3 * np.abs(want["t"]).max()          # not noise here


# ---- addresses, ranks, poison, errors ----------------------------------------------------------------------------------------------------------
def test_parameters_at_odd_float_offsets_give_the_same_bits(dev):
    """Every weight and bias a slice of one flat buffer starting at an odd float offset (4-byte but not 8- or 16-byte aligned), as in the
    model's flat parameter buffer: the f32x4g / f32x2g loads may not assume more."""
    B = 33
    p, running = operands()
    leaves = [(k, i, a) for k, v in p.items() for i, a in (enumerate(v) if k in H.PER_HEAD else [(None, v)])]
    flat = torch.zeros(sum(a.size + 2 for _, _, a in leaves) + 1, device=dev)
    assert flat.data_ptr() % 16 == 0
    odd, at = {k: [None] * 4 for k in H.PER_HEAD}, 1
    for k, i, a in leaves:
        view = flat[at:at + a.size].view(a.shape)
        view.copy_(T(a, dev))
        assert view.data_ptr() % 8 == 4
        if i is None:
            odd[k] = view
        else:
            odd[k][i] = view
        at += a.size + (2 if a.size % 2 == 0 else 1)          # the next start is odd again
    comb, dout = T(H.make_comb(B), dev), T(H.make_dout(B), dev)
    results = []
    for params in (to_dev(p, dev), odd):
        rm, rv = T(running[0], dev), T(running[1], dev)
        f = ops.head_fwd(comb, params, rm, rv, True)
        b = ops.head_bwd(dout, comb, f, params, True)
        results.append(dict(f, running_mean=rm, running_var=rv, **b))
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    close(N(results[1]["out"]), forward_reference("ordinary", B, True)["out"], "odd offsets out")


def two_ranks(dev, per, comb, dout, p, running):
    """Two ranks emulated in one process: one shared, zero-initialised `partial` per direction; rank 0 then rank 1, then both again so that
    each second launch sees both slots -- the second pass, from fresh running statistics, is the result."""
    P = to_dev(p, dev)
    shard = [T(comb[r * per:(r + 1) * per], dev) for r in range(2)]
    dshard = [T(dout[r * per:(r + 1) * per], dev) for r in range(2)]
    blocks = (per + 15) // 16
    partial_f, partial_b = (torch.zeros(2 * blocks * 2 * 256, device=dev) for _ in range(2))
    for _ in range(2):
        fwd, stats = [], []
        for r in range(2):
            rm, rv = T(running[0], dev), T(running[1], dev)
            fwd.append(ops.head_fwd(shard[r], P, rm, rv, True, world=2, rank=r, partial=partial_f))
            stats.append((rm, rv))
    for _ in range(2):
        bwd = [ops.head_bwd(dshard[r], shard[r], fwd[r], P, True, world=2, rank=r, partial=partial_b) for r in range(2)]
    return fwd, stats, bwd


def test_two_ranks_of_32_rows_are_bit_identical_to_one_call_on_64(dev):
    """Same 16-row block partition, same merge order: out, hb, the statistics, dh and dcomb carry the single call's bits.  dgamma / dbeta
    are each rank's LOCAL sums (the caller reduces parameter gradients), while dh used the global ones."""
    per = 32
    p, running = operands()
    comb, dout = H.make_comb(2 * per), H.make_dout(2 * per)
    fwd, stats, bwd = two_ranks(dev, per, comb, dout, p, running)
    rm, rv = T(running[0], dev), T(running[1], dev)
    one = ops.head_fwd(T(comb, dev), to_dev(p, dev), rm, rv, True)
    one_b = ops.head_bwd(T(dout, dev), T(comb, dev), one, to_dev(p, dev), True)
    for k in ("attn", "fused", "h", "hb", "h2", "h3", "out"):
        assert torch.equal(torch.cat([fwd[0][k], fwd[1][k]]), one[k]), k
    for r in range(2):
        for k in ("bn_mean", "bn_rstd"):
            assert torch.equal(fwd[r][k], one[k]), (r, k)
        assert torch.equal(stats[r][0], rm) and torch.equal(stats[r][1], rv)
    for k in ("dh3", "dh2", "dhb", "dh", "dcomb"):
        assert torch.equal(torch.cat([bwd[0][k], bwd[1][k]]), one_b[k]), k
    want = H.backward(dout, saved_of({k: N(v) for k, v in one.items()}, comb), p, True)
    xhat = (N(one["h"]).astype(np.float64) - N(one["bn_mean"])) * N(one["bn_rstd"]).astype(np.float64)
    for r in range(2):
        rows = slice(r * per, (r + 1) * per)
        close(N(bwd[r]["dgamma"]), (want["dhb"][rows] * xhat[rows]).sum(axis=0), f"rank {r} of 2 x 32: local dgamma")
        close(N(bwd[r]["dbeta"]), want["dhb"][rows].sum(axis=0), f"rank {r} of 2 x 32: local dbeta")
    close(N(bwd[0]["dgamma"]) + N(bwd[1]["dgamma"]), want["dgamma"], "2 x 32: dgamma summed over the ranks")
    close(N(one_b["dh"]), want["dh"], "64 rows: dh")


def test_two_ranks_of_20_rows_against_the_oracle_on_40(dev):
    """Ragged blocks inside each rank (16 + 4 rows, twice): block sizes in the merge come from the rank's own B."""
    per = 20
    p, running = operands()
    comb, dout = H.make_comb(2 * per), H.make_dout(2 * per)
    fwd, stats, bwd = two_ranks(dev, per, comb, dout, p, running)
    want = H.forward(comb, p, running, True)
    cat = {k: np.concatenate([N(fwd[0][k]), N(fwd[1][k])], axis=1 if k == "hid" else 0) for k in H.FORWARD_OUT if k not in ("bn_mean", "bn_rstd")}
    for k, v in cat.items():
        close(v, want[k], f"2 x 20 {k}")
    for r in range(2):
        for k in ("bn_mean", "bn_rstd"):
            close(N(fwd[r][k]), want[k], f"rank {r} of 2 x 20 {k}")
        close(N(stats[r][0]), want["running_mean"], f"rank {r} of 2 x 20 running_mean")
        close(N(stats[r][1]), want["running_var"], f"rank {r} of 2 x 20 running_var")
    saved = dict(cat, comb=comb, bn_mean=N(fwd[0]["bn_mean"]), bn_rstd=N(fwd[0]["bn_rstd"]))
    wb = H.backward(dout, saved, p, True)
    for k in ("dh3", "dh2", "dhb", "dh", "dcomb"):
        close(np.concatenate([N(bwd[0][k]), N(bwd[1][k])]), wb[k], f"2 x 20 {k}")
    xhat = (saved["h"].astype(np.float64) - saved["bn_mean"]) * saved["bn_rstd"].astype(np.float64)
    for r in range(2):
        rows = slice(r * per, (r + 1) * per)
        close(N(bwd[r]["dgamma"]), (wb["dhb"][rows] * xhat[rows]).sum(axis=0), f"rank {r} of 2 x 20: local dgamma")
        close(N(bwd[r]["dbeta"]), wb["dhb"][rows].sum(axis=0), f"rank {r} of 2 x 20: local dbeta")


def test_poisoned_outputs_and_workspace(dev, monkeypatch):
    """Outputs and `partial` out of poisoned pools, `partial` larger than needed: the same bits under every fill, guard bands and the unused
    tail of `partial` untouched -- the kernels read nothing they did not write and write no row >= B (the outputs hold exactly B rows)."""
    B, extra = 33, 1000
    p, running = operands()
    need = ((B + 15) // 16) * 2 * 256
    comb, dout, P = T(H.make_comb(B), dev), T(H.make_dout(B), dev), to_dev(p, dev)
    results = []
    for fill in poison.FILLS:
        rm, rv = T(running[0], dev), T(running[1], dev)
        with poison.poisoned_allocations(monkeypatch, fill) as pa:
            partial_f, partial_b = (torch.empty(need + extra, device=dev, dtype=torch.float32) for _ in range(2))
            f = ops.head_fwd(comb, P, rm, rv, True, partial=partial_f)
            b = ops.head_bwd(dout, comb, f, P, True, partial=partial_b)
            torch.cuda.synchronize()
            assert pa.check() == 2 + 10 + 9
            for part in (partial_f, partial_b):
                assert bool((part[need:].view(torch.uint8) == fill).all()), "the tail of partial was written"
        results.append(dict(f, running_mean=rm, running_var=rv, **b))
    for other in results[1:]:
        for k in results[0]:
            assert torch.equal(results[0][k], other[k]), k
    want = forward_reference("ordinary", B, True)
    for k in ("out", "hb", "running_var"):
        close(N(results[0][k]), want[k], f"poisoned B={B} {k}")


def test_training_on_one_row_is_refused_and_eval_works(dev):
    p, running = operands()
    P, comb = to_dev(p, dev), T(H.make_comb(1), dev)
    rm, rv = T(running[0], dev), T(running[1], dev)
    with pytest.raises(RuntimeError, match=r"Expected more than 1 value per channel when training, got input size \[1, 256\]"):
        ops.head_fwd(comb, P, rm, rv, True)
    f = ops.head_fwd(comb, P, rm, rv, False)
    close(N(f["out"]), forward_reference("ordinary", 1, False)["out"], "eval B=1 out")
    with pytest.raises(RuntimeError, match="Expected more than 1 value per channel"):
        ops.head_bwd(T(H.make_dout(1), dev), comb, f, P, True)
    b = ops.head_bwd(T(H.make_dout(1), dev), comb, f, P, False)
    want = H.backward(H.make_dout(1), saved_of({k: N(v) for k, v in f.items()}, H.make_comb(1)), p, False)
    close(N(b["dcomb"]), want["dcomb"], "eval B=1 dcomb")
    assert np.array_equal(N(rm), running[0]) and np.array_equal(N(rv), running[1])
