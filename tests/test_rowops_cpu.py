"""CPU: the numpy oracle of the row kernels (tests/rowops_oracle.py) is pinned from outside -- its Philox core to the published known
answers of Philox4x32-10, its stream to the keep rate and the independence a dropout stream must have, its float64 references to torch's
float64 autograd on the case lists the GPU tests use -- and the float32 restatements it derives tolerances from are measured here."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowops_oracle as O

# (counter, key) -> output of Philox4x32-10: the known-answer vectors shipped with Random123 (kat_vectors)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

HIGH_SEED = 2 ** 60 + 12345
REF_BOUND = 1e-12


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_core_known_answers(ctr, key, want):
    assert tuple(int(w) for w in O.philox4x32_10(*ctr, *key)) == want


def test_philox_core_is_vectorised():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64).T
    key = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(O.philox4x32_10(*ctr, *key), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]


@pytest.mark.parametrize("seed", [0, 5, 2 ** 32 - 1, 2 ** 32, HIGH_SEED, 2 ** 64 - 1])
def test_stream_layout(seed):
    """Word idx = component idx & 3 of the block whose counter is (lo32, hi32 of idx >> 2, two constants), keyed (lo32, hi32 of seed)."""
    idx = np.array([0, 1, 2, 3, 4, 7, 2 ** 20 + 1, 2 ** 34 + 2, 2 ** 40 + 3], dtype=np.uint64)
    got = O.stream_words(seed, idx)
    for i, w in zip(idx.tolist(), got.tolist()):
        blk = i >> 2
        block = O.philox4x32_10(blk & 0xffffffff, blk >> 32, 0x9E3779B9, 0xBB67AE85, seed & 0xffffffff, seed >> 32)
        assert w == int(block[i & 3])
        assert int(O.stream_words(seed, i)) == w                         # a scalar call equals the vectorised call
    assert len(set(got.tolist())) == len(idx)


def test_keep_scale_arithmetic():
    """u = float32(word >> 8) * 2^-24, keep iff u >= float32(p), scale 1 / (1 - p) in float32."""
    idx = np.arange(4096, dtype=np.uint64)
    for p in (0.1, 0.25, 0.9):
        w = O.stream_words(5, idx)
        u = (w >> np.uint64(8)).astype(np.float64) / 2.0 ** 24            # exact: 24 bits
        k = O.keep_scale(5, idx, p)
        assert k.dtype == np.float32
        assert np.array_equal(k != 0, u >= float(np.float32(p)))
        assert set(np.unique(k).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert float(O.keep_scale(5, 3, 0.1)) == float(O.keep_scale(5, idx, 0.1)[3])


def test_effective_seed_wraps():
    assert O.effective_seed(5) == 5 and O.effective_seed(5, 0) == 5
    assert O.effective_seed(5, 1) == 0x9E3779B97F4A7C15 + 5
    assert O.effective_seed(2 ** 64 - 1, 2) == (2 * 0x9E3779B97F4A7C15 + 2 ** 64 - 1) % 2 ** 64
    assert O.effective_seed(7, 2 ** 63 + 1) == ((2 ** 63 + 1) * 0x9E3779B97F4A7C15 + 7) % 2 ** 64
    assert O.effective_seed(7, -(2 ** 63 - 1)) == O.effective_seed(7, 2 ** 63 + 1)       # the int64 a device tensor holds
    x = O.rnd(1000, seed=1)
    assert np.array_equal(O.dropout(x, 0.3, 7, 3), O.dropout(x, 0.3, O.effective_seed(7, 3)))
    assert not np.array_equal(O.dropout(x, 0.3, 7, 3), O.dropout(x, 0.3, 7, 4))
    assert np.array_equal(O.dropout(x, 0.0, 7), x)


N = 1 << 20
RATE_SEEDS = [5, 6, 777, 987654321, HIGH_SEED]


@pytest.fixture(scope="module")
def masks():
    idx = np.arange(2 * N, dtype=np.uint64)
    return {(s, p): O.keep_scale(s, idx, p) != 0 for s in RATE_SEEDS for p in (0.1, 0.3)}


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_keep_rate(masks, p):
    for s in RATE_SEEDS:
        rate = float(masks[(s, p)][:N].mean())
        print(f"seed {s}, p {p}: keep rate off by {abs(rate - (1 - p)):.2e}")
        assert abs(rate - (1 - p)) < 2e-3, (s, rate)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_streams_are_separate(masks, p):
    """Two independent masks agree with probability (1 - p)^2 + p^2: across seeds, and across index ranges of one seed."""
    want = (1 - p) ** 2 + p ** 2
    for a, b in itertools.combinations(RATE_SEEDS, 2):
        agree = float((masks[(a, p)][:N] == masks[(b, p)][:N]).mean())
        assert abs(agree - want) < 2e-3, (a, b, agree)
    for s in RATE_SEEDS:
        agree = float((masks[(s, p)][:N] == masks[(s, p)][N:]).mean())
        assert abs(agree - want) < 2e-3, (s, agree)


# ---- float64 references against torch float64 autograd, on the GPU tests' cases -----------------------------------------------------
def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _dev(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max()) if a.size else 0.0


def test_softmax_references_follow_torch():
    cases = [O.softmax_inputs(r, c) for r in O.SOFTMAX_ROWS for c in O.SOFTMAX_COLS]
    cases += [(row, O.rnd(*row.shape, seed=9)) for row in O.softmax_special_rows().values()]
    worst = 0.0
    for x, dp in cases:
        xr = _t(x).requires_grad_(True)
        pr = torch.softmax(xr, dim=-1)
        scale = O.keep_scale_like(x, 0.3, 777)
        pr.backward(_t(dp) * _t(scale))
        got = O.softmax_fwd(x)
        worst = max(worst, _dev(got, pr.detach().numpy()), _dev(O.softmax_bwd(dp, got, scale), xr.grad.numpy()))
    print(f"softmax references: {worst:.3g}")
    assert worst <= REF_BOUND
    masked = O.softmax_fwd(O.softmax_special_rows()["neg-inf"])
    assert (masked[0, ::3] == 0).all() and abs(masked.sum() - 1) < 1e-15


def test_batchnorm_references_follow_torch():
    worst = 0.0
    cases = [(r, c, False) for r in O.BN_ROWS for c in O.BN_COLS] + [O.BN_SHIFTED + (True,)]
    for (rows, cols, shifted), momentum in itertools.product(cases, O.BN_MOMENTA):
        x, gamma, beta, rm, rv, dy = O.batchnorm_inputs(rows, cols, shifted)
        for training in (True, False):
            xr, gr, br = (_t(v).requires_grad_(True) for v in (x, gamma, beta))
            trm, trv = _t(rm).clone(), _t(rv).clone()
            yr = F.batch_norm(xr, trm, trv, gr, br, training, momentum, 1e-5)
            yr.backward(_t(dy))
            y, sm, sr, nrm, nrv = O.batchnorm_fwd(x, gamma, beta, rm, rv, training, 1e-5, momentum)
            dx, dg, db = O.batchnorm_bwd(dy, x, gamma, sm, sr, training)
            worst = max(worst, _dev(y, yr.detach().numpy()), _dev(nrm, trm.numpy()), _dev(nrv, trv.numpy()),
                        _dev(dx, xr.grad.numpy()), _dev(dg, gr.grad.numpy()), _dev(db, br.grad.numpy()))
        # the ReLU gate: BatchNorm over relu(pre), differentiated to pre
        pre = _t(x).requires_grad_(True)
        gr = _t(gamma).requires_grad_(True)
        yr = F.batch_norm(torch.relu(pre), None, None, gr, _t(beta), True, momentum, 1e-5)
        yr.backward(_t(dy))
        xa = np.maximum(x, 0)
        _, sm, sr, _, _ = O.batchnorm_fwd(xa, gamma, beta, rm, rv, True, 1e-5, momentum)
        dx, dg, _ = O.batchnorm_bwd(dy, xa, gamma, sm, sr, True, relu_gate=True)
        worst = max(worst, _dev(dx, pre.grad.numpy()), _dev(dg, gr.grad.numpy()))
    print(f"batchnorm references: {worst:.3g}")
    assert worst <= REF_BOUND


def test_sharded_batchnorm_pieces_compose_to_batchnorm():
    """Moments without a centre, then about the global mean, summed over shards; bwd_apply with the global sums == BatchNorm."""
    worst = 0.0
    n = sum(O.SHARD_ROWS)
    for cols in O.SHARD_COLS:
        x, gamma, beta, rm, rv, dy = O.batchnorm_inputs(n, cols)
        cuts = np.cumsum((0,) + O.SHARD_ROWS)
        shards = [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        mean = sum(O.column_moments(x[s])[0] for s in shards) / n
        var = sum(O.column_moments(x[s], mean)[1] for s in shards) / n
        rstd = 1.0 / np.sqrt(var + 1e-5)
        y, sm, sr, _, _ = O.batchnorm_fwd(x, gamma, beta, rm, rv, True)
        dx, dg, db = O.batchnorm_bwd(dy, x, gamma, sm, sr, True)
        worst = max(worst, _dev(mean, sm), _dev(rstd, sr))
        got = np.concatenate([O.batchnorm_bwd_apply(dy[s], x[s], gamma, mean, rstd, db, dg, n) for s in shards])
        worst = max(worst, _dev(got, dx))
    assert worst <= REF_BOUND


def test_mse_and_bias_act_references_follow_torch():
    worst = 0.0
    for n, gs in itertools.product(O.MSE_NS, O.MSE_SCALES):
        pred, tgt = O.rnd(n, seed=n), O.rnd(n, seed=n + 1)
        pr = _t(pred).requires_grad_(True)
        lr = F.mse_loss(pr, _t(tgt))
        (lr * gs).backward()
        loss, dpred = O.mse(pred, tgt, gs)
        worst = max(worst, _dev(loss, lr.item()), _dev(dpred, pr.grad.numpy()))
    for rows, cols, scale in itertools.product(O.BIAS_ACT_ROWS, O.BIAS_ACT_COLS, O.BIAS_ACT_SCALES):
        pre, dy = O.rnd(rows, cols, seed=rows + cols), O.rnd(rows, cols, seed=rows + cols + 1)
        for act, fn in ((1, torch.relu), (2, torch.tanh)):
            pr = _t(pre).requires_grad_(True)
            y = fn(pr)
            y.backward(_t(dy) * scale)
            d, db = O.bias_act_bwd(dy, y.detach().numpy(), act, scale)
            worst = max(worst, _dev(d, pr.grad.numpy()), _dev(db, pr.grad.sum(0).numpy()))
        d, db = O.bias_act_bwd(dy, None, 0, scale)
        assert np.array_equal(d, dy.astype(np.float64)) and _dev(db, dy.astype(np.float64).sum(0)) <= REF_BOUND
    print(f"mse / bias_act references: {worst:.3g}")
    assert worst <= REF_BOUND


def test_fusion_reference_follows_torch():
    worst = 0.0
    for nh, hd, dim, rows in itertools.product(O.FUSION_HEADS, O.FUSION_HIDDEN, O.FUSION_DIMS, O.FUSION_ROWS):
        comb, hid, w2, b2, _ = O.fusion_inputs(nh, hd, dim, rows)
        logits = torch.stack([_t(hid[h]) @ _t(w2[h]) + float(b2[h]) for h in range(nh)], dim=1)
        attn = torch.softmax(logits, dim=1)
        out = sum(attn[:, h:h + 1] * _t(comb) for h in range(nh))
        lg, at, ou = O.fusion_combine_fwd(comb, hid, w2, b2)
        worst = max(worst, _dev(lg, logits.numpy()), _dev(at, attn.numpy()), _dev(ou, out.numpy()))
    assert worst <= REF_BOUND


# ---- what float32 gives: the restatements against float64, at the tolerances the GPU tests apply ------------------------------------
def _ratio(a, ref, rtol, atol_frac):
    """Worst error of ``a`` as a multiple of helpers.assert_close's tolerance."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = rtol * np.abs(ref) + atol_frac * np.abs(ref).max() + 1e-30
    return float((np.abs(a - ref) / tol).max())


def test_float32_restatements_are_the_kernels_arithmetic():
    """The restatements are float32 throughout and agree with float64 to float32 rounding on a well-conditioned case; the figures the
    GPU file quotes as S come from report_float32_deviations below."""
    x, dp = O.softmax_inputs(5, 167)
    p32 = O.softmax_fwd32(x)
    assert p32.dtype == np.float32 and _ratio(p32, O.softmax_fwd(x), 1e-5, 1e-5) < 1
    x, gamma, beta, rm, rv, dy = O.batchnorm_inputs(33, 65)
    for training in (True, False):
        got = O.batchnorm_fwd32(x, gamma, beta, rm, rv, training)
        want = O.batchnorm_fwd(x, gamma, beta, rm, rv, training)
        assert all(g.dtype == np.float32 for g in got)
        assert max(_ratio(g, w, 1e-5, 1e-5) for g, w in zip(got, want)) < 1
        bwd = O.batchnorm_bwd32(dy, x, gamma, got[1], got[2], training)
        assert max(_ratio(g, w, 1e-4, 2e-5) for g, w in zip(bwd, O.batchnorm_bwd(dy, x, gamma, want[1], want[2], training))) < 1


def report_float32_deviations():
    """Worst error / tolerance of the float32 restatements over the GPU case lists (run: python tests/test_rowops_cpu.py)."""
    rows = []
    for r, c in itertools.product(O.SOFTMAX_ROWS, O.SOFTMAX_COLS):
        x, _ = O.softmax_inputs(r, c)
        rows.append((f"softmax {r}x{c}", _ratio(O.softmax_fwd32(x), O.softmax_fwd(x), 1e-5, 1e-5), O.deviation(O.softmax_fwd32(x), O.softmax_fwd(x))))
    for name, x in O.softmax_special_rows().items():
        rows.append((f"softmax {name}", _ratio(O.softmax_fwd32(x), O.softmax_fwd(x), 1e-5, 1e-5), O.deviation(O.softmax_fwd32(x), O.softmax_fwd(x))))
    for (r, c, sh) in [(r, c, False) for r in O.BN_ROWS for c in O.BN_COLS] + [O.BN_SHIFTED + (True,)]:
        x, gamma, beta, rm, rv, dy = O.batchnorm_inputs(r, c, sh)
        got, want = O.batchnorm_fwd32(x, gamma, beta, rm, rv, True), O.batchnorm_fwd(x, gamma, beta, rm, rv, True)
        for nm, g, w in zip(("y", "mean", "rstd", "rm", "rv"), got, want):
            rows.append((f"bn {r}x{c}{' shifted' if sh else ''} {nm}", _ratio(g, w, 1e-5, 1e-5), O.deviation(g, w)))
        bwd, bw = O.batchnorm_bwd32(dy, x, gamma, got[1], got[2], True), O.batchnorm_bwd(dy, x, gamma, want[1], want[2], True)
        for nm, g, w in zip(("dx", "dgamma", "dbeta"), bwd, bw):
            rows.append((f"bn {r}x{c}{' shifted' if sh else ''} {nm}", _ratio(g, w, 1e-4, 2e-5), O.deviation(g, w)))
    for name, ratio, s in rows:
        if ratio > 0.25:
            print(f"{name}: {ratio:.2f} x tolerance, S = {s:.3e}")
    print(f"{len(rows)} figures, worst {max(r[1] for r in rows):.2f} x tolerance")


if __name__ == "__main__":
    report_float32_deviations()
