"""GPU: random_forest.RandomForestRegressor / DecisionTreeRegressor.  A regression fit has no summation order (exact int64 sums of the
rounded targets, seven float64 roundings per score), so the GPU's trees are compared bit for bit with the numpy restatement
(tests/rfr_numpy.py), which tests/test_rfr_cpu.py ties to scikit-learn's trees; prediction is compared bit for bit with scikit-learn's;
quality is measured against scikit-learn's own scatter over random_state."""
import numpy as np
import pytest
import torch

import rfr_numpy as Q
import rfr_replay as R
from poison import FILLS, poisoned_allocations
from test_rfr_cpu import problem, rounded

pytestmark = pytest.mark.gpu


def RFR(*a, **kw):
    from bbbp_amd.random_forest import RandomForestRegressor
    return RandomForestRegressor(*a, **kw)


def DTR(**kw):
    from bbbp_amd.random_forest import DecisionTreeRegressor
    return DecisionTreeRegressor(**kw)


def _same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


def _case_data(n, d, variant):
    if variant == "collide":                              # repeated feature values and repeated targets: ties in both
        X, y = problem(n, d)
        return np.round(X, 1), np.round(y, 1)
    return problem(n, d, 1000.0 if variant == "+1000" else 0.0)


# n, d, variant, trees, parameters.  65: one wave and one row; 257 / 513 / 2049: one row more than 1, 2 and 8 passes of 256 positions;
# 6000: the split kernel's 12 n bytes of LDS pass 64 KB; "+1000": node sums near 2^57, where the int64 -> float64 conversions round
CASES = [(65, 3, None, 5, dict()),
         (257, 5, None, 4, dict(max_features="sqrt", min_samples_leaf=3)),
         (513, 12, None, 1, dict(bootstrap=False)),
         (2049, 7, None, 3, dict(max_depth=8)),
         (65, 3, "collide", 5, dict()), (257, 5, "collide", 4, dict(max_features="sqrt", min_samples_leaf=3)),
         (65, 3, "+1000", 5, dict()), (257, 5, "+1000", 4, dict(max_features="sqrt", min_samples_leaf=3)), (2049, 7, "+1000", 3, dict(max_depth=8)),
         (6000, 4, None, 1, dict(max_depth=3))]


@pytest.mark.parametrize("n,d,variant,T,kw", CASES)
def test_trees_equal_the_restatement(dev, n, d, variant, T, kw):
    X, y = _case_data(n, d, variant)
    reg = RFR(T, random_state=9, device=dev, **kw).fit(X, y)
    want = Q.fit_forest(X, y, T, seed=9, with_weights=True, **kw)
    weight = want.pop("weighted_n_node_samples")
    assert reg.n_estimators_ == T and reg.n_features_in_ == d and reg.y_quantum_ == rounded(y)[1]
    for k in want:
        assert reg.trees_[k].dtype == want[k].dtype and np.array_equal(reg.trees_[k], want[k]), k
    assert _same(reg.trees_, want)
    assert reg.weighted_n_node_samples_.dtype == np.float64 and np.array_equal(reg.weighted_n_node_samples_, weight)       # the value0 slot
    if variant == "+1000":
        assert np.abs(Q.quantise(y)[0]).sum() > 2 ** 53
    if n <= 257:
        seen = R.replay(X, rounded(y)[0], reg.trees_, seed=9, own=True, quantum=reg.y_quantum_, **kw)
        print(n, d, variant, kw, seen)
        if variant == "collide" and "min_samples_leaf" not in kw:                 # under min_samples_leaf = 3 that rule ends the nodes first
            assert seen["stop_reasons"].get("pure", 0) >= 1
    p = reg.predict(X[:300])
    assert p.dtype == np.float64 and p.shape == (min(n, 300),) and np.array_equal(p, Q.predict(want, X[:300]))


def test_depth_beyond_a_block_of_rounds(dev):
    """24 rows on one feature with y_i = 2^i: every split peels off the largest target, 14 levels (scikit-learn's tree on this data has the
    same depth): more levels than one block of eight rounds."""
    X, y = np.arange(24.0)[:, None], 2.0 ** np.arange(24)
    reg = DTR(device=dev).fit(X, y)
    want = Q.fit_forest(X, y, 1, bootstrap=False)
    assert _same(reg.trees_, want)
    seen = R.replay(X, y, reg.trees_, seed=0, own=True, quantum=reg.y_quantum_, bootstrap=False)
    assert seen["max_depth"] == 14 and seen["nodes"] == 47
    assert np.array_equal(reg.predict(X), y)


def test_tie_rule_lowest_feature_wins(dev):
    """Column 3 is a copy of column 1: every score of one is a score of the other, bit for bit, and no split may name column 3."""
    X, y = problem(257, 5)
    X = X.copy()
    X[:, 3] = X[:, 1]
    reg = RFR(6, random_state=2, device=dev).fit(X, y)
    split = reg.trees_["left"] >= 0
    assert (reg.trees_["feature"][split] == 1).any() and not (reg.trees_["feature"][split] == 3).any()
    assert _same(reg.trees_, Q.fit_forest(X, y, 6, seed=2))


# ---- determinism --------------------------------------------------------------------------------------------------------------------------
def _batch(dev, X, y, param_list):
    """Grow the regression forests of ``param_list`` (n_trees, max_depth, min_samples_split, min_samples_leaf, max_features, bootstrap, seed)
    over one matrix in one batch: per forest its flat trees, values in grid units."""
    from bbbp_amd import random_forest as F
    from bbbp_amd._tree_host import Matrix as _Matrix
    mat = _Matrix(np.ascontiguousarray(X, dtype=np.float32), dev)
    q, _ = F._quantise(y, len(y), "test")
    t_d = torch.from_numpy(q).to(dev)
    specs = [F._Spec(mat, t_d, *p, regression=True) for p in param_list]
    F._grow(specs)
    return [s.trees for s in specs]


def test_determinism_alone_in_a_batch_reversed_and_again(dev):
    from bbbp_amd.random_forest import fit_regressors
    X, y = problem(257, 5)
    mine = (3, None, 2, 1, 2, True, 4)
    others = [(2, 3, 5, 1, 5, False, 4), (4, None, 2, 3, 1, True, 7), (3, None, 2, 1, 2, True, 5), (1, 1, 10, 1, 2, True, 4)]
    alone = _batch(dev, X, y, [mine])[0]
    batch = _batch(dev, X, y, others[:2] + [mine] + others[2:])
    backwards = _batch(dev, X, y, (others[:2] + [mine] + others[2:])[::-1])
    again = _batch(dev, X, y, [mine])[0]
    for name, got in (("in a batch", batch[2]), ("in the reversed batch", backwards[2]), ("a second run", again)):
        assert _same(alone, got), name
    assert all(_same(a, b) for a, b in zip(batch, backwards[::-1]))
    assert not _same(alone, batch[3])                                               # another seed, another forest
    # fit_regressors: problems of different shapes and scales in one batch; each equals its single fit
    problems = [(X, y), problem(65, 3), (X[:200], y[:200] + 1000.0), problem(513, 12)]
    kw = dict(n_estimators=3, max_depth=6, max_features=2, random_state=4, device=dev)
    together = fit_regressors(problems, **kw)
    for (Xp, yp), got in zip(problems, together):
        single = RFR(**kw).fit(Xp, yp)
        assert _same(got.trees_, single.trees_) and got.y_quantum_ == single.y_quantum_
        assert np.array_equal(got.weighted_n_node_samples_, single.weighted_n_node_samples_)
        assert np.array_equal(got.predict(Xp), single.predict(Xp))
    assert together[0].y_quantum_ != together[2].y_quantum_


# ---- prediction -----------------------------------------------------------------------------------------------------------------------------
def _threshold_queries(sk, X):
    """Training rows, and for every split node one row with that feature exactly on the threshold's float32 value, one float32 below and
    one above."""
    rs = np.random.RandomState(0)
    rows = [X.astype(np.float32)]
    for est in (sk.estimators_ if hasattr(sk, "estimators_") else [sk]):
        t = est.tree_
        for f, thr in zip(t.feature[t.feature >= 0], t.threshold[t.feature >= 0]):
            at = np.float32(thr)
            q = np.repeat(X[rs.randint(len(X))][None, :].astype(np.float32), 3, axis=0)
            q[:, f] = [np.nextafter(at, np.float32(-np.inf)), at, np.nextafter(at, np.float32(np.inf))]
            rows.append(q)
    return np.concatenate(rows)


@pytest.mark.parametrize("kind,kw", [("forest", dict()), ("forest", dict(max_depth=3, max_features="sqrt")), ("extra", dict(min_samples_leaf=3)),
                                     ("tree", dict()), ("tree", dict(max_depth=2))])
def test_adopted_models_predict_as_sklearn(dev, kind, kw):
    from sklearn.ensemble import ExtraTreesRegressor, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    from bbbp_amd import random_forest as F
    X, y = problem(257, 5)
    if kind == "tree":
        sk = DecisionTreeRegressor(random_state=0, **kw).fit(X, y)
    else:
        sk = (RandomForestRegressor if kind == "forest" else ExtraTreesRegressor)(n_estimators=10, random_state=0, **kw).fit(X, y)
    reg = (F.DecisionTreeRegressor if kind == "tree" else F.RandomForestRegressor).from_sklearn(sk, dev)
    Xq = _threshold_queries(sk, X)
    assert np.array_equal(reg.predict(Xq), sk.predict(Xq))
    on_device = reg.predict(torch.from_numpy(Xq).to(dev))
    assert on_device.is_cuda and on_device.dtype == torch.float64 and np.array_equal(on_device.cpu().numpy(), sk.predict(Xq))
    assert reg.n_estimators_ == (1 if kind == "tree" else 10) and np.array_equal(reg.trees_["value"], R.trees_of_sklearn(sk)["value"])


def test_limits_view_equals_the_pruned_model(dev):
    """The forest grown with (8 trees, no depth limit, min_samples_split 2), seen through the predict kernel's limits, is the single fit
    under those limits bit for bit: the materialised trees and the predictions."""
    X, y = problem(257, 5)
    big = RFR(8, max_features="sqrt", random_state=1, device=dev).fit(X, y)
    from bbbp_amd import random_forest as F
    X32, q, s, mf = big._checked(X, y)
    spec = big._spec(X32, q, mf)
    F._grow([spec])
    assert big.y_quantum_ == 2.0 ** -s
    Xq, _ = big._queries(X[:64])
    for T in (3, 8):
        for depth in (4, None):
            for mss in (2, 20):
                kw = dict(max_depth=depth, min_samples_split=mss, max_features="sqrt", random_state=1, device=dev)
                single = RFR(T, **kw).fit(X, y)
                view = RFR(T, **kw)
                view._adopt(spec, s, (T, depth, mss))
                assert _same(view.trees_, single.trees_), (T, depth, mss)
                want = single.predict(X[:64])
                assert np.array_equal(view.predict(X[:64]), want), (T, depth, mss)
                assert np.array_equal(big._mean(Xq, (T, depth, mss)).cpu().numpy(), want), (T, depth, mss)
                assert np.array_equal(want, Q.predict(big.trees_, X[:64], (T, depth, mss))), (T, depth, mss)


def test_stacking_regressor_takes_the_regressor_as_a_base_learner(dev):
    from sklearn.linear_model import Ridge
    from bbbp_amd.ensemble import StackingRegressor
    rs = np.random.default_rng(3)
    X = rs.standard_normal((60, 4))
    y = X @ np.array([0.5, 0.3, 0.1, 0.1]) + 0.05 * rs.standard_normal(60)
    stack = StackingRegressor([("rf", RFR(20, max_depth=15, random_state=42, device=dev)), ("ridge", Ridge(1.0))]).fit(X, y)
    fitted = dict(stack.estimators_)["rf"]
    assert type(fitted).__name__ == "RandomForestRegressor" and fitted.n_estimators_ == 20
    p = stack.predict(X)
    assert p.shape == (60,) and np.isfinite(p).all() and np.mean((p - y) ** 2) < np.var(y)
    assert np.array_equal(fitted.predict(X), RFR(20, max_depth=15, random_state=42, device=dev).fit(X, y).predict(X))


# ---- quality against scikit-learn's own scatter -----------------------------------------------------------------------------------------
def test_quality_within_sklearn_scatter(dev):
    """make_friedman1(600, 10, noise=1), 400 rows to fit and 200 to score, 50 trees of depth 15: the test MSE of each of our seeds 0..4 lies
    inside [min - 3 sigma, max + 3 sigma] of scikit-learn's seeds 0..9 -- three of scikit-learn's own seed-to-seed standard deviations, since our
    bootstrap is another stream of the same distribution.  Measured on one MI355X: ours 4.1085, 4.1612, 4.1842, 4.1926, 4.1037 (the numpy
    restatement gives the same on the CPU); scikit-learn mean 4.0355, sigma 0.1862, range [3.7345, 4.2862]."""
    from sklearn.datasets import make_friedman1
    from sklearn.ensemble import RandomForestRegressor
    from bbbp_amd.random_forest import fit_regressors
    X, y = make_friedman1(600, 10, noise=1, random_state=0)
    Xa, ya, Xb, yb = X[:400], y[:400], X[400:], y[400:]
    sk = [float(np.mean((RandomForestRegressor(50, max_depth=15, random_state=rs).fit(Xa, ya).predict(Xb) - yb) ** 2)) for rs in range(10)]
    sigma = float(np.std(sk, ddof=1))
    ours = [float(np.mean((RFR(50, max_depth=15, random_state=seed, device=dev).fit(Xa, ya).predict(Xb) - yb) ** 2)) for seed in range(5)]
    print(f"test MSE: ours {[round(v, 4) for v in ours]}, scikit-learn mean {np.mean(sk):.4f} sigma {sigma:.4f} [{min(sk):.4f}, {max(sk):.4f}]")
    assert sigma > 0
    for seed, mse in enumerate(ours):
        assert min(sk) - 3 * sigma <= mse <= max(sk) + 3 * sigma, (seed, mse)


# ---- poisoned memory ------------------------------------------------------------------------------------------------------------------------
def test_fit_and_predict_under_poison(dev, monkeypatch):
    """Outputs, the work area and the node slots come out of pools filled with 0x00, 0xFF and 0x7B: nothing may depend on what an
    allocation held, and no guard band may be written (tests/poison.py)."""
    X, y = problem(257, 5)
    results = {}
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            reg = RFR(5, min_samples_leaf=2, max_features=3, random_state=3, device=dev).fit(X, y)
            pred = reg.predict(X[:100])
            limited = reg._mean(reg._queries(X[:33])[0], (3, 4, 10)).cpu().numpy()
            torch.cuda.synchronize()
        assert pa.check() >= 10, "the forest's allocations did not go through the pools"
        pa.release()
        results[fill] = (reg.trees_, pred, limited, reg.weighted_n_node_samples_)
    first = results[FILLS[0]]
    for fill in FILLS[1:]:
        got = results[fill]
        assert _same(first[0], got[0]) and all(np.array_equal(a, b) for a, b in zip(first[1:], got[1:])), hex(fill)
    assert np.isfinite(first[1]).all() and np.isfinite(first[2]).all()
    assert _same(first[0], Q.fit_forest(X, y, 5, seed=3, min_samples_leaf=2, max_features=3))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu_box(dev):
    from bbbp_amd.random_forest import MAX_FEATURES, MAX_ROWS
    with pytest.raises(ValueError, match="BBBP_RF_FIT_MAX_N"):
        RFR(device=dev).fit(torch.zeros(MAX_ROWS + 1, 2, device=dev), np.zeros(MAX_ROWS + 1))
    with pytest.raises(ValueError, match="BBBP_RF_FIT_MAX_D"):
        RFR(device=dev).fit(torch.zeros(4, MAX_FEATURES + 1, device=dev), np.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RFR(device=dev).fit(torch.zeros(4, 2), np.zeros(4))
    reg = DTR(device=dev).fit(torch.arange(8.0, device=dev).reshape(4, 2), torch.tensor([1.0, 1.0, 3.0, 5.0]))
    with pytest.raises(ValueError, match="queries"):
        reg.predict(np.zeros((3, 5)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.predict(torch.zeros(3, 2))
    assert list(reg.predict(np.array([[0.0, 1.0], [4.0, 5.0], [6.0, 7.0]]))) == [1.0, 3.0, 5.0] and reg.predict(np.zeros((0, 2))).shape == (0,)
    assert reg.n_estimators_ == 1 and len(reg.trees_["left"]) == 5 and list(reg.trees_["value"][:1]) == [2.5]
    flat = DTR(device=dev).fit(np.arange(8.0).reshape(4, 2), np.zeros(4))             # all targets 0: the grid's step is 1, the root is pure
    assert flat.y_quantum_ == 1.0 and len(flat.trees_["left"]) == 1 and list(flat.predict(np.zeros((2, 2)))) == [0.0, 0.0]
