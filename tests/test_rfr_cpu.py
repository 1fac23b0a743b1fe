"""CPU: the numpy restatement of random_forest's regression fit (tests/rfr_numpy.py) against scikit-learn's trees, its certifier
(tests/rfr_replay.py) on scikit-learn's models and on the restatement's, the planted faults it must name, and what the regressors refuse
without a GPU."""
import functools

import numpy as np
import pytest

import rf_numpy as N
import rfr_numpy as Q
import rfr_replay as R

U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def problem(n, d, shift=0.0):
    """X standard normal float32, y = sin(2 x0) + x1 x2 + 0.1 noise (+ shift), from default_rng(1000 n + d); read-only."""
    rs = np.random.default_rng(1000 * n + d)
    X = rs.standard_normal((n, d)).astype(np.float32)
    y = np.sin(2 * X[:, 0].astype(np.float64)) + X[:, 1].astype(np.float64) * X[:, 2] + 0.1 * rs.standard_normal(n) + shift
    X.setflags(write=False); y.setflags(write=False)
    return X, y


def rounded(y):
    q, s = Q.quantise(y)
    return Q.dequantise(q, s), float(np.ldexp(1.0, -s))


def _copy(trees):
    return {k: v.copy() for k, v in trees.items()}


# ---- the targets' grid -----------------------------------------------------------------------------------------------------------------
def test_quantise():
    _, y = problem(257, 5)
    q, s = Q.quantise(y)
    e = int(np.frexp(np.abs(y).max())[1])
    assert s == 49 - e and np.abs(q).max() <= 2 ** 49 and np.abs(Q.dequantise(q, s) - y).max() <= 2.0 ** (e - 50)
    assert np.abs(Q.dequantise(q, s) - y).max() <= 7.2e-15                        # |y| < 8
    assert Q.quantise(np.zeros(4))[1] == 0 and not Q.quantise(np.zeros(4))[0].any()
    q2, s2 = Q.quantise(np.array([1.0, -0.75, 2.0 ** -60]))
    assert s2 == 48 and list(q2) == [2 ** 48, -3 * 2 ** 46, 0]
    big, sb = Q.quantise(np.array([3.0e300, -1.0e300]))
    assert np.abs(big).max() <= 2 ** 49 and sb < 0
    from bbbp_amd.random_forest import TARGET_BITS, _quantise
    qf, sf = _quantise(y, len(y), "test")
    assert TARGET_BITS == Q.TARGET_BITS and sf == s and qf.dtype == np.float64 and np.array_equal(qf, q.astype(np.float64))


# ---- the restatement is scikit-learn's tree on the rounded targets ----------------------------------------------------------------------
def _walk_equal(X, mine, sk, y_hat, w):
    """Node for node along a parallel walk (scikit-learn numbers depth first): the same feature, the same threshold bits, the same
    n_node_samples, values within (m + 2) U mean |y_hat| of the node.  Returns the number of nodes compared."""
    pairs, count = [(0, 0, np.nonzero(w > 0)[0])], 0
    while pairs:
        a, b, rows = pairs.pop()
        count += 1
        assert (mine["left"][a] < 0) == (sk.children_left[b] < 0), (a, b)
        assert mine["n_node_samples"][a] == sk.n_node_samples[b] == len(rows), (a, b)
        m = len(rows)
        bound = (m + 2) * U * np.abs(y_hat[rows]).mean()
        assert abs(mine["value"][a] - sk.value[b, 0, 0]) <= bound, (a, b, mine["value"][a], sk.value[b, 0, 0], bound)
        if mine["left"][a] >= 0:
            assert mine["feature"][a] == sk.feature[b], (a, b)
            assert np.float64(mine["threshold"][a]).tobytes() == np.float64(sk.threshold[b]).tobytes(), (a, b)
            go = X[rows, sk.feature[b]].astype(np.float64) <= sk.threshold[b]
            pairs.append((int(mine["left"][a]), int(sk.children_left[b]), rows[go]))
            pairs.append((int(mine["right"][a]), int(sk.children_right[b]), rows[~go]))
    return count


def _sklearn_trees(X, y, y_hat, depth, weight=None):
    """scikit-learn's tree for random_state 0..9 on y_hat and once on y; the precondition is that they are one tree (the problem has no ties
    for scikit-learn's random feature order to break, and rounding the targets moves no split)."""
    from sklearn.tree import DecisionTreeRegressor
    fits = [DecisionTreeRegressor(max_depth=depth, min_samples_leaf=5, random_state=rs).fit(X, y_hat, sample_weight=weight).tree_ for rs in range(10)]
    fits.append(DecisionTreeRegressor(max_depth=depth, min_samples_leaf=5, random_state=0).fit(X, y, sample_weight=weight).tree_)
    first = fits[0]
    for other in fits[1:]:
        same = (first.node_count == other.node_count and np.array_equal(first.feature, other.feature) and np.array_equal(first.threshold, other.threshold)
                and np.array_equal(first.n_node_samples, other.n_node_samples))
        assert same, "fixture error: scikit-learn's own trees on this problem differ over random_state or between y and its rounding"
    return first


@pytest.mark.parametrize("n,d,depth,shift", [(257, 5, 5, 0.0), (513, 12, 6, 0.0), (2049, 7, 8, 0.0), (257, 5, 5, 1000.0), (513, 12, 6, 1000.0)])
def test_restatement_equals_sklearn(n, d, depth, shift):
    """shift 1000: the node sums reach 2^57 in grid units, so the int64 -> float64 conversions of the score round."""
    X, y = problem(n, d, shift)
    y_hat, _ = rounded(y)
    sk = _sklearn_trees(X, y, y_hat, depth)
    mine = Q.fit_forest(X, y, 1, max_depth=depth, min_samples_leaf=5, bootstrap=False)
    if shift:
        assert np.abs(Q.quantise(y)[0]).sum() > 2 ** 53
    assert _walk_equal(X, mine, sk, y_hat, np.ones(n, dtype=np.int64)) == sk.node_count == len(mine["left"]) and sk.node_count > 15


@pytest.mark.parametrize("t", [0, 1, 2])
def test_restatement_equals_sklearn_under_bootstrap_weights(t):
    n, d, depth = 513, 12, 6
    X, y = problem(n, d)
    y_hat, _ = rounded(y)
    w = N.bootstrap_weights(5, t, n)
    sk = _sklearn_trees(X, y, y_hat, depth, weight=w.astype(np.float64))
    mine = Q.fit_forest(X, y, 1, max_depth=depth, min_samples_leaf=5, weights=[w], with_weights=True)
    assert _walk_equal(X, mine, sk, y_hat, w) == sk.node_count == len(mine["left"])
    assert mine["weighted_n_node_samples"][0] == n and sorted(mine["weighted_n_node_samples"]) == sorted(sk.weighted_n_node_samples)


# ---- the certifier on scikit-learn's models -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(min_samples_leaf=3, min_samples_split=8), dict(max_depth=4)])
def test_replayer_accepts_sklearn_trees(kw):
    """Full depth with min_samples_leaf = 1 included: ties abound there, and the certifier does not depend on how they were broken."""
    from sklearn.tree import DecisionTreeRegressor
    X, y = problem(257, 5)
    X = X.copy()
    X[:, 3] = np.round(X[:, 3], 1)                                               # heavy value ties
    for rs in range(2):
        sk = DecisionTreeRegressor(random_state=rs, **kw).fit(X, y)
        seen = R.replay(X, y, R.trees_of_sklearn(sk), **kw)
        assert seen["nodes"] == sk.tree_.node_count and seen["splits"] >= 5


def test_replayer_accepts_a_sklearn_forest():
    from sklearn.ensemble import RandomForestRegressor
    X, y = problem(257, 5)
    sk = RandomForestRegressor(n_estimators=3, random_state=0).fit(X, y)
    seen = R.replay(X, y, R.trees_of_sklearn(sk), weights=R.bootstrap_weights_of_sklearn(sk, len(y)))
    assert seen["nodes"] == sum(e.tree_.node_count for e in sk.estimators_) and seen["stop_reasons"].get("min_samples_split", 0) > 100
    shifted = RandomForestRegressor(n_estimators=2, random_state=1, min_samples_leaf=2).fit(X, y + 1000.0)
    R.replay(X, y + 1000.0, R.trees_of_sklearn(shifted), weights=R.bootstrap_weights_of_sklearn(shifted, len(y)), min_samples_leaf=2)


# ---- the certifier on the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 1000.0])
@pytest.mark.parametrize("kw", [dict(), dict(max_depth=4), dict(min_samples_split=10, min_samples_leaf=3), dict(max_features="sqrt"),
                                dict(max_features=3, min_samples_leaf=2, bootstrap=False)])
def test_replayer_accepts_the_restatement(kw, shift):
    X, y = problem(257, 5, shift)
    y_hat, quantum = rounded(y)
    trees = Q.fit_forest(X, y, 2, seed=5, **kw)
    seen = R.replay(X, y_hat, trees, seed=5, own=True, quantum=quantum, **kw)
    assert seen["splits"] >= 6 and len(trees["root"]) == 3
    if "max_depth" in kw:
        assert seen["max_depth"] == 4 and seen["stop_reasons"].get("depth", 0) > 0


def test_pure_nodes_and_level_order():
    """Repeated targets: a node whose targets are one grid point is a leaf although a feature could still split it."""
    X, _ = problem(257, 5)
    y = np.round(X[:, 0].astype(np.float64))
    trees = Q.fit_forest(X, y, 2, seed=1)
    seen = R.replay(X, rounded(y)[0], trees, seed=1, own=True, quantum=rounded(y)[1])
    assert seen["stop_reasons"].get("pure", 0) > 0
    for t in range(2):
        lo, hi = trees["root"][t], trees["root"][t + 1]
        kids = np.stack([trees["left"][lo:hi], trees["right"][lo:hi]], axis=1)
        assert np.array_equal(kids[kids[:, 0] >= 0].ravel(), np.arange(lo + 1, hi))


def _root_candidates(X, q, w, msl):
    """Per feature the root's valid positions, their float64 scores and the sorted float32 values."""
    rows = np.nonzero(w > 0)[0]
    out = {}
    for f in range(X.shape[1]):
        o = np.argsort(X[rows, f], kind="stable")
        p, WL, SL = Q.position_sums(X[rows, f][o], w[rows][o], (w * q)[rows][o], msl)
        out[f] = (p, Q.scores(WL, SL, int(w.sum()), int((w * q).sum())), X[rows, f][o])
    return out


def _expect(check, X, y, trees, **kw):
    with pytest.raises(R.ReplayError) as e:
        R.replay(X, y, trees, **kw)
    assert e.value.check == check, str(e.value)


def test_replayer_rejects_planted_faults():
    X, y = problem(257, 5)
    y_hat, quantum = rounded(y)
    kw = dict(seed=7, own=True, quantum=quantum, min_samples_leaf=3, bootstrap=True)
    good = Q.fit_forest(X, y, 1, seed=7, min_samples_leaf=3)
    R.replay(X, y_hat, good, **kw)
    w = N.bootstrap_weights(7, 0, len(y))
    cands = _root_candidates(X, Q.quantise(y)[0], w, 3)
    f0 = int(good["feature"][0])
    # a suboptimal feature: the best position of another feature, whose score is clearly lower
    other = min((f for f in cands if f != f0 and cands[f][1].max() < cands[f0][1].max() * (1 - 1e-6)), key=lambda f: -cands[f][1].max())
    p, score, fv = cands[other]
    j = int(np.argmax(score))
    bad = _copy(good)
    bad["feature"][0], bad["threshold"][0] = other, N.midpoint(fv[p[j] - 1], fv[p[j]])
    _expect("optimal", X, y_hat, bad, **kw)
    # a shifted threshold: off by one float32
    bad = _copy(good)
    bad["threshold"][0] = np.float64(np.nextafter(np.float32(good["threshold"][0]), np.float32(np.inf))) + 0.0
    assert bad["threshold"][0] != good["threshold"][0]
    _expect("valid", X, y_hat, bad, **kw)
    # a wrong value: one unit in the last place
    bad = _copy(good)
    bad["value"][0] = np.nextafter(bad["value"][0], 2.0)
    _expect("samples", X, y_hat, bad, **kw)
    # a wrong count
    bad = _copy(good)
    bad["n_node_samples"][1] += 1
    _expect("samples", X, y_hat, bad, **kw)
    # a forbidden leaf
    bad = _copy(good)
    bad["left"][0] = bad["right"][0] = -1
    _expect("stop", X, y_hat, bad, **kw)


def test_replayer_rejects_a_tie_taken_against_the_rule():
    """Column 4 is a copy of column 0: every score of one is a score of the other, bit for bit.  Naming the copy is optimal, not the rule's."""
    X, y = problem(257, 5)
    X = X.copy()
    X[:, 4] = X[:, 0]
    y_hat, quantum = rounded(y)
    kw = dict(seed=3, own=True, quantum=quantum, bootstrap=False)
    good = Q.fit_forest(X, y, 1, seed=3, bootstrap=False)
    seen = R.replay(X, y_hat, good, **kw)
    split = good["left"] >= 0
    assert seen["ties"] >= 1 and (good["feature"][split] == 0).any() and not (good["feature"][split] == 4).any()
    bad = _copy(good)
    bad["feature"][np.nonzero(split & (good["feature"] == 0))[0][0]] = 4
    _expect("tie", X, y_hat, bad, **kw)
    R.replay(X, y_hat, bad, **{**kw, "own": False, "quantum": None})           # as some other implementation's tree it is a correct one


# ---- structure ------------------------------------------------------------------------------------------------------------------------------------
def test_pruning_and_prefix_property_of_the_restatement():
    from bbbp_amd.random_forest import _prune
    X, y = problem(257, 5)
    big = Q.fit_forest(X, y, 5, seed=2, with_weights=True)
    big["value0"] = big.pop("weighted_n_node_samples")
    cut = _prune(big, 5, 4, 20)
    single = Q.fit_forest(X, y, 5, seed=2, max_depth=4, min_samples_split=20)
    assert all(np.array_equal(cut[k], single[k]) for k in single) and len(single["left"]) < len(big["left"])
    three = Q.fit_forest(X, y, 3, seed=2)
    end = three["root"][-1]
    assert np.array_equal(three["root"], big["root"][:4]) and all(np.array_equal(three[k], big[k][:end]) for k in three if k != "root")
    limited = Q.predict(big, X[:50], (3, 4, 20))
    assert np.array_equal(limited, Q.predict(_prune(big, 3, 4, 20), X[:50])) and not np.array_equal(limited, Q.predict(big, X[:50]))


# ---- the public classes without a GPU ---------------------------------------------------------------------------------------------------------------
def test_clone_round_trips_the_parameters():
    from sklearn.base import clone
    from bbbp_amd.random_forest import DecisionTreeRegressor, RandomForestRegressor
    reg = RandomForestRegressor(300, max_depth=15, random_state=42)
    twin = clone(reg)
    assert twin is not reg and type(twin) is RandomForestRegressor and twin.get_params() == reg.get_params()
    assert reg.get_params() == dict(n_estimators=300, max_depth=15, min_samples_split=2, min_samples_leaf=1, max_features=1.0, bootstrap=True,
                                    random_state=42, device="cuda")
    tree = clone(DecisionTreeRegressor(max_depth=3, min_samples_leaf=np.int64(2)))
    assert tree.get_params() == dict(max_depth=3, min_samples_split=2, min_samples_leaf=2, max_features=None, bootstrap=False, random_state=0,
                                     device="cuda") and tree.n_estimators == 1
    assert reg.set_params(max_depth=None, n_estimators=7) is reg and reg.max_depth is None and reg.n_estimators == 7
    with pytest.raises(ValueError, match="n_estimators"):
        reg.set_params(n_estimators=0)
    with pytest.raises(ValueError, match="unknown"):
        reg.set_params(gamma=1)
    assert reg.n_estimators == 7 and not hasattr(reg, "estimators_") and not hasattr(reg, "trees_")


def test_refusals_without_a_gpu():
    from bbbp_amd.random_forest import DecisionTreeRegressor, MAX_FEATURES, MAX_ROWS, RandomForestRegressor, fit_regressors
    for kw in (dict(criterion="absolute_error"), dict(criterion="friedman_mse"), dict(max_samples=0.5), dict(max_leaf_nodes=8), dict(ccp_alpha=0.1),
               dict(min_impurity_decrease=0.1), dict(oob_score=True), dict(min_samples_split=0.1), dict(min_samples_leaf=0.05), dict(max_features=0.5)):
        name = next(iter(kw))
        with pytest.raises(NotImplementedError, match=name):
            RandomForestRegressor(**kw)
        with pytest.raises(NotImplementedError, match=name):
            DecisionTreeRegressor(**kw)
    with pytest.raises(ValueError, match="unknown parameter"):
        RandomForestRegressor(gamma=1)
    with pytest.raises(ValueError, match="random_state"):
        RandomForestRegressor(random_state=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RandomForestRegressor(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DecisionTreeRegressor(device="cpu")
    with pytest.raises(ValueError, match="max_features"):
        RandomForestRegressor(max_features="auto")
    reg = RandomForestRegressor(criterion="squared_error", oob_score=False)        # the defaults, spelled out, are accepted
    assert reg.n_estimators == 100 and reg.max_features == 1.0 and reg.bootstrap and reg.random_state == 0
    for mf in (1.0, None, "sqrt", "log2", 3):
        RandomForestRegressor(max_features=mf)
    X, y = np.zeros((6, 2)), np.arange(6.0)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        reg.fit(X, y, sample_weight=np.ones(6))
    with pytest.raises(NotImplementedError, match="multi-output"):
        reg.fit(X, np.zeros((6, 2)))
    with pytest.raises(ValueError, match="NaN"):
        reg.fit(X, np.array([0.0, 1.0, np.nan, 0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="NaN"):
        reg.fit(np.full((6, 2), np.nan), y)
    with pytest.raises(ValueError, match="rows"):
        reg.fit(X, y[:5])
    with pytest.raises(ValueError, match="BBBP_RF_FIT_MAX_N"):
        reg.fit(np.zeros((MAX_ROWS + 1, 1)), np.zeros(MAX_ROWS + 1))
    with pytest.raises(ValueError, match="BBBP_RF_FIT_MAX_D"):
        reg.fit(np.zeros((4, MAX_FEATURES + 1)), np.zeros(4))
    with pytest.raises(ValueError, match="max_features"):
        RandomForestRegressor(max_features=3).fit(X, y)
    with pytest.raises(RuntimeError, match="not fitted"):
        reg.predict(X)
    with pytest.raises(AttributeError, match="feature_importances_ is not supported"):
        reg.feature_importances_
    with pytest.raises(ValueError, match="no problems"):
        fit_regressors([])
    with pytest.raises(NotImplementedError, match="criterion"):
        fit_regressors([(X, y)], criterion="poisson")


def test_new_symbols_are_declared_bound_and_exported():
    from bbbp_amd import _lib
    new = ["bbbp_rf_fit_regression", "bbbp_rf_fit_regression_work_bytes", "bbbp_rf_predict_mean"]
    L = _lib.lib()
    for name in new:
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(L, name)
    # validation runs before any GPU call: these answer on a machine without one
    assert L.bbbp_rf_fit_regression_work_bytes(8193, 4, 2) == 0 and b"BBBP_RF_FIT_MAX_N" in L.bbbp_last_error()
    assert L.bbbp_rf_fit_regression_work_bytes(100, 1025, 2) == 0 and b"BBBP_RF_FIT_MAX_D" in L.bbbp_last_error()
    assert L.bbbp_rf_fit_regression_work_bytes(100, 4, 5) == 0 and b"max_features" in L.bbbp_last_error()
    for n, d, mf in [(2, 1, 1), (257, 5, 2), (8192, 1024, 32)]:
        assert L.bbbp_rf_fit_regression_work_bytes(n, d, mf) == L.bbbp_rf_fit_work_bytes(n, d, mf) + sum((b * n + 15) // 16 * 16 for b in (8, 2, 8))
    assert L.bbbp_rf_fit_regression(None, None, None, 1, None) != 0 and b"null pointer" in L.bbbp_last_error()
    assert L.bbbp_rf_predict_mean(None, None, 4, 0, 4, *[None] * 7, 1, 1, 2, None) != 0 and b"positive" in L.bbbp_last_error()
    tree = _lib.RfTree(1, 1, 1, 9000, 4, 3, 2, 1, 2, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert L.bbbp_rf_fit_regression(None, (_lib.RfTree * 1)(tree), 1, 1, 1) != 0 and b"BBBP_RF_FIT_MAX_N" in L.bbbp_last_error()
