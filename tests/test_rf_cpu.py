"""CPU: the numpy restatement of random_forest's fit (tests/rf_numpy.py), its certifier (tests/rf_replay.py) and what random_forest refuses
without a GPU.  The replayer must accept scikit-learn's weighted trees and the restatement's, and reject planted faults by name."""
import functools

import numpy as np
import pytest

import rf_numpy as N
import rf_replay as R
from gbt_replay import make_data


@functools.lru_cache(maxsize=None)
def _data():
    """300 x 8 with a column rounded to one decimal (heavy value ties) and a binary column."""
    X, y = make_data(300, 8, seed=3)
    X[:, 1] = np.round(X[:, 1], 1)
    X[:, 2] = (X[:, 2] > 0).astype(np.float64)
    X.setflags(write=False); y.setflags(write=False)
    return X, y


def _copy(trees):
    return {k: v.copy() for k, v in trees.items()}


# ---- the replayer accepts correct trees ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msl", [1, 2, 4])
@pytest.mark.parametrize("mss", [2, 5, 10])
def test_replayer_accepts_sklearn_weighted_trees(msl, mss):
    """scikit-learn's DecisionTreeClassifier under bootstrap-count sample weights: every split attains the exact maximum (zero allowance)."""
    from sklearn.tree import DecisionTreeClassifier
    X, y = _data()
    splits = ties = 0
    for t in range(2):
        w = N.bootstrap_weights(11, t, len(y))
        sk = DecisionTreeClassifier(min_samples_leaf=msl, min_samples_split=mss, random_state=t).fit(X, y, sample_weight=w.astype(np.float64))
        seen = R.replay(X, y, R.trees_of_sklearn(sk), min_samples_split=mss, min_samples_leaf=msl, weights=[w])
        assert seen["nodes"] == sk.tree_.node_count
        splits += seen["splits"]; ties += seen["ties"]
    print(f"msl {msl} mss {mss}: {splits} splits, {ties} with an exact tie for the maximum")
    assert splits >= 10


@pytest.mark.parametrize("kw", [dict(), dict(max_depth=4), dict(min_samples_split=10, min_samples_leaf=3), dict(max_features=None, bootstrap=False),
                                dict(max_features=3, min_samples_leaf=2), dict(max_features="log2", max_depth=6)])
def test_replayer_accepts_the_restatement(kw):
    X, y = _data()
    trees = N.fit_forest(X, y, 3, seed=5, **kw)
    seen = R.replay(X, y, trees, seed=5, own=True, **{"max_features": "sqrt", **kw})
    assert seen["splits"] >= 3 and len(trees["root"]) == 4
    if "max_depth" in kw:
        assert seen["max_depth"] == kw["max_depth"] and seen["stop_reasons"].get("depth", 0) > 0


def test_restatement_numbers_nodes_level_by_level():
    X, y = _data()
    trees = N.fit_forest(X, y, 2, seed=1)
    for t in range(2):
        lo, hi = trees["root"][t], trees["root"][t + 1]
        kids = np.stack([trees["left"][lo:hi], trees["right"][lo:hi]], axis=1)
        kids = kids[kids[:, 0] >= 0].ravel()
        assert np.array_equal(kids, np.arange(lo + 1, hi))              # children in order of their parents, two by two


def test_pruning_and_prefix_property_of_the_restatement():
    """A tree under a larger min_samples_split or a smaller max_depth is the pruning of the unlimited tree; fewer trees are a prefix."""
    from bbbp_amd.random_forest import _prune
    X, y = _data()
    big = N.fit_forest(X, y, 3, seed=2, min_samples_leaf=2)
    big["value0"] = 1.0 - big["value"]
    for T, depth, mss in [(3, None, 2), (2, 3, 2), (3, None, 10), (1, 4, 10)]:
        single = N.fit_forest(X, y, T, seed=2, min_samples_leaf=2, max_depth=depth, min_samples_split=mss)
        cut = _prune(big, T, depth, mss)
        assert all(np.array_equal(cut[k], single[k]) for k in single), (T, depth, mss)


# ---- the replayer rejects planted faults ----------------------------------------------------------------------------------------------------
def _root_candidates(X, y, w, msl):
    """Per feature the root's valid positions, their float64 scores and the sorted float32 values."""
    X32 = X.astype(np.float32)
    rows = np.nonzero(w > 0)[0]
    out = {}
    for f in range(X.shape[1]):
        o = np.argsort(X32[rows, f], kind="stable")
        p, num, den = N.position_scores(X32[rows, f][o], w[rows][o], (w * y)[rows][o], msl)
        out[f] = (p, num / den, X32[rows, f][o])
    return out


def _expect(check, X, y, trees, **kw):
    with pytest.raises(R.ReplayError) as e:
        R.replay(X, y, trees, **kw)
    assert e.value.check == check, str(e.value)


def test_replayer_rejects_planted_faults():
    X, y = _data()
    kw = dict(seed=7, own=True, max_features=None, min_samples_leaf=3, bootstrap=True)
    good = N.fit_forest(X, y, 1, seed=7, max_features=None, min_samples_leaf=3)
    R.replay(X, y, good, **kw)
    w = N.bootstrap_weights(7, 0, len(y))
    cands = _root_candidates(X, y, w, 3)
    # a second-best split: the best position of another feature, whose score is strictly lower
    f0 = int(good["feature"][0])
    other = min((f for f in cands if f != f0 and len(cands[f][0]) and cands[f][1].max() < cands[f0][1].max()), key=lambda f: -cands[f][1].max())
    p, score, fv = cands[other]
    j = int(np.argmax(score))
    bad = _copy(good)
    bad["feature"][0], bad["threshold"][0] = other, N.midpoint(fv[p[j] - 1], fv[p[j]])
    _expect("optimal", X, y, bad, **kw)
    # a threshold off by one float32
    bad = _copy(good)
    bad["threshold"][0] = np.float64(np.nextafter(np.float32(good["threshold"][0]), np.float32(np.inf))) + 0.0
    assert bad["threshold"][0] != good["threshold"][0]
    _expect("valid", X, y, bad, **kw)
    # a wrong n_node_samples
    bad = _copy(good)
    bad["n_node_samples"][1] += 1
    _expect("samples", X, y, bad, **kw)
    # a violated min_samples_leaf: one row on the left where three are asked for
    p, score, fv = _root_candidates(X, y, w, 1)[f0]
    assert p[0] == 1
    bad = _copy(good)
    bad["threshold"][0] = N.midpoint(fv[0], fv[1])
    _expect("valid", X, y, bad, **kw)
    # a wrong value
    bad = _copy(good)
    bad["value"][0] = np.nextafter(bad["value"][0], 2.0)
    _expect("samples", X, y, bad, **kw)
    # a leaf where a split is due
    bad = _copy(good)
    bad["left"][0] = bad["right"][0] = -1
    _expect("stop", X, y, bad, **kw)


def test_replayer_rejects_a_feature_outside_the_draw():
    X, y = _data()
    kw = dict(seed=7, own=True, max_features=2, bootstrap=True)
    good = N.fit_forest(X, y, 1, seed=7, max_features=2)
    R.replay(X, y, good, **kw)
    w = N.bootstrap_weights(7, 0, len(y))
    drawn = set(int(f) for f in N.draw_features(N.tree_key(7, 0), X.astype(np.float32)[w > 0], 2))
    assert len(drawn) == 2 and int(good["feature"][0]) in drawn
    cands = _root_candidates(X, y, w, 1)
    outside = next(f for f in range(X.shape[1]) if f not in drawn)
    p, score, fv = cands[outside]
    j = int(np.argmax(score))
    bad = _copy(good)
    bad["feature"][0], bad["threshold"][0] = outside, N.midpoint(fv[p[j] - 1], fv[p[j]])
    _expect("draw", X, y, bad, **kw)


def test_replayer_rejects_a_tie_taken_against_the_rule():
    """Column 5 is a copy of column 0: every score of one is a score of the other.  Naming the copy is optimal and valid, yet not the rule's."""
    X, y = _data()
    X = X.copy()
    X[:, 5] = X[:, 0]
    kw = dict(seed=3, own=True, max_features=None, bootstrap=False)
    good = N.fit_forest(X, y, 1, seed=3, max_features=None, bootstrap=False)
    seen = R.replay(X, y, good, **kw)
    split = good["left"] >= 0
    assert seen["ties"] >= 1 and (good["feature"][split] == 0).any() and not (good["feature"][split] == 5).any()
    bad = _copy(good)
    bad["feature"][np.nonzero(split & (good["feature"] == 0))[0][0]] = 5
    _expect("tie", X, y, bad, **kw)
    R.replay(X, y, bad, **{**kw, "own": False})                 # as some other implementation's tree it is a correct one


# ---- the hash ---------------------------------------------------------------------------------------------------------------------------------
def test_hash_equals_the_library():
    from bbbp_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(0)
    for a, b in [(0, 0), (1, 0), (0, 1), ((1 << 64) - 1, (1 << 64) - 1)] + [tuple(int(v) for v in rs.randint(0, 2 ** 62, 2)) for _ in range(20)]:
        assert int(N.rf_hash(a, b)) == L.bbbp_rf_hash(a, b)
    assert np.array_equal(N.rf_hash(5, np.arange(4, dtype=np.uint64)), [N.rf_hash(5, j) for j in range(4)])


def test_bootstrap_share_of_distinct_rows():
    n = 2000
    share = np.mean([(N.bootstrap_weights(0, t, n) > 0).mean() for t in range(50)])
    assert all(N.bootstrap_weights(0, t, n).sum() == n for t in range(3))
    assert abs(share - 0.632) <= 0.02, share


@pytest.mark.parametrize("mf", [1, 3, 6])
def test_root_draw_frequencies(mf):
    d, T = 12, 2000
    Xn = np.random.RandomState(1).randn(5, d).astype(np.float32)
    counts = np.zeros(d)
    for t in range(T):
        drawn = N.draw_features(N.tree_key(0, t), Xn, mf)
        assert len(drawn) == mf and len(set(drawn)) == mf
        counts[drawn] += 1
    p = mf / d
    assert np.all(np.abs(counts / T - p) <= 5 * np.sqrt(p * (1 - p) / T)), counts / T


def test_draw_skips_constant_features():
    Xn = np.random.RandomState(2).randn(6, 5).astype(np.float32)
    Xn[:, 1] = 2.0
    Xn[:, 3] = Xn[0, 3] + np.float32(5e-8) * (np.arange(6) % 2)          # not more than 1e-7f apart: constant
    for t in range(20):
        assert set(N.draw_features(N.tree_key(1, t), Xn, 4)) == {0, 2, 4}        # fewer non-constant features than max_features: all of them
        assert not {1, 3} & set(N.draw_features(N.tree_key(1, t), Xn, 2))


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    from bbbp_amd.random_forest import DecisionTreeClassifier, MAX_FEATURES, MAX_ROWS, RandomForestClassifier, grid_search_cv
    for kw in (dict(criterion="entropy"), dict(class_weight="balanced"), dict(max_samples=0.5), dict(max_leaf_nodes=8), dict(ccp_alpha=0.1),
               dict(min_impurity_decrease=0.1), dict(oob_score=True), dict(min_samples_split=0.1), dict(min_samples_leaf=0.05), dict(max_features=0.5)):
        name = next(iter(kw))
        with pytest.raises(NotImplementedError, match=name):
            RandomForestClassifier(**kw)
        with pytest.raises(NotImplementedError, match=name):
            DecisionTreeClassifier(**kw)
    with pytest.raises(ValueError, match="unknown parameter"):
        RandomForestClassifier(gamma=1)
    with pytest.raises(ValueError, match="random_state"):
        RandomForestClassifier(random_state=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RandomForestClassifier(device="cpu")
    with pytest.raises(ValueError, match="n_estimators"):
        RandomForestClassifier(0)
    with pytest.raises(ValueError, match="max_features"):
        RandomForestClassifier(max_features="auto")
    clf = RandomForestClassifier(criterion="gini", oob_score=False)           # the defaults, spelled out, are accepted
    assert clf.n_estimators == 100 and clf.max_features == "sqrt" and clf.bootstrap and clf.random_state == 0
    tree = DecisionTreeClassifier()
    assert tree.n_estimators == 1 and tree.max_features is None and not tree.bootstrap
    X, y = np.zeros((6, 2)), np.array([0, 1, 2, 0, 1, 2])
    with pytest.raises(ValueError, match="3 classes"):
        clf.fit(X, y)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        clf.fit(X, y % 2, sample_weight=np.ones(6))
    with pytest.raises(ValueError, match="NaN"):
        clf.fit(np.full((6, 2), np.nan), y % 2)
    with pytest.raises(ValueError, match="BBBP_RF_FIT_MAX_N"):
        clf.fit(np.zeros((MAX_ROWS + 1, 1)), np.arange(MAX_ROWS + 1) % 2)
    with pytest.raises(ValueError, match="BBBP_RF_FIT_MAX_D"):
        clf.fit(np.zeros((4, MAX_FEATURES + 1)), [0, 1, 0, 1])
    with pytest.raises(ValueError, match="max_features"):
        RandomForestClassifier(max_features=3).fit(np.zeros((4, 2)), [0, 1, 0, 1])
    with pytest.raises(ValueError, match="unsupported grid keys"):
        grid_search_cv(X, y % 2, {"criterion": ["gini"]})
    with pytest.raises(RuntimeError, match="not fitted"):
        clf.predict(X)
