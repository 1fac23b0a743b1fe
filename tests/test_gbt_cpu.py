"""CPU: the boosted-tree replayer (tests/gbt_replay.py) accepts scikit-learn's own fits and rejects planted faults, each by its named
check; every refusal of gradient_boosting and of its C entry points comes before any GPU call; grid_search_cv's point order and keys."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
import gbt_replay as R

ERR_ARG = 1
SHAPES = [(257, 5, 3, 2, None), (257, 5, 7, 2, None), (300, 8, 5, 10, None), (257, 5, 5, 2, 1)]      # n, d, max_depth, min_samples_split, decimals


@functools.lru_cache(maxsize=None)
def sklearn_fit(n, d, depth, mss, decimals, random_state=0):
    from sklearn.ensemble import GradientBoostingClassifier as SK
    X, y = R.make_data(n, d, seed=1, decimals=decimals)
    sk = SK(n_estimators=10, max_depth=depth, min_samples_split=mss, random_state=random_state).fit(X, y)
    trees, init = R.trees_of_sklearn(sk)
    stages = np.array([s.ravel() for s in sk.staged_decision_function(X)])
    return X, y, sk, trees, init, stages


def _replay(case, trees=None, stages=None, **kw):
    X, y, sk, trees0, init, stages0 = sklearn_fit(*case)
    args = dict(max_depth=case[2], min_samples_split=case[3], min_samples_leaf=1)
    args.update(kw)
    return R.replay(X, y, trees0 if trees is None else trees, init, sk.learning_rate, raw_stages=stages0 if stages is None else stages,
                    train_score=sk.train_score_, **args)


@pytest.mark.parametrize("case", SHAPES)
@pytest.mark.parametrize("random_state", [0, 1])
def test_replayer_accepts_sklearn(case, random_state):
    seen = _replay(case + (random_state,))
    print({k: v for k, v in seen.items() if k != "raw"})
    assert seen["splits"] > 0 and seen["leaves"] > seen["splits"] and seen["leaf_share"] < 1.0
    X, y, sk, *_ = sklearn_fit(*case, random_state)
    assert np.array_equal(seen["raw"], sk.decision_function(X))           # the replay of raw += lr * value is exact


def test_sklearn_trees_differ_between_random_states():
    """Why no test compares trees with scikit-learn's: its own fits differ from seed to seed."""
    a, b = sklearn_fit(*SHAPES[0], 0), sklearn_fit(*SHAPES[0], 1)
    assert not (len(a[3]["threshold"]) == len(b[3]["threshold"]) and np.array_equal(a[3]["threshold"], b[3]["threshold"]))


def _root_candidates(case):
    """Every valid candidate of the first tree's root: (feature, position, score, allowance, threshold), best first."""
    X, y, sk, trees, init, _ = sklearn_fit(*case)
    X32 = X.astype(np.float32)
    g, D = R.residuals_x(y.astype(np.float64), np.full(len(y), init))
    out = []
    for f in range(X.shape[1]):
        o = np.argsort(X32[:, f], kind="stable")
        fv = X32[:, f][o]
        pos = R.candidates(fv, 1)
        score, allow = R._scores(g[o], D.sum(), pos)
        out += [(f, int(p), float(s), float(a), R.midpoint(fv[p - 1], fv[p])) for p, s, a in zip(pos, score, allow)]
    return sorted(out, key=lambda c: -c[2])


def _copy(trees):
    return {k: v.copy() for k, v in trees.items()}


def test_replayer_rejects_a_second_best_split():
    case = SHAPES[0]
    trees = _copy(sklearn_fit(*case)[3])
    cands = _root_candidates(case)
    best = cands[0]
    second = next(c for c in cands if c[2] + c[3] < best[2] - best[3])     # the best candidate that rounding cannot lift to the top
    assert int(trees["feature"][0]) == best[0] and trees["threshold"][0] == best[4]           # scikit-learn took the extended-precision maximum
    trees["feature"][0], trees["threshold"][0] = second[0], second[4]
    with pytest.raises(R.ReplayError) as e:
        _replay(case, trees=trees)
    assert e.value.check == "optimal"


def test_replayer_rejects_a_threshold_off_by_one_float32_neighbour():
    case = SHAPES[0]
    trees = _copy(sklearn_fit(*case)[3])
    thr = trees["threshold"][0]
    moved = np.float64(np.nextafter(np.float32(thr), np.float32(np.inf)))
    X32 = sklearn_fit(*case)[0].astype(np.float32)[:, int(trees["feature"][0])].astype(np.float64)
    assert moved != thr and ((X32 <= thr) == (X32 <= moved)).all()           # the same rows go left: only the threshold rule can object
    trees["threshold"][0] = moved
    with pytest.raises(R.ReplayError) as e:
        _replay(case, trees=trees)
    assert e.value.check == "threshold"
    trees = _copy(sklearn_fit(*case)[3])
    trees["n_node_samples"][1] += 1
    with pytest.raises(R.ReplayError) as e:
        _replay(case, trees=trees)
    assert e.value.check == "threshold"


def test_replayer_rejects_a_split_below_min_samples_split():
    case = SHAPES[1]                                                       # depth 7: nodes of a few rows are split
    trees = sklearn_fit(*case)[3]
    split_sizes = trees["n_node_samples"][trees["left"] >= 0]
    assert split_sizes.min() < 10
    with pytest.raises(R.ReplayError) as e:
        _replay(case, min_samples_split=10)
    assert e.value.check == "stop"
    with pytest.raises(R.ReplayError) as e:                                # and a leaf that no rule allows
        _replay(SHAPES[0], max_depth=4)
    assert e.value.check == "stop"


def test_replayer_rejects_a_leaf_value_off_by_1e_9():
    case = SHAPES[0]
    trees = _copy(sklearn_fit(*case)[3])
    first = np.arange(trees["root"][0], trees["root"][1])
    leaves = first[trees["left"][first] < 0]
    leaf = leaves[np.argmax(np.abs(trees["value"][leaves]))]               # in the first tree: the leaf whose residuals cancel least
    trees["value"][leaf] *= 1.0 + 1e-9
    with pytest.raises(R.ReplayError) as e:
        _replay(case, trees=trees)
    assert e.value.check == "leaf"


def test_replayer_rejects_a_missing_stage_update():
    case = SHAPES[0]
    stages = sklearn_fit(*case)[5].copy()
    stages[3:] -= stages[3] - stages[2]                                    # stage 3's update never reached the raw scores
    with pytest.raises(R.ReplayError) as e:
        _replay(case, stages=stages)
    assert e.value.check == "raw"
    X, y, sk, trees, init, st = sklearn_fit(*case)
    score = sk.train_score_.copy()
    score[5] *= 1.0 + 1e-9
    with pytest.raises(R.ReplayError) as e:
        R.replay(X, y, trees, init, sk.learning_rate, 3, 2, 1, raw_stages=st, train_score=score)
    assert e.value.check == "raw"


# ---- refusals: all on the host, before any GPU call (this machine has none: a GPU call would raise something else) ------------------------
def test_gradient_boosting_refusals():
    from bbbp_amd.gradient_boosting import GradientBoostingClassifier as GBC, grid_search_cv, MAX_ROWS, MAX_FEATURES
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GBC(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"max_depth": [1]}, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GBC().fit(torch.zeros(8, 4), [0, 1] * 4)
    for kw, name in ((dict(loss="exponential"), "loss"), (dict(criterion="squared_error"), "criterion"), (dict(subsample=0.5), "subsample"),
                     (dict(max_features="sqrt"), "max_features"), (dict(max_features=3), "max_features"), (dict(init="zero"), "init"),
                     (dict(init=object()), "init"), (dict(n_iter_no_change=5), "n_iter_no_change"), (dict(max_leaf_nodes=8), "max_leaf_nodes"),
                     (dict(ccp_alpha=0.01), "ccp_alpha"), (dict(min_impurity_decrease=0.1), "min_impurity_decrease"),
                     (dict(min_weight_fraction_leaf=0.1), "min_weight_fraction_leaf"), (dict(warm_start=True), "warm_start"), (dict(max_depth=8), "max_depth"),
                     (dict(max_depth=None), "max_depth"), (dict(max_depth=0), "max_depth"), (dict(min_samples_split=0.5), "min_samples_split"),
                     (dict(min_samples_split=1), "min_samples_split"), (dict(min_samples_leaf=0.1), "min_samples_leaf"), (dict(min_samples_leaf=0), "min_samples_leaf"),
                     (dict(n_estimators=0), "n_estimators"), (dict(n_estimators=2.5), "n_estimators"), (dict(learning_rate=0.0), "learning_rate"),
                     (dict(learning_rate=float("inf")), "learning_rate"), (dict(learning_rate="0.1"), "learning_rate"), (dict(colsample=1), "colsample")):
        with pytest.raises((ValueError, NotImplementedError), match=name):
            GBC(**kw)
    clf = GBC(50, 0.05, 5, 10, 3, subsample=1.0, max_features=None, random_state=7)
    assert (clf.n_estimators, clf.learning_rate, clf.max_depth, clf.min_samples_split, clf.min_samples_leaf) == (50, 0.05, 5, 10, 3)
    Xok, yok = np.zeros((6, 2)), [0, 1] * 3
    with pytest.raises(ValueError, match="sample_weight"):
        GBC().fit(Xok, yok, sample_weight=np.ones(6))
    with pytest.raises(ValueError, match="classes"):
        GBC().fit(Xok, [0, 1, 2] * 2)
    with pytest.raises(ValueError, match="classes"):
        GBC().fit(Xok, np.zeros(6))
    with pytest.raises(ValueError, match="rows"):
        GBC().fit(Xok, [0, 1] * 2)
    for bad in (np.nan, np.inf, -np.inf, 1e39):                            # 1e39 is finite in float64 and infinite in the float32 the trees compare
        Xbad = Xok.copy()
        Xbad[3, 1] = bad
        with pytest.raises(ValueError, match="NaN"):
            GBC().fit(Xbad, yok)
    with pytest.raises(ValueError, match="BBBP_GBT_FIT_MAX_N"):
        GBC().fit(np.zeros((MAX_ROWS + 1, 1)), [0, 1] * (MAX_ROWS // 2) + [0])
    with pytest.raises(ValueError, match="BBBP_GBT_FIT_MAX_D"):
        GBC().fit(np.zeros((4, MAX_FEATURES + 1)), [0, 1] * 2)
    with pytest.raises(ValueError, match="two rows"):
        GBC().fit(np.zeros((1, 2)), [0, 1])                                # the shape is judged before the row counts are compared
    with pytest.raises(ValueError, match="2-D"):
        GBC().fit(np.zeros(6), yok)
    for method in ("decision_function", "predict", "predict_proba", "predict_log_proba"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(GBC(), method)(np.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="not fitted"):
        next(GBC().staged_decision_function(np.zeros((2, 4))))


def test_grid_search_point_order_and_keys():
    from bbbp_amd.gradient_boosting import grid_points, grid_search_cv
    grid = {"n_estimators": [50, 100], "learning_rate": [0.01, 0.1], "max_depth": [3, 5], "min_samples_split": [2, 10]}
    points, full = grid_points(grid)
    from sklearn.model_selection import ParameterGrid
    assert points == list(ParameterGrid(grid)) and len(points) == 16
    assert points[0] == dict(learning_rate=0.01, max_depth=3, min_samples_split=2, n_estimators=50)
    assert points[1] == dict(learning_rate=0.01, max_depth=3, min_samples_split=2, n_estimators=100)
    assert full[1] == (100, 0.01, 3, 2, 1) and full[-1] == (100, 0.1, 5, 10, 1)
    two = [{"max_depth": [3]}, {"min_samples_leaf": [1, 3]}]
    assert grid_points(two)[0] == list(ParameterGrid(two)) and grid_points(two)[1] == [(100, 0.1, 3, 2, 1), (100, 0.1, 3, 2, 1), (100, 0.1, 3, 2, 3)]
    X, y = np.zeros((10, 2)), [0, 1] * 5
    with pytest.raises(ValueError, match="grid keys"):
        grid_search_cv(X, y, {"max_depth": [3], "subsample": [0.5]})
    with pytest.raises(ValueError, match="grid keys"):
        grid_search_cv(X, y, {"max_features": ["sqrt"]})
    with pytest.raises(ValueError, match="empty"):
        grid_search_cv(X, y, [])
    with pytest.raises(NotImplementedError, match="max_depth"):
        grid_search_cv(X, y, {"max_depth": [3, 9]})
    with pytest.raises(ValueError, match="learning_rate"):
        grid_search_cv(X, y, [{"max_depth": [3]}, {"learning_rate": [0.0]}])
    with pytest.raises(ValueError, match="classes"):
        grid_search_cv(X, np.arange(10), {"max_depth": [3]}, device="cuda")
    with pytest.raises(ValueError, match="rows"):
        grid_search_cv(X, [0, 1] * 4, {"max_depth": [3]})
    with pytest.raises(ValueError, match="NaN"):
        grid_search_cv(np.full((10, 2), np.nan), y, {"max_depth": [3]})


def _chain(**kw):
    base = dict(XT=4096, order0=4096, y=4096, n=257, d=5, n_estimators=10, max_depth=3, min_samples_split=2, min_samples_leaf=1, learning_rate=0.1, init=0.0,
                work=4096, left=4096, right=4096, feature=4096, n_node_samples=4096, threshold=4096, value=4096, tree_nodes=4096, train_score=4096, raw=4096)
    base.update(kw)
    return _lib.GbtChain(**base)


def test_gbt_entry_points_validate_before_touching_the_gpu():
    """Pointers are the fake address 4096: validation comes first and none is dereferenced."""
    L = _lib.lib()
    fit = lambda **kw: L.bbbp_gbt_fit(None, ctypes.byref(_chain(**kw)), 4096, 1)  # noqa: E731
    for bad, word in ((dict(n=1), b"n >= 2"), (dict(d=0), b"d >= 1"), (dict(n=8193), b"BBBP_GBT_FIT_MAX_N"), (dict(d=1025), b"BBBP_GBT_FIT_MAX_D"),
                      (dict(max_depth=0), b"max_depth"), (dict(max_depth=8), b"max_depth"), (dict(n_estimators=0), b"n_estimators"),
                      (dict(n_estimators=10001), b"n_estimators"), (dict(min_samples_split=1), b"min_samples_split"), (dict(min_samples_leaf=0), b"min_samples_leaf"),
                      (dict(learning_rate=0.0), b"learning_rate"), (dict(learning_rate=float("nan")), b"learning_rate"), (dict(init=float("inf")), b"init"),
                      (dict(XT=None), b"null"), (dict(order0=None), b"null"), (dict(y=None), b"null"), (dict(work=None), b"null"), (dict(left=None), b"null"),
                      (dict(value=None), b"null"), (dict(tree_nodes=None), b"null"), (dict(train_score=None), b"null"), (dict(raw=None), b"null")):
        assert fit(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert L.bbbp_gbt_fit(None, None, 4096, 1) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_gbt_fit(None, ctypes.byref(_chain()), None, 1) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_gbt_fit(None, ctypes.byref(_chain()), 4096, 0) == ERR_ARG and b"n_chains" in L.bbbp_last_error()
    two = (_lib.GbtChain * 2)(_chain(), _chain(max_depth=9))               # the second of a batch is examined too
    assert L.bbbp_gbt_fit(None, two, 4096, 2) == ERR_ARG and b"chain 1" in L.bbbp_last_error()

    dec = lambda X=4096, ld=5, m=7, d=5, left=4096, root=4096, n_trees=3, stages=4096, n_stages=2, out=4096: L.bbbp_gbt_staged_decision(  # noqa: E731
        None, X, ld, m, d, left, 4096, 4096, 4096, 4096, root, n_trees, 0.0, 0.1, stages, n_stages, out)
    for bad, word in ((dict(m=0), b"positive"), (dict(d=0), b"positive"), (dict(ld=4), b"leading"), (dict(n_trees=0), b"n_stages"), (dict(n_stages=0), b"n_stages"),
                      (dict(n_stages=4), b"n_stages"), (dict(X=None), b"null"), (dict(left=None), b"null"), (dict(root=None), b"null"), (dict(stages=None), b"null"),
                      (dict(out=None), b"null")):
        assert dec(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad

    nbytes = L.bbbp_gbt_fit_work_bytes
    assert nbytes(1, 3) == 0 and b"n >= 2" in L.bbbp_last_error()
    assert nbytes(8193, 3) == 0 and b"BBBP_GBT_FIT_MAX_N" in L.bbbp_last_error()
    assert nbytes(100, 1025) == 0 and b"BBBP_GBT_FIT_MAX_D" in L.bbbp_last_error()
    assert nbytes(8000, 100) >= 2 * 8000 * 100 * 4 and nbytes(8000, 100) % 16 == 0 and nbytes(2, 1) > 0
    assert [L.bbbp_gbt_fit_tree_capacity(k) for k in (0, 1, 3, 7, 8)] == [0, 3, 15, 255, 0]
