"""CPU: the squared-error replayer (tests/gbr_replay.py) accepts scikit-learn's own GradientBoostingRegressor fits and rejects planted
faults, each by its named check; the numpy restatement of the fit kernels (tests/gbr_numpy.py) passes it and agrees with scikit-learn on
the training rows within a derived bound; bbbp_gbr_fit and gradient_boosting.GradientBoostingRegressor refuse before any GPU call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
import gbr_numpy
import gbr_replay as R

ERR_ARG = 1
IDS = [f"{'-'.join(str(v) for v in c)}-{v}-{T}" for c, v, T in R.CASES]
PLAIN = ((257, 5, 3, 2, 1, 0.1), None, 8)                                  # the case the faults are planted in


@functools.lru_cache(maxsize=None)
def sklearn_fit(case, variant, T, random_state=0):
    from sklearn.ensemble import GradientBoostingRegressor as SK
    n, d, depth, mss, msl, lr = case
    X, y = R.make_data(n, d, variant=variant)
    sk = SK(n_estimators=T, learning_rate=lr, max_depth=depth, min_samples_split=mss, min_samples_leaf=msl, random_state=random_state).fit(X, y)
    trees, init = R.trees_of_sklearn(sk)
    return X, y, sk, trees, init, np.array(list(sk.staged_predict(X)))


def _replay(entry, trees=None, stages=None, score=None, random_state=0, **kw):
    case = entry[0]
    X, y, sk, trees0, init, stages0 = sklearn_fit(*entry, random_state)
    args = dict(max_depth=case[2], min_samples_split=case[3], min_samples_leaf=case[4])
    args.update(kw)
    return R.replay(X, y, trees0 if trees is None else trees, init, case[5], raw_stages=stages0 if stages is None else stages,
                    train_score=sk.train_score_ if score is None else score, **args)


@pytest.mark.parametrize("entry", R.CASES, ids=IDS)
@pytest.mark.parametrize("random_state", [0, 1, 2])
def test_replayer_accepts_sklearn(entry, random_state):
    (n, d, *_), variant, T = entry
    seen = _replay(entry, random_state=random_state)
    print({k: v for k, v in seen.items() if k != "raw"})
    X, y, sk, trees, init, stages = sklearn_fit(*entry, random_state)
    assert init == float(np.average(y))                                   # scikit-learn's DummyRegressor constant, bit for bit
    assert np.array_equal(seen["raw"], sk.predict(X))                       # the replay of raw += lr * value is exact
    assert seen["leaf_share"] < 1.0
    if variant == "constant_y":
        assert seen["nodes"] == T and seen["stop_reasons"] == {"impurity": T} and not sk.train_score_.any()
    else:
        assert seen["splits"] >= T and seen["leaves"] > seen["splits"]
    if variant == "flat":
        assert seen["stop_reasons"].get("impurity", 0) >= 1


def test_sklearn_trees_differ_between_random_states_on_ties():
    """Why no test compares trees with scikit-learn's: where candidates tie, its own fits differ from seed to seed."""
    entry = ((257, 5, 7, 2, 1, 0.1), None, 8)                               # depth 7: two-row nodes, where every feature ties
    a, b = sklearn_fit(*entry, 0)[3], sklearn_fit(*entry, 1)[3]
    assert not (len(a["feature"]) == len(b["feature"]) and np.array_equal(a["feature"], b["feature"]) and np.array_equal(a["threshold"], b["threshold"]))


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
def _root_candidates(entry):
    """Every valid candidate of the first tree's root: (feature, position, score, allowance, threshold), best first."""
    X, y, sk, trees, init, _ = sklearn_fit(*entry)
    X32 = X.astype(np.float32)
    g, D = R.residuals_x(y, np.full(len(y), init))
    out = []
    for f in range(X.shape[1]):
        o = np.argsort(X32[:, f], kind="stable")
        fv = X32[:, f][o]
        pos = R.candidates(fv, entry[0][4])
        score, allow = R._scores(g[o], D.sum(), pos)
        out += [(f, int(p), float(s), float(a), R.midpoint(fv[p - 1], fv[p])) for p, s, a in zip(pos, score, allow)]
    return sorted(out, key=lambda c: -c[2])


def _copy(trees):
    return {k: v.copy() for k, v in trees.items()}


def _rejected(check, **kw):
    with pytest.raises(R.ReplayError) as e:
        _replay(PLAIN, **kw)
    assert e.value.check == check, str(e.value)


def test_replayer_rejects_a_threshold_moved_to_a_neighbouring_value():
    trees = _copy(sklearn_fit(*PLAIN)[3])
    thr = trees["threshold"][0]
    moved = np.float64(np.nextafter(np.float32(thr), np.float32(np.inf)))
    col = sklearn_fit(*PLAIN)[0].astype(np.float32)[:, int(trees["feature"][0])].astype(np.float64)
    assert moved != thr and ((col <= thr) == (col <= moved)).all()           # the same rows go left: only the threshold rule can object
    trees["threshold"][0] = moved
    _rejected("threshold", trees=trees)
    trees = _copy(sklearn_fit(*PLAIN)[3])
    trees["n_node_samples"][1] += 1
    _rejected("threshold", trees=trees)


def test_replayer_rejects_a_leaf_value_off_by_1e_9():
    trees = _copy(sklearn_fit(*PLAIN)[3])
    first = np.arange(trees["root"][0], trees["root"][1])
    leaves = first[trees["left"][first] < 0]
    leaf = leaves[np.argmax(np.abs(trees["value"][leaves]))]
    trees["value"][leaf] *= 1.0 + 1e-9
    _rejected("leaf", trees=trees)
    trees = _copy(sklearn_fit(*PLAIN)[3])                                    # a split node's value is held to the same rule
    inner = first[trees["left"][first] >= 0]
    trees["value"][inner[np.argmax(np.abs(trees["value"][inner]))]] *= 1.0 + 1e-9
    _rejected("leaf", trees=trees)


def test_replayer_rejects_a_second_best_split():
    trees = _copy(sklearn_fit(*PLAIN)[3])
    cands = _root_candidates(PLAIN)
    best = cands[0]
    second = next(c for c in cands if c[2] + c[3] < best[2] - best[3])     # the best candidate that rounding cannot lift to the top
    assert int(trees["feature"][0]) == best[0] and trees["threshold"][0] == best[4]           # scikit-learn took the extended-precision maximum
    trees["feature"][0], trees["threshold"][0] = second[0], second[4]
    _rejected("optimal", trees=trees)


def test_replayer_rejects_a_splittable_node_turned_into_a_leaf():
    trees = _copy(sklearn_fit(*PLAIN)[3])
    node = int(trees["left"][0])                                            # the root's left child: 100 rows or so, depth 1 of 3
    assert trees["left"][node] >= 0 and trees["n_node_samples"][node] >= 4
    trees["left"][node] = trees["right"][node] = -1
    _rejected("stop", trees=trees)
    _rejected("stop", max_depth=4)                                          # and leaves at depth 3 that no rule allows under max_depth 4


def test_replayer_rejects_a_split_below_min_samples_leaf():
    """The root's split leaves fewer rows on one side than a larger min_samples_leaf allows: it is then no valid position (``optimal``); a
    node of fewer than 2 min_samples_leaf rows must not be split at all (``stop``)."""
    trees = sklearn_fit(*PLAIN)[3]
    small = int(min(trees["n_node_samples"][trees["left"][0]], trees["n_node_samples"][trees["right"][0]]))
    assert 2 * (small + 1) <= 257
    _rejected("optimal", min_samples_leaf=small + 1)
    _rejected("stop", min_samples_leaf=129)


def test_replayer_rejects_a_stage_off_by_1e_12():
    X, y, sk, trees, init, stages = sklearn_fit(*PLAIN)
    off = stages.copy()
    off[3, 17] += 1e-12                                                     # one row of one stage
    _rejected("raw", stages=off)
    off = stages.copy()
    off[3:] -= stages[3] - stages[2]                                        # stage 3's update never reached the predictions
    _rejected("raw", stages=off)
    score = sk.train_score_.copy()
    score[5] *= 1.0 + 1e-9
    _rejected("raw", score=score)


# ---- the numpy restatement of the kernels -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def numpy_fit(case, variant, T):
    n, d, depth, mss, msl, lr = case
    X, y = R.make_data(n, d, variant=variant)
    return (X, y) + gbr_numpy.fit(X, y, T, lr, depth, mss, msl)


@pytest.mark.parametrize("entry", R.CASES, ids=IDS)
def test_restatement_passes_the_replayer(entry):
    (n, d, depth, mss, msl, lr), variant, T = entry
    X, y, trees, init, stages, scores = numpy_fit(*entry)
    seen = R.replay(X, y, trees, init, lr, depth, mss, msl, raw_stages=stages, train_score=scores)
    print({k: v for k, v in seen.items() if k != "raw"})
    assert init == float(np.average(y)) and len(trees["root"]) == T + 1
    if variant == "constant_y":
        assert len(trees["left"]) == T and not trees["value"].any() and not scores.any() and (stages == 1.5).all()
    if variant == "constant":
        assert not (trees["feature"][trees["left"] >= 0] == 2).any()


PARITY = [(c, None, T) for c, T in R.PARITY_CASES] + [((257, 5, 5, 2, 1, 0.1), None, 20)]


@pytest.mark.parametrize("entry", PARITY, ids=[f"{'-'.join(str(v) for v in c)}-{T}" for c, _, T in PARITY])
def test_restatement_agrees_with_sklearn_on_the_training_rows(entry):
    """On continuous features exact score ties arise only between candidates that induce the same partition (any feature splits a two-row
    node), so the training rows' predictions do not depend on how ties are broken: the restatement's staged predictions and train_score_
    agree with scikit-learn's within ``gbr_replay.parity_bound``, whatever either did with its ties."""
    case, _, T = entry
    X, y, trees, init, stages, scores = numpy_fit(*entry)
    _, _, sk, sk_trees, sk_init, sk_stages = sklearn_fit(*entry, 0)
    bound, score_bound = R.parity_bound(y, sk_stages, case[5], sk_init)
    err = np.abs(stages - sk_stages).max(axis=1)
    score_err = np.abs(scores - sk.train_score_)
    spread = max(float(np.abs(sklearn_fit(*entry, rs)[5] - sk_stages).max()) for rs in (1, 2))
    print(f"{entry}: max |restatement - scikit-learn| {err.max():.3e} (bound at the last stage {bound[-1]:.3e}), train_score_ {score_err.max():.3e} "
          f"(bound {score_bound[-1]:.3e}); scikit-learn's own spread over random_state 0..2: {spread:.3e}")
    assert init == sk_init and len(trees["left"]) == len(sk_trees["left"])
    assert (err <= bound).all() and (score_err <= score_bound).all()


# ---- refusals: all on the host, before any GPU call (this machine has none: a GPU call would raise something else) ----------------------
def _chain(**kw):
    base = dict(XT=4096, order0=4096, y=4096, n=257, d=5, n_estimators=10, max_depth=3, min_samples_split=2, min_samples_leaf=1, learning_rate=0.1, init=0.0,
                work=4096, left=4096, right=4096, feature=4096, n_node_samples=4096, threshold=4096, value=4096, tree_nodes=4096, train_score=4096, raw=4096)
    base.update(kw)
    return _lib.GbtChain(**base)


def test_gbr_entry_point_validates_before_touching_the_gpu():
    """Pointers are the fake address 4096: validation comes first and none is dereferenced."""
    L = _lib.lib()
    assert hasattr(L, "bbbp_gbr_fit") and "bbbp_gbr_fit" in _lib._SIGNATURES
    fit = lambda **kw: L.bbbp_gbr_fit(None, ctypes.byref(_chain(**kw)), 4096, 1)  # noqa: E731
    for bad, word in ((dict(n=1), b"n >= 2"), (dict(d=0), b"d >= 1"), (dict(n=8193), b"BBBP_GBT_FIT_MAX_N"), (dict(d=1025), b"BBBP_GBT_FIT_MAX_D"),
                      (dict(max_depth=0), b"max_depth"), (dict(max_depth=8), b"max_depth"), (dict(n_estimators=0), b"n_estimators"),
                      (dict(n_estimators=10001), b"n_estimators"), (dict(min_samples_split=1), b"min_samples_split"), (dict(min_samples_leaf=0), b"min_samples_leaf"),
                      (dict(learning_rate=0.0), b"learning_rate"), (dict(learning_rate=float("nan")), b"learning_rate"), (dict(init=float("inf")), b"init"),
                      (dict(XT=None), b"null"), (dict(order0=None), b"null"), (dict(y=None), b"null"), (dict(work=None), b"null"), (dict(left=None), b"null"),
                      (dict(value=None), b"null"), (dict(tree_nodes=None), b"null"), (dict(train_score=None), b"null"), (dict(raw=None), b"null")):
        assert fit(**bad) == ERR_ARG and word in L.bbbp_last_error() and L.bbbp_last_error().startswith(b"gbr_fit: chain 0:"), bad
    assert L.bbbp_gbr_fit(None, None, 4096, 1) == ERR_ARG and L.bbbp_last_error() == b"gbr_fit: null pointer"
    assert L.bbbp_gbr_fit(None, ctypes.byref(_chain()), None, 1) == ERR_ARG and L.bbbp_last_error() == b"gbr_fit: null pointer"
    assert L.bbbp_gbr_fit(None, ctypes.byref(_chain()), 4096, 0) == ERR_ARG and b"gbr_fit: n_chains" in L.bbbp_last_error()
    two = (_lib.GbtChain * 2)(_chain(), _chain(max_depth=9))               # the second of a batch is examined too
    assert L.bbbp_gbr_fit(None, two, 4096, 2) == ERR_ARG and L.bbbp_last_error().startswith(b"gbr_fit: chain 1: max_depth 9")
    assert L.bbbp_gbt_fit(None, two, 4096, 2) == ERR_ARG and L.bbbp_last_error().startswith(b"gbt_fit: chain 1: max_depth 9")     # the classifier's prefix stays


def test_regressor_refusals():
    from bbbp_amd.gradient_boosting import GradientBoostingRegressor as GBR, fit_regressors, MAX_ROWS, MAX_FEATURES
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GBR(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GBR().fit(torch.zeros(8, 4), np.arange(8.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_regressors([(np.zeros((6, 2)), np.arange(6.0))], device="cpu")
    with pytest.raises(ValueError, match="no problems"):
        fit_regressors([])
    for kw, name in ((dict(loss="huber"), "loss"), (dict(loss="absolute_error"), "loss"), (dict(loss="quantile"), "loss"), (dict(alpha=0.5), "alpha"),
                     (dict(criterion="squared_error"), "criterion"), (dict(subsample=0.5), "subsample"), (dict(max_features="sqrt"), "max_features"),
                     (dict(max_features=3), "max_features"), (dict(init="zero"), "init"), (dict(init=object()), "init"), (dict(n_iter_no_change=5), "n_iter_no_change"),
                     (dict(max_leaf_nodes=8), "max_leaf_nodes"), (dict(ccp_alpha=0.01), "ccp_alpha"), (dict(min_impurity_decrease=0.1), "min_impurity_decrease"),
                     (dict(min_weight_fraction_leaf=0.1), "min_weight_fraction_leaf"), (dict(warm_start=True), "warm_start"), (dict(max_depth=8), "max_depth"),
                     (dict(max_depth=None), "max_depth"), (dict(max_depth=0), "max_depth"), (dict(max_depth=2.5), "max_depth"),
                     (dict(min_samples_split=0.5), "min_samples_split"), (dict(min_samples_split=1), "min_samples_split"), (dict(min_samples_leaf=0.1), "min_samples_leaf"),
                     (dict(min_samples_leaf=0), "min_samples_leaf"), (dict(n_estimators=0), "n_estimators"), (dict(n_estimators=2.5), "n_estimators"),
                     (dict(learning_rate=0.0), "learning_rate"), (dict(learning_rate=float("inf")), "learning_rate"), (dict(learning_rate="0.1"), "learning_rate"),
                     (dict(colsample=1), "colsample")):
        with pytest.raises((ValueError, NotImplementedError), match=name):
            GBR(**kw)
    GBR(200, learning_rate=0.1, max_depth=5, random_state=42, subsample=1.0, alpha=0.9, criterion="friedman_mse", init=None)      # the reference's call, and defaults spelled out
    GBR(verbose=2, tol=1e-3, validation_fraction=0.2)                       # accepted and ignored: none of them changes the model
    Xok, yok = np.zeros((6, 2)), np.arange(6.0)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        GBR().fit(Xok, yok, sample_weight=np.ones(6))
    with pytest.raises(NotImplementedError, match="more than one output"):
        GBR().fit(Xok, np.zeros((6, 2)))
    with pytest.raises(ValueError, match="rows"):
        GBR().fit(Xok, yok[:4])
    with pytest.raises(ValueError, match="numeric"):
        GBR().fit(Xok, ["a"] * 6)
    for bad in (np.nan, np.inf, -np.inf):
        ybad = yok.copy()
        ybad[2] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            GBR().fit(Xok, ybad)
    # (y - mean)^2 overflows; the mean overflows; y - mean overflows; and 1e150, whose square is finite but whose split score is not
    for big in (np.array([1e200, -1e200] * 3), np.full(6, 1.7e308), np.array([1.7e308, -1.7e308] * 3), np.array([1e150, -1e150] * 3),
                np.array([0.0] * 5 + [1.3e140])):
        with pytest.raises(ValueError, match="overflows float64"):
            GBR().fit(Xok, big)
    from bbbp_amd.gradient_boosting import _regression_targets, MAX_TARGET_SPREAD
    edge = np.full(2, 1e300)                                                # large targets close together pass: the limit is on |y - mean|
    assert MAX_TARGET_SPREAD == 1e140 and _regression_targets(np.array([1e139, -1e139]), 2, "t")[1] == 0.0 and _regression_targets(edge, 2, "t")[1] == 1e300
    for bad in (np.nan, np.inf, 1e39):                                     # 1e39 is finite in float64 and infinite in the float32 the trees compare
        Xbad = Xok.copy()
        Xbad[3, 1] = bad
        with pytest.raises(ValueError, match="NaN"):
            GBR().fit(Xbad, yok)
    with pytest.raises(ValueError, match="BBBP_GBT_FIT_MAX_N"):
        GBR().fit(np.zeros((MAX_ROWS + 1, 1)), np.zeros(MAX_ROWS + 1))
    with pytest.raises(ValueError, match="BBBP_GBT_FIT_MAX_D"):
        GBR().fit(np.zeros((4, MAX_FEATURES + 1)), np.zeros(4))
    with pytest.raises(ValueError, match="two rows"):
        GBR().fit(np.zeros((1, 2)), np.zeros(1))
    with pytest.raises(ValueError, match="2-D"):
        GBR().fit(np.zeros(6), yok)
    for method in ("predict", "predict_device"):
        with pytest.raises((RuntimeError, TypeError), match="not fitted|CUDA"):
            getattr(GBR(), method)(np.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="not fitted"):
        next(GBR().staged_predict(np.zeros((2, 4))))


def test_regressor_parameters_clone_and_set_params():
    from sklearn.base import clone
    from bbbp_amd.gradient_boosting import GradientBoostingRegressor as GBR
    lr, depth = np.float64(0.05), np.int64(5)
    reg = GBR(200, learning_rate=lr, max_depth=depth, min_samples_split=10, min_samples_leaf=3, random_state=42, device="cuda:0")
    assert reg.learning_rate is lr and reg.max_depth is depth                # kept as given, not cast
    params = reg.get_params()
    assert params == dict(n_estimators=200, learning_rate=lr, max_depth=depth, min_samples_split=10, min_samples_leaf=3, loss="squared_error",
                          random_state=42, device="cuda:0")
    twin = clone(reg)
    assert twin is not reg and twin.get_params() == params and not hasattr(twin, "trees_")
    assert all(type(twin.get_params()[k]) is type(v) for k, v in params.items())
    assert reg.set_params(n_estimators=50, max_depth=3) is reg and (reg.n_estimators, reg.max_depth, reg.min_samples_leaf) == (50, 3, 3)
    with pytest.raises(NotImplementedError, match="max_depth"):
        reg.set_params(max_depth=9)
    with pytest.raises(NotImplementedError, match="loss"):
        reg.set_params(loss="huber")
    with pytest.raises(ValueError, match="unknown"):
        reg.set_params(subsample=0.5)
    assert reg.max_depth == 3 and reg.loss == "squared_error"               # a refused set_params changes nothing
    reg.max_depth = None                                                    # as from_sklearn stores a limit that was not an int
    assert reg.set_params(n_estimators=7).n_estimators == 7                 # only what is being set is judged
    with pytest.raises(NotImplementedError, match="max_depth"):
        clone(reg)                                                          # a clone is an unfitted regressor with max_depth=None: refused
    assert GBR().get_params() == dict(n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, loss="squared_error",
                                      random_state=None, device="cuda")
