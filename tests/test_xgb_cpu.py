"""``bbbp_amd.xgb`` without a GPU: the numpy restatement (``tests/xgb_numpy.py``) against XGBoost's own recorded statistics, against
scikit-learn's histogram booster, against exact rational arithmetic on tiny problems; the quantisation; the host API."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xgb_numpy as xn  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24                              # the relative error of one rounding to float32


# ---- 1. XGBoost's own output: the statistics of the model the reference ships --------------------------------------------------------------
def shipped():
    head, stats = np.load(os.path.join(GOLDEN, "xgb_maccs_head.npz")), np.load(os.path.join(GOLDEN, "xgb_maccs_stats.npz"))
    return head["left"].astype(np.int64), head["right"].astype(np.int64), head["root"].astype(np.int64), head["cond"], {k: stats[k] for k in stats.files}


def test_recorded_gains_follow_from_recorded_weights_and_hessians():
    """``G = -w (H + lambda)`` from the stored weights (a leaf's is its value / float32(0.01)), then ``gain`` must give every ``loss_changes``.

    The tolerance, from the float32 rounding of the three stored fields.  ``sum_hessian`` is a row count: exact.  A stored weight is
    XGBoost's weight rounded to float32 (relative error u = 2^-24); a leaf's went through one more float32 product with the rate, and the
    division by float32(0.01) here is done in float64: 2 u at most.  So each recovered G is off by 2 u relatively, each ``term = G^2 / (H +
    lambda)`` by 4 u, and the gain, a sum and difference of three terms, by 4 u (term_L + term_R + term_P) absolutely -- the gain itself
    can be orders of magnitude below the terms, which is why a relative bound on the gain means nothing.  ``loss_changes`` is the gain
    rounded to float32: u |gain| more.  float64 rounding in ``gain`` is 2^-29 of that and left out."""
    left, right, root, cond, s = shipped()
    assert len(s["parents"]) == len(left) == root[-1]
    w, H, recorded = s["base_weights"].astype(np.float64), s["sum_hessian"].astype(np.float64), s["loss_changes"].astype(np.float64)
    leaf = left < 0
    assert np.array_equal(s["base_weights"][leaf], cond[leaf]), "a leaf's base_weights is its scaled value"
    G = -np.where(leaf, w / np.float64(np.float32(0.01)), w) * (H + 1.0)
    i = np.flatnonzero(~leaf)
    l, r = left[i], right[i]
    got = xn.gain(G[l], H[l], G[r], H[r], G[i], H[i], 1.0)
    tol = 4 * U32 * (xn.term(G[l], H[l], 1.0) + xn.term(G[r], H[r], 1.0) + xn.term(G[i], H[i], 1.0)) + U32 * np.abs(recorded[i])
    err = np.abs(got - recorded[i])
    print(f"gain identity on {len(i)} splits: largest error / tolerance {np.max(err / tol):.3f}, "
          f"largest |gain - recorded| / max(|gain|, 1e-3) {np.max(err / np.maximum(np.abs(got), 1e-3)):.2e}")
    assert np.all(err <= tol)
    assert np.array_equal(xn.weight(G, H, 1.0)[~leaf].astype(np.float32), s["base_weights"][~leaf])
    assert np.all(recorded[leaf] == 0)


def test_recorded_hessians_and_stop_rule():
    left, right, root, _, s = shipped()
    H, i = s["sum_hessian"].astype(np.float64), np.flatnonzero(left >= 0)
    assert np.array_equal(H[left[i]] + H[right[i]], H[i]), "children's sum_hessian add to the parent's exactly"
    assert H.min() >= 1 and np.array_equal(H, np.round(H))
    assert s["loss_changes"][i].min() > 1e-6, "every recorded split clears kRtEps"


def test_recorded_node_ids_are_breadth_first():
    """The numbering rule of the module docstring: the root is 0, nodes are expanded in ascending id, each split appends its two children
    as the next two ids -- and ``parents`` says the same."""
    left, right, root, _, s = shipped()
    for t in range(len(root) - 1):
        lo, hi = root[t], root[t + 1]
        nxt = 1
        assert s["parents"][lo] == 2147483647
        for node in range(hi - lo):
            if left[lo + node] >= 0:
                assert (left[lo + node] - lo, right[lo + node] - lo) == (nxt, nxt + 1), f"tree {t} node {node}"
                assert s["parents"][lo + nxt] == node and s["parents"][lo + nxt + 1] == node
                nxt += 2
        assert nxt == hi - lo


# ---- 2. scikit-learn's histogram booster --------------------------------------------------------------------------------------------------
def sk_data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    y = 1.5 * X[:, 0] + np.sin(3 * X[:, 1]) + 0.3 * X[:, 2] * X[:, 3] + 0.1 * rng.standard_normal(n)
    return X, y


@pytest.mark.parametrize("n,d,T,D,eta", [(200, 12, 20, 4, 0.3), (250, 8, 30, 6, 0.1), (255, 6, 10, 3, 0.5)])
def test_training_predictions_agree_with_sklearn_hist(n, d, T, D, eta):
    """Same gain, same leaf weight; with at most 255 rows of continuous features every value has its own bin on both sides, so the partitions
    agree (shallow trees only: on tiny nodes scikit-learn's ``min_hessian_to_split`` and stop rule differ from XGBoost's).

    The bound, from T float32 roundings of the margin.  scikit-learn keeps float64 throughout; the restatement rounds y to float32 once,
    and per tree rounds g = margin - y, the leaf's value and the sum margin + value to float32: four roundings of numbers no larger than
    M = max(|y|, |margin|), half an ulp of M each.  A leaf's weight is an average of its rows' g shrunk by m / (m + lambda) and by the rate,
    so an error already in the margins comes back smaller, not larger: to first order the errors add, 2 ulp(M) per tree and 2 T ulp(M)
    after T trees."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    X, y = sk_data(n, d)
    sk = HistGradientBoostingRegressor(loss="squared_error", l2_regularization=1.0, max_bins=255, min_samples_leaf=1, max_leaf_nodes=None, max_depth=D,
                                       learning_rate=eta, max_iter=T, early_stopping=False).fit(X, y)
    model = xn.fit(X, y, n_estimators=T, max_depth=D, learning_rate=eta)
    want, got = sk.predict(X), model["train_margin"].astype(np.float64)
    bound = 2 * T * float(np.spacing(np.float32(max(np.abs(y).max(), np.abs(got).max()))))
    err = np.abs(got - want).max()
    print(f"({n}, {d}, {T}, {D}, {eta}): max |restatement - scikit-learn| on the training rows {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- 3. exhaustive check on tiny problems, in exact rationals -----------------------------------------------------------------------------------
def exact_gain(q_l, m_l, Q, m, lam):
    term = lambda q, h: Fraction(q) ** 2 / (Fraction(h) + lam)  # noqa: E731  (the common factor 4^-k is left out: it does not change an order)
    return term(q_l, m_l) + term(Q - q_l, m - m_l) - term(Q, m)


@pytest.mark.parametrize("seed", range(12))
def test_every_split_is_the_best_and_every_leaf_has_none(seed):
    rng = np.random.default_rng(seed)
    n, d = int(rng.integers(2, 13)), int(rng.integers(1, 4))
    X = rng.integers(0, 4, size=(n, d)).astype(np.float32)
    y = rng.integers(-8, 9, size=n) / 4.0
    lam, gamma, mcw, depth = [(1.0, 0.0, 1.0, 4), (0.0, 0.0, 1.0, 3), (2.5, 0.25, 2.0, 4)][seed % 3]
    model = xn.fit(X, y, n_estimators=1, max_depth=depth, reg_lambda=lam, gamma=gamma, min_child_weight=mcw, base_score=0.125)
    live, cc, B = xn.quantise(X)
    k, q = xn.quantise_gradients(np.float32(0.125) - y.astype(np.float32))
    lam_q, scale = Fraction(lam), Fraction(4) ** k
    rows_of, depth_of = {0: np.arange(n)}, {0: 0}
    for node in range(len(model["left"])):
        rows, m = rows_of[node], len(rows_of[node])
        Q = int(q[rows].sum())
        assert model["sum_hessian"][node] == m
        cands = []                                                    # every (feature, boundary) pair, the tie rule's order
        for f in range(len(live)):
            for b in range(len(cc[f])):
                m_l = int((B[f, rows] <= b).sum())
                if m_l >= max(1, mcw) and m - m_l >= max(1, mcw):
                    q_l = int(q[rows][B[f, rows] <= b].sum())
                    cands.append((exact_gain(q_l, m_l, Q, m, lam_q) / scale, f, b))
        admissible = [c for c in cands if c[0] > Fraction(1e-6) and c[0] >= Fraction(gamma)] if depth_of[node] < depth else []
        if model["left"][node] < 0:
            assert not admissible, f"leaf {node} has an admissible split {admissible[0]}"
            want = np.float32(np.float64(np.float32(0.3)) * float(-Fraction(Q, 2 ** k) / (m + lam_q)))
            assert abs(float(model["cond"][node]) - float(want)) <= abs(float(want)) * 2 * U32
            continue
        best = max(c[0] for c in cands)
        first = min((c[1], c[2]) for c in cands if c[0] == best)
        f, b = first
        assert admissible and model["feature"][node] == live[f] and model["cond"][node] == cc[f][b], f"node {node}: not the best split under the tie rule"
        assert abs(float(model["loss_changes"][node]) - float(best)) <= float(best) * 2 * U32
        go_left = B[f, rows] <= b
        assert np.array_equal(X[rows, live[f]] < model["cond"][node], go_left)
        rows_of[int(model["left"][node])], rows_of[int(model["right"][node])] = rows[go_left], rows[~go_left]
        depth_of[int(model["left"][node])] = depth_of[int(model["right"][node])] = depth_of[node] + 1
    assert len(rows_of) == len(model["left"])


# ---- 4. quantisation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_bin", [2, 16, 256])
def test_cuts_and_bins(max_bin):
    rng = np.random.default_rng(max_bin)
    n = 600
    for distinct in (1, 2, max_bin, max_bin + 1, n):
        col = rng.permutation(np.resize(np.round(rng.standard_normal(distinct), 4).astype(np.float32) if distinct < n else
                                        rng.standard_normal(n).astype(np.float32), n))
        k = len(np.unique(col))
        c = xn.cuts(col, max_bin)
        b = xn.bins(col, c)
        assert np.all(np.diff(c) > 0) and len(c) <= max_bin - 1 and b.dtype == np.uint8 and b.max(initial=0) <= len(c)
        if k <= max_bin:
            assert np.array_equal(c, np.unique(col)[1:]), "all distinct values above the minimum"
            assert np.array_equal(b, np.searchsorted(np.unique(col), col)), "every value has its own bin"
        else:
            s = np.sort(col)
            assert set(c) <= {s[(j * n) // max_bin] for j in range(1, max_bin)} and c.min() > s[0]
        assert (len(c) == 0) == (k == 1), "only a constant column has no cut"
        for split_bin in range(len(c)):                              # x < split_condition <=> bin <= split bin, for every training value
            assert np.array_equal(col < c[split_bin], b <= split_bin)
        order = np.argsort(col, kind="stable")
        assert np.all(np.diff(b[order].astype(int)) >= 0), "bins rise with the value"


def test_duplicates_and_constant_columns():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((80, 5)).astype(np.float32)
    X[:, 1], X[:, 3] = 2.5, -0.0
    X[40:, 0] = X[:40, 0]                                            # every value twice
    y = X[:, 0] + X[:, 2] * X[:, 4]
    live, cc, B = xn.quantise(X)
    assert list(live) == [0, 2, 4] and len(cc[0]) == 39 and B.shape == (3, 80)
    model = xn.fit(X, y, n_estimators=5, max_depth=30)
    assert not np.isin(model["feature"][model["left"] >= 0], [1, 3]).any(), "constant columns never appear in a tree"
    assert np.array_equal(xn.predict(model, X).view(np.int32), model["train_margin"].view(np.int32))
    assert np.array_equal(xn.cuts(np.float32([-0.0, 0.0, 1.0, -1.0])).view(np.int32), np.float32([0.0, 1.0]).view(np.int32))


# ---- 5. host API ----------------------------------------------------------------------------------------------------------------------------------
def small_model():
    X, y = sk_data(60, 5, seed=3)
    return X, y, xn.fit(X, y, n_estimators=4, max_depth=3)


def test_refusals_by_name():
    from bbbp_amd import xgb
    R = xgb.XGBRegressor
    for kw, name in [(dict(objective="reg:absoluteerror"), "objective"), (dict(subsample=0.8), "subsample"), (dict(colsample_bytree=0.5), "colsample_bytree"),
                     (dict(colsample_bylevel=0.5), "colsample_bylevel"), (dict(colsample_bynode=0.5), "colsample_bynode"), (dict(reg_alpha=0.1), "reg_alpha"),
                     (dict(max_delta_step=1), "max_delta_step"), (dict(grow_policy="lossguide"), "grow_policy"), (dict(max_leaves=8), "max_leaves"),
                     (dict(tree_method="exact"), "tree_method"), (dict(tree_method="approx"), "tree_method"), (dict(early_stopping_rounds=5), "early_stopping_rounds"),
                     (dict(monotone_constraints="(1,0)"), "monotone_constraints"), (dict(interaction_constraints=[[0, 1]]), "interaction_constraints"),
                     (dict(enable_categorical=True), "enable_categorical"), (dict(feature_types=["c"]), "feature_types"), (dict(max_depth=0), "max_depth"),
                     (dict(max_depth=1025), "max_depth"), (dict(max_depth=None), "max_depth"), (dict(n_estimators=10001), "10000 trees"),
                     (dict(max_bin=257), "max_bin"), (dict(max_bin=1), "max_bin"), (dict(device=["cuda:0", "cuda:1"]), "more than one GPU"),
                     (dict(booster="gblinear"), "booster"), (dict(num_parallel_tree=2), "num_parallel_tree")]:
        with pytest.raises(NotImplementedError, match=name):
            R(**kw)
    for kw, name in [(dict(learning_rate=0), "learning_rate"), (dict(reg_lambda=-1), "reg_lambda"), (dict(gamma=float("nan")), "gamma"),
                     (dict(min_child_weight=-1), "min_child_weight"), (dict(n_estimators=0), "n_estimators"), (dict(colsample=1), "unknown parameter colsample")]:
        with pytest.raises(ValueError, match=name):
            R(**kw)
    R(objective="reg:squarederror", subsample=1, colsample_bytree=1.0, reg_alpha=0, max_leaves=0, grow_policy="depthwise", tree_method="auto", random_state=7,
      n_jobs=4, verbosity=0, monotone_constraints=None, enable_categorical=False)          # the neutral values pass
    X, y = sk_data(20, 4)
    reg = R()
    with pytest.raises(NotImplementedError, match="sample_weight"):
        reg.fit(X, y, sample_weight=np.ones(20))
    with pytest.raises(NotImplementedError, match="eval_set"):
        reg.fit(X, y, eval_set=[(X, y)])
    with pytest.raises(NotImplementedError, match="early stopping"):
        reg.fit(X, y, early_stopping_rounds=3)
    with pytest.raises(NotImplementedError, match="8192"):
        reg.fit(np.zeros((8193, 2), np.float32), np.zeros(8193))
    with pytest.raises(NotImplementedError, match="live features"):
        reg.fit(np.arange(2 * 65537, dtype=np.float32).reshape(2, 65537), np.zeros(2))
    bad = X.copy(); bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        reg.fit(bad, y)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        reg.fit(bad, y)
    with pytest.raises(ValueError, match="NaN or infinity"):
        reg.fit(X, np.where(np.arange(20) == 2, np.nan, y))
    with pytest.raises(NotImplementedError, match="one output"):
        reg.fit(X, np.stack([y, y], axis=1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R(device="cpu").fit(X, y)
    with pytest.raises(RuntimeError, match="not fitted"):
        reg.predict(X)


def test_params_clone_and_aliases():
    from sklearn.base import clone
    from bbbp_amd import xgb
    reg = xgb.XGBRegressor(eta=0.05, min_split_loss=0.5, n_estimators=7, random_state=3, n_jobs=2, **{"lambda": 2.0})
    assert (reg.learning_rate, reg.gamma, reg.reg_lambda) == (0.05, 0.5, 2.0)
    twin = clone(reg)
    assert twin is not reg and twin.get_params() == reg.get_params() and set(reg.get_params()) >= {"n_estimators", "max_depth", "learning_rate", "device"}
    assert reg.set_params(eta=0.1, max_depth=3) is reg and (reg.learning_rate, reg.max_depth) == (0.1, 3)
    with pytest.raises(NotImplementedError, match="max_depth"):
        reg.set_params(max_depth=0)
    with pytest.raises(ValueError, match="unknown"):
        reg.set_params(depth=3)
    assert xgb.XGBRegressor().get_params() == dict(n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0,
                                                   max_bin=256, base_score=None, tree_method="hist", random_state=None, n_jobs=None, device="cuda")


def test_model_json_round_trip_and_validation():
    from bbbp_amd import boosters, xgb
    X, y, model = small_model()
    keys = ("left", "right", "feature", "cond", "default_left", "root", "base_weights", "loss_changes", "sum_hessian", "parents")
    reg = xgb.XGBRegressor.from_trees({k: model[k] for k in keys}, model["base_score"], X.shape[1], device="cpu", n_estimators=4, max_depth=3)
    assert boosters.validate_gbt(*(model[k] for k in keys[:6]), X.shape[1]) == reg.booster_.max_depth <= 3
    text = reg.get_model_json()
    back = boosters.XGBTrees.from_raw(text.encode("utf-8"), device="cpu")
    for k in ("left", "right", "feature", "cond", "default_left", "root"):
        assert back.arrays[k].dtype == reg.booster_.arrays[k].dtype and np.array_equal(back.arrays[k].view(np.uint8), reg.booster_.arrays[k].view(np.uint8)), k
    assert back.base_score == float(model["base_score"]) and back.n_features == X.shape[1] and back.n_trees == 4
    doc = json.loads(text)
    trees = doc["learner"]["gradient_booster"]["model"]["trees"]
    shipped_keys = {"base_weights", "categories", "categories_nodes", "categories_segments", "categories_sizes", "default_left", "id", "left_children",
                    "loss_changes", "parents", "right_children", "split_conditions", "split_indices", "split_type", "sum_hessian", "tree_param"}
    assert set(trees[0]) == shipped_keys and trees[0]["parents"][0] == 2147483647 and trees[1]["left_children"][0] in (1, -1)
    assert doc["learner"]["learner_model_param"]["num_feature"] == str(X.shape[1]) and doc["learner"]["objective"]["name"] == "reg:squarederror"
    for t, tree in enumerate(trees):
        lo, hi = model["root"][t], model["root"][t + 1]
        for key, name in (("base_weights", "base_weights"), ("loss_changes", "loss_changes"), ("sum_hessian", "sum_hessian"), ("cond", "split_conditions")):
            assert np.array_equal(np.asarray(tree[name], np.float32).view(np.int32), model[key][lo:hi].view(np.int32)), name
        assert int(tree["tree_param"]["num_nodes"]) == hi - lo
    derived = xgb.XGBRegressor.from_trees({k: model[k] for k in keys[:9]}, model["base_score"], X.shape[1], device="cpu")
    assert np.array_equal(derived.trees_["parents"], model["parents"])
    with pytest.raises(RuntimeError, match="GPU"):
        reg.predict(X)
