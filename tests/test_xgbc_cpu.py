"""``bbbp_amd.xgb.XGBClassifier`` without a GPU: the sigmoid, the hash and the draws; the numpy restatement (``tests/xgbc_numpy.py``) against
its own invariants and against scikit-learn's histogram booster; the host API."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xgbc_numpy as xc  # noqa: E402
from bbbp_amd.xgb import XGBClassifier  # noqa: E402,F401  (the restatement restates this class: without it nothing here has a subject)

EDGES = np.float32([0, -0.0, 1e-30, -1e-30, 17, -17, 87, -87, 88, -88, 1e9, -1e9])
KEYS = ("left", "right", "feature", "cond", "default_left", "root", "base_weights", "loss_changes", "sum_hessian", "parents")


def margins():
    rng = np.random.default_rng(0)
    return np.concatenate([rng.uniform(-110, 110, 700_000), rng.normal(0, 3, 300_000), EDGES]).astype(np.float32)


def small_problem(n=120, d=6, seed=3):
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, d)), 2).astype(np.float32)
    y = (X[:, 0] + np.sin(3 * X[:, 1]) + 0.3 * X[:, 2] * X[:, 3] + 0.4 * rng.normal(size=n) > 0).astype(np.int64)
    return X, y


# ---- 1. the sigmoid and the draws ---------------------------------------------------------------------------------------------------------
def test_sigmoid32_is_the_rounded_long_double_sigmoid_and_monotone():
    """Against the float32 rounding of an ``np.longdouble`` sigmoid of the clamped argument (x87 extended precision: 64-bit significand, so
    the float32 rounding of its result is the float32 rounding of the exact value except within 2^-40 of a tie, which no sample hits)."""
    x = margins()
    got = xc.sigmoid32(x)
    z = np.clip(x.astype(np.longdouble), -87, 87)
    want = (1 / (1 + np.exp(-z))).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.all(np.diff(xc.sigmoid32(np.sort(x))) >= 0)
    assert got.min() >= np.finfo(np.float32).tiny and got.max() <= 1 and xc.sigmoid32(np.float32(0)) == np.float32(0.5)
    assert xc.sigmoid32(np.float32(-88)) == xc.sigmoid32(np.float32(-87)) == xc.sigmoid32(np.float32(-1e9))


def test_package_sigmoid_and_hash_equal_the_restatement():
    from bbbp_amd import xgb
    x = margins()
    assert np.array_equal(xgb.sigmoid32(x).view(np.int32), xc.sigmoid32(x).view(np.int32))
    for seed in (0, 7, 2 ** 63 + 5, 2 ** 64 - 1):
        for stream in (0, 1):
            trees, i = np.arange(5)[:, None], np.arange(300)[None, :]
            got, want = xgb.sample_hash(seed, stream, trees, i), xc.draw(seed, stream, trees, i)
            assert got.dtype == np.uint64 and got.shape == (5, 300) and np.array_equal(got, want)
    assert np.array_equal(xgb.row_sample(3, 4, 500, 0.8), xc.row_sample(3, 4, 500, 0.8))
    cols = np.sort(np.random.default_rng(1).choice(400, 77, replace=False))
    masks = xgb.column_masks(3, 9, cols, 0.8)
    assert np.array_equal(masks, xc.column_masks(3, 9, cols, 0.8))
    packed = xgb._pack_masks(masks)
    assert packed.dtype == np.uint32 and packed.shape == (9, 3)
    assert np.array_equal((packed[:, np.arange(77) // 32] >> (np.arange(77) % 32).astype(np.uint32)) & 1, masks)
    # the hash by hand for one value: Python integers modulo 2^64
    M = 2 ** 64

    def mix(v):
        v ^= v >> 30; v = v * 0xBF58476D1CE4E5B9 % M
        v ^= v >> 27; v = v * 0x94D049BB133111EB % M
        return v ^ (v >> 31)
    assert int(xc.draw(42, 1, 3, 17)[0]) == mix((mix((mix((42 + 0x9E3779B97F4A7C15 * 2) % M) + 3) % M) + 17) % M)


def test_row_draw_share_and_column_draw_count():
    n, T = 8192, 50
    used = np.stack([xc.row_sample(0, t, n, 0.8) for t in range(T)])
    share, sd = used.mean(), np.sqrt(0.8 * 0.2 / (n * T))
    print(f"sampled share {share:.5f}, 0.8 +- 4 x {sd:.5f}")
    assert abs(share - 0.8) <= 4 * sd
    assert xc.row_sample(0, 0, n, 1.0).all() and not np.array_equal(used[0], used[1])
    assert np.array_equal(used[7], xc.row_sample(0, 7, n // 2, 0.8).tolist() + used[7][n // 2:].tolist()), "a row's draw depends on (tree, position) only"
    for d in (1, 2, 6, 50, 333):
        for c in (0.01, 0.5, 0.8, 0.999, 1.0):
            m = xc.column_masks(5, 12, np.arange(d) * 3, c)
            assert m.shape == (12, d) and np.all(m.sum(axis=1) == (d if c >= 1 else max(1, int(np.floor(c * d)))))
    a, b = xc.column_masks(5, 12, np.arange(50), 0.5), xc.column_masks(5, 24, np.arange(50), 0.5)
    assert np.array_equal(a, b[:12]) and len({tuple(r) for r in b}) > 12, "tree t's draw does not depend on n_estimators"


# ---- 2. the restatement's invariants ------------------------------------------------------------------------------------------------------------
def node_sums(model, X, y, tree):
    """Per node of ``tree``: its training rows, from the walk."""
    lo, hi = model["root"][tree], model["root"][tree + 1]
    rows = {lo: np.arange(len(X))}
    for node in range(lo, hi):
        if model["left"][node] >= 0:
            r = rows[node]
            go_left = X[r, model["feature"][node]] < model["cond"][node]
            rows[int(model["left"][node])], rows[int(model["right"][node])] = r[go_left], r[~go_left]
    return rows


@pytest.mark.parametrize("extra", [dict(), dict(gamma=0.5), dict(min_child_weight=3.0), dict(gamma=0.2, min_child_weight=2.5, reg_lambda=3.0),
                                   dict(subsample=0.8, colsample_bytree=0.8, random_state=5)])
def test_restatement_invariants(extra):
    X, y = small_problem()
    T = 4
    model = xc.fit(X, y, n_estimators=T, max_depth=5, **extra)
    inner = model["left"] >= 0
    gamma, mcw = extra.get("gamma", 0.0), extra.get("min_child_weight", 1.0)
    assert inner.any() and model["loss_changes"][inner].min() > 1e-6 and model["loss_changes"][inner].min() >= np.float32(gamma)
    assert np.all(model["loss_changes"][~inner] == 0)
    children = np.concatenate([model["left"][inner], model["right"][inner]])
    assert model["sum_hessian"][children].min() >= np.float32(mcw), "both children satisfy H >= min_child_weight"
    # a child's recorded hessian is the float32 rounding of an exact sum: parent = left + right up to those roundings
    H = model["sum_hessian"].astype(np.float64)
    assert np.allclose(H[model["left"][inner]] + H[model["right"][inner]], H[inner], rtol=3 * 2.0 ** -24, atol=0)
    # the recorded hessian of every node is the sum of p (1 - p) over its sampled rows, margins replayed from the model itself
    margin = np.full(len(X), model["base_margin"], np.float32)
    for t in range(T):
        p = xc.sigmoid32(margin)
        h = (p * (np.float32(1) - p)).astype(np.float64) * model["row_masks"][t]
        rows = node_sums(model, X, y, t)
        for node, r in rows.items():
            assert abs(h[r].sum() - H[node]) <= 1e-6 * max(1.0, H[node]), (t, node)
            if model["left"][node] >= 0:
                col = int(np.flatnonzero(model["live"] == model["feature"][node])[0])
                assert model["col_masks"][t, col], "no split names a masked column"
        margin = xc.predict_margin({**model, "root": model["root"][:t + 2]}, X)
    assert np.array_equal(margin.view(np.int32), model["train_margin"].view(np.int32))
    longer = xc.fit(X, y, n_estimators=2 * T, max_depth=5, **extra)
    for k in KEYS:
        assert np.array_equal(longer[k][:len(model[k])].view(np.uint8), model[k].view(np.uint8)), f"{k}: a T-tree fit is the prefix of a 2T-tree fit"


def test_initial_margin_and_unsampled_root():
    t = np.float32([0, 1, 1, 1])
    m0, p0 = xc.initial_margin(t)
    assert m0 == np.float32(1.0) and p0 == xc.sigmoid32(np.float32(1.0)) and p0.dtype == np.float32
    m0, p0 = xc.initial_margin(t, 0.25)
    assert m0 == np.float32(np.log(0.25 / 0.75)) and p0 == np.float32(0.25)
    X, y = small_problem(40, 4, seed=9)
    model = xc.fit(X, y, n_estimators=12, max_depth=4, subsample=0.02, reg_lambda=0.0, random_state=1)
    empty = np.flatnonzero(~model["row_masks"].any(axis=1))
    assert len(empty), "choose another seed: no tree of this problem is left without rows"
    for t in empty:                                       # a node that holds only unsampled rows: a leaf of -0.0 and sum_hessian 0
        node = model["root"][t]
        assert model["root"][t + 1] == node + 1 and model["left"][node] == -1 and model["sum_hessian"][node] == 0
        assert model["cond"][node:node + 1].view(np.int32)[0] == np.float32(-0.0).view(np.int32)
    assert np.isfinite(model["train_margin"]).all() and np.isfinite(model["cond"]).all()


# ---- 3. scikit-learn's histogram booster --------------------------------------------------------------------------------------------------
def sk_leaves(predictor, X):
    """(leaf node index, leaf value) per row from a fitted ``TreePredictor``'s node table (left when ``x <= num_threshold``)."""
    nodes = predictor.nodes
    at = np.zeros(len(X), np.int64)
    while not nodes["is_leaf"][at].all():
        inner = ~nodes["is_leaf"][at].astype(bool)
        go_left = X[np.arange(len(X)), nodes["feature_idx"][at]].astype(np.float64) <= nodes["num_threshold"][at]
        at = np.where(inner, np.where(go_left, nodes["left"][at], nodes["right"][at]), at)
    return at, nodes["value"][at]


def test_leaves_and_values_agree_with_sklearn_hist():
    """Same gradients, hessians, gain and leaf weight; 200 rows of continuous features, so every value has its own bin on both sides, and
    a tie-free problem, so the best split is the same one.  Both trees part the training rows into the same leaves, and the leaf values
    agree to ``rtol = 1e-5``: scikit-learn keeps margins in float64 and rounds g and h to float32, the restatement keeps margins in float32,
    scikit-learn adds 1e-15 to the denominator -- a few float32 roundings, 6e-8 each, against a tolerance of 1e-5.  No private rule of
    scikit-learn's stands in the way at this shape: ``min_hessian_to_split = 1e-3`` and ``min_samples_leaf = 1`` bind nowhere (every leaf's
    hessian sum is checked to exceed 1e-3 below), ``max_leaf_nodes = 31`` exceeds the 8 leaves of depth 3."""
    from sklearn.ensemble import HistGradientBoostingClassifier
    rng = np.random.default_rng(12)
    n, d, eta = 200, 5, 0.3
    X = rng.standard_normal((n, d)).astype(np.float32)
    y = (X[:, 0] - 0.8 * X[:, 1] * X[:, 2] + 0.5 * rng.standard_normal(n) > 0.2).astype(np.int64)
    sk = HistGradientBoostingClassifier(max_iter=2, max_depth=3, learning_rate=eta, l2_regularization=1.0, min_samples_leaf=1, early_stopping=False).fit(X, y)
    model = xc.fit(X, y, n_estimators=2, max_depth=3, learning_rate=eta, reg_lambda=1.0, min_child_weight=0.0, base_score=float(np.mean(y)))
    assert abs(float(model["base_margin"]) - float(sk._baseline_prediction.ravel()[0])) <= 1e-6
    for t in range(2):
        sk_leaf, sk_value = sk_leaves(sk._predictors[t][0], X)
        rows = node_sums(model, X, y, t)
        ours = np.full(n, -1)
        for node, r in rows.items():
            if model["left"][node] < 0:
                ours[r] = node
                assert model["sum_hessian"][node] > 1e-3
        assert (ours >= 0).all()
        pairs = {(int(a), int(b)) for a, b in zip(ours, sk_leaf)}
        assert len(pairs) == len(set(ours)) == len(set(sk_leaf)), f"tree {t}: the rows are parted into other leaves"
        err = np.abs(model["cond"][ours].astype(np.float64) - sk_value) / np.abs(sk_value)
        print(f"tree {t}: {len(pairs)} leaves, largest relative difference of a leaf value {err.max():.2e}")
        assert np.allclose(model["cond"][ours].astype(np.float64), sk_value, rtol=1e-5, atol=0)


# ---- 4. host API -------------------------------------------------------------------------------------------------------------------------------
def test_constructor_aliases_and_refusals_by_name():
    from bbbp_amd import xgb
    C = xgb.XGBClassifier
    ref = C(use_label_encoder=False, eval_metric="logloss", learning_rate=0.02, n_estimators=500, max_depth=7, colsample_bytree=0.8, subsample=0.8,
            reg_lambda=3, tree_method="hist", device="cuda")
    assert (ref.learning_rate, ref.n_estimators, ref.max_depth, ref.colsample_bytree, ref.subsample, ref.reg_lambda) == (0.02, 500, 7, 0.8, 0.8, 3)
    al = C(eta=0.05, min_split_loss=0.5, **{"lambda": 2.0})
    assert (al.learning_rate, al.gamma, al.reg_lambda) == (0.05, 0.5, 2.0)
    C(objective="binary:logistic", eval_metric=None, scale_pos_weight=1, colsample_bylevel=1.0, colsample_bynode=1, subsample=1, random_state=7, n_jobs=4,
      base_score=0.3, min_child_weight=0, verbosity=0)
    for kw, name in [(dict(objective="reg:squarederror"), "objective"), (dict(objective="multi:softprob"), "objective"), (dict(eval_metric="auc"), "eval_metric"),
                     (dict(scale_pos_weight=2.0), "scale_pos_weight"), (dict(colsample_bylevel=0.5), "colsample_bylevel"),
                     (dict(colsample_bynode=0.5), "colsample_bynode"), (dict(reg_alpha=0.1), "reg_alpha"), (dict(max_delta_step=1), "max_delta_step"),
                     (dict(grow_policy="lossguide"), "grow_policy"), (dict(max_leaves=8), "max_leaves"), (dict(tree_method="exact"), "tree_method"),
                     (dict(early_stopping_rounds=5), "early_stopping_rounds"), (dict(monotone_constraints="(1,0)"), "monotone_constraints"),
                     (dict(enable_categorical=True), "enable_categorical"), (dict(max_depth=0), "max_depth"), (dict(n_estimators=10001), "10000 trees"),
                     (dict(max_bin=257), "max_bin"), (dict(device=["cuda:0", "cuda:1"]), "more than one GPU"), (dict(booster="gblinear"), "booster"),
                     (dict(num_parallel_tree=2), "num_parallel_tree"), (dict(sampling_method="gradient_based"), "sampling_method"),
                     (dict(random_state=np.random.RandomState(0)), "random_state")]:
        with pytest.raises(NotImplementedError, match=name):
            C(**kw)
    for kw, name in [(dict(learning_rate=0), "learning_rate"), (dict(reg_lambda=-1), "reg_lambda"), (dict(gamma=float("nan")), "gamma"),
                     (dict(min_child_weight=-1), "min_child_weight"), (dict(n_estimators=0), "n_estimators"), (dict(subsample=0), "subsample"),
                     (dict(subsample=1.5), "subsample"), (dict(colsample_bytree=0.0), "colsample_bytree"), (dict(colsample_bytree=2), "colsample_bytree"),
                     (dict(base_score=0.0), "base_score"), (dict(base_score=1.0), "base_score"), (dict(base_score=-0.5), "base_score"),
                     (dict(colsample=1), "unknown parameter colsample")]:
        with pytest.raises(ValueError, match=name):
            C(**kw)
    X, y = small_problem(20, 4)
    clf = C()
    with pytest.raises(NotImplementedError, match="sample_weight"):
        clf.fit(X, y, sample_weight=np.ones(20))
    with pytest.raises(NotImplementedError, match="eval_set"):
        clf.fit(X, y, eval_set=[(X, y)])
    with pytest.raises(NotImplementedError, match="early stopping"):
        clf.fit(X, y, early_stopping_rounds=3)
    with pytest.raises(ValueError, match="exactly two classes"):
        clf.fit(X, np.arange(20) % 3)
    with pytest.raises(ValueError, match="exactly two classes"):
        clf.fit(X, np.ones(20))
    with pytest.raises(NotImplementedError, match="8192"):
        clf.fit(np.zeros((8193, 2), np.float32), np.arange(8193) % 2)
    bad = X.copy(); bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        clf.fit(bad, y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C(device="cpu").fit(X, y)
    with pytest.raises(RuntimeError, match="not fitted"):
        clf.predict_proba(X)
    with pytest.raises(RuntimeError, match="no CPU path"):
        xgb.randomized_search_cv(X, y, dict(n_estimators=[2, 3]), n_iter=2, cv=2, device="cpu")
    with pytest.raises(NotImplementedError, match="max_leaves"):
        xgb.randomized_search_cv(X, y, dict(max_leaves=[2, 3]), n_iter=2, cv=2)


def test_params_and_clone():
    from sklearn.base import clone
    from bbbp_amd import xgb
    clf = xgb.XGBClassifier(eta=0.05, n_estimators=7, subsample=0.8, colsample_bytree=0.5, random_state=3, eval_metric="logloss", use_label_encoder=False)
    twin = clone(clf)
    assert twin is not clf and twin.get_params() == clf.get_params()
    assert clf.set_params(eta=0.1, max_depth=3, subsample=0.9) is clf and (clf.learning_rate, clf.max_depth, clf.subsample) == (0.1, 3, 0.9)
    with pytest.raises(ValueError, match="subsample"):
        clf.set_params(subsample=0)
    with pytest.raises(ValueError, match="unknown"):
        clf.set_params(depth=3)
    assert clf.subsample == 0.9
    assert xgb.XGBClassifier().get_params() == dict(n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0,
                                                    max_bin=256, base_score=None, subsample=1.0, colsample_bytree=1.0, tree_method="hist",
                                                    random_state=None, n_jobs=None, device="cuda")


def test_model_json_round_trip():
    from bbbp_amd import boosters, xgb
    X, y = small_problem(60, 5)
    model = xc.fit(X, y, n_estimators=4, max_depth=3, subsample=0.8, random_state=2)
    clf = xgb.XGBClassifier.from_trees({k: model[k] for k in KEYS}, model["base_score"], X.shape[1], classes=model["classes"], device="cpu", n_estimators=4)
    assert clf.base_score_ == model["base_score"] and abs(float(clf.base_margin_) - float(model["base_margin"])) <= 1e-6
    text = clf.get_model_json()
    doc = json.loads(text)
    assert doc["learner"]["objective"]["name"] == "binary:logistic" and doc["learner"]["learner_model_param"]["num_class"] == "0"
    assert np.float32(float(doc["learner"]["learner_model_param"]["base_score"])) == model["base_score"]
    for source in (text, text.encode("utf-8"), doc):
        back = xgb.XGBClassifier.from_model_json(source, classes=model["classes"], device="cpu")
        for k in KEYS:
            assert back.trees_[k].dtype == model[k].dtype and np.array_equal(back.trees_[k].view(np.uint8), model[k].view(np.uint8)), k
        assert back.base_score_ == clf.base_score_ and back.base_margin_ == clf.base_margin_ and back.n_features_in_ == 5 and back.n_estimators == 4
    with pytest.raises(ValueError, match="objective"):
        boosters.XGBTrees.from_raw(text.encode("utf-8"), device="cpu")              # the regression loader keeps refusing other objectives
    with pytest.raises(ValueError, match="binary:logistic"):
        xgb.XGBClassifier.from_model_json(text.replace("binary:logistic", "reg:squarederror"))
    with pytest.raises(RuntimeError, match="GPU"):
        clf.predict_proba(X)
