"""``bbbp_amd.xgb.XGBClassifier`` on the GPU against its numpy restatement (``tests/xgbc_numpy.py``), bit for bit: every node array, every
recorded statistic, the training margins, the initial margin and the base score; then the variants, the draws, saturation, prediction,
batch invariance, the stack and the search.

The shapes are the smallest at which the kernels can go wrong: the smallest problems, nodes on either side of the 64-row boundary between
the lane-against-lane form and the histogram form (64 and 65 rows at the root, both forms inside one deep tree), more feature blocks than
one, dropped constant columns (index remapping), the quantile rule (more distinct values than bins) and max_bin = 2."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xgbc_numpy as xc  # noqa: E402

pytestmark = pytest.mark.gpu

STATS = ("base_weights", "loss_changes", "sum_hessian")
KEYS = ("left", "right", "feature", "root", "parents", "default_left", "cond") + STATS


def data(n, d, seed):
    """Features rounded to two decimals (duplicates and ties on purpose), labels that need several columns and carry noise."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, d)), 2).astype(np.float32)
    s = 1.5 * X[:, 0] + np.sin(3 * X[:, 1 % d]) + 0.3 * X[:, 2 % d] * X[:, 3 % d] + 0.5 * rng.normal(size=n)
    y = (s > 0).astype(np.int64)
    y[:2] = [0, 1]                                            # both classes whatever n is
    return X, y


def mixed_data(n=1058, seed=11):
    """``tests/test_gpu_xgb.py``'s mixed matrix -- 120 binary columns, 60 constant ones and 120 of 5-40 distinct values, interleaved -- with
    its target thresholded at the median."""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(300):
        kind = j % 5
        if kind in (0, 1):
            cols.append((rng.random(n) < 0.3).astype(np.float32))
        elif kind == 2:
            cols.append(np.full(n, np.float32(j % 7)))
        else:
            cols.append(rng.integers(0, 5 + (j * 7) % 36, size=n).astype(np.float32) / 4)
    X = np.stack(cols, axis=1)
    s = X[:, 0] - X[:, 5] + 0.5 * X[:, 3] * X[:, 8] + 0.2 * X[:, 13] + 0.1 * rng.normal(size=n)
    return X, (s > np.median(s)).astype(np.int64)


#            n, d, trees, depth, max_bin, eta, further parameters
CASES = {
    "n2": (2, 1, 3, 1, 256, 0.3, dict(min_child_weight=0)), "n3": (3, 5, 4, 30, 256, 0.3, dict(min_child_weight=0)),
    "n64": (64, 7, 5, 30, 256, 0.3, dict(min_child_weight=0)), "n65": (65, 7, 5, 30, 256, 0.3, dict(min_child_weight=0)),
    "n300": (300, 20, 1, 30, 256, 0.3, dict(min_child_weight=0)), "n257_bin16": (257, 9, 5, 5, 16, 0.3, dict()),
    "n600_bin2": (600, 4, 4, 8, 2, 0.3, dict()), "n1058_mixed": (1058, 300, 3, 30, 256, 0.1, dict()),
}


@functools.lru_cache(maxsize=None)
def case(name):
    n, d, T, depth, max_bin, eta, extra = CASES[name]
    X, y = mixed_data(n) if name == "n1058_mixed" else data(n, d, seed=n + d)
    params = dict(n_estimators=T, max_depth=depth, max_bin=max_bin, learning_rate=eta, **extra)
    return X, y, params, xc.fit(X, y, **params)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_model(clf, ref, what=""):
    for key in KEYS:
        got, want = np.asarray(clf.trees_[key]), np.asarray(ref[key])
        assert got.shape == want.shape, f"{what}{key}: {got.shape} nodes, the restatement has {want.shape}"
        assert got.dtype == want.dtype, f"{what}{key}: dtype {got.dtype} != {want.dtype}"
        assert np.array_equal(bits(got), bits(want)), f"{what}{key}: first difference at node {int(np.flatnonzero(bits(got) != bits(want))[0])}"
    assert np.float32(clf.base_score_).tobytes() == np.float32(ref["base_score"]).tobytes(), f"{what}base_score"
    assert np.float32(clf.base_margin_).tobytes() == np.float32(ref["base_margin"]).tobytes(), f"{what}base_margin"
    assert clf.train_margin_.dtype == np.float32 and np.array_equal(bits(clf.train_margin_), bits(ref["train_margin"])), f"{what}train_margin_"
    assert np.array_equal(clf.classes_, ref["classes"]), f"{what}classes_"


def as_ref(clf):
    return {**clf.trees_, "base_score": clf.base_score_, "base_margin": clf.base_margin_, "train_margin": clf.train_margin_, "classes": clf.classes_}


def fit(dev, X, y, **params):
    from bbbp_amd import xgb
    return xgb.XGBClassifier(device=dev, **params).fit(X, y)


@pytest.mark.parametrize("name", list(CASES))
def test_fit_equals_the_restatement_bit_for_bit(dev, name):
    X, y, params, ref = case(name)
    clf = fit(dev, X, y, **params)
    assert_same_model(clf, ref)
    assert clf.n_features_in_ == X.shape[1] and len(ref["left"]) > params["n_estimators"], "the case grows trees"
    if name == "n300":                        # both forms in one tree, and a tree that grows until rows are alone
        leaf = ref["left"] < 0
        rows = np.zeros(len(leaf), np.int64)                   # row counts per node, from the walk
        for node, r in node_rows(ref, X, 0).items():
            rows[node] = len(r)
        assert (rows[~leaf] > 64).any() and (rows[~leaf] <= 64).any() and (rows[leaf] == 1).any()
    if name == "n1058_mixed":                 # constant columns never split, features keep their original indices
        used = np.unique(ref["feature"][ref["left"] >= 0])
        assert not np.isin(used % 5, [2]).any() and used.max() > 240


def node_rows(model, X, tree):
    lo, hi = model["root"][tree], model["root"][tree + 1]
    rows = {int(lo): np.arange(len(X))}
    for node in range(lo, hi):
        if model["left"][node] >= 0:
            r = rows[node]
            go_left = X[r, model["feature"][node]] < model["cond"][node]
            rows[int(model["left"][node])], rows[int(model["right"][node])] = r[go_left], r[~go_left]
    return rows


def variant_data():
    return data(120, 6, seed=3)


def test_default_min_child_weight(dev):
    X, y = variant_data()
    clf = fit(dev, X, y, n_estimators=4)
    assert_same_model(clf, xc.fit(X, y, n_estimators=4))
    t = clf.trees_
    assert (t["left"] >= 0).any() and np.delete(t["sum_hessian"], t["root"][:-1]).min() >= 1


def test_min_child_weight_gamma_lambda_and_base_score(dev):
    X, y = variant_data()
    plain = fit(dev, X, y, n_estimators=4)
    for extra in (dict(min_child_weight=5), dict(gamma=0.5), dict(reg_lambda=0), dict(reg_lambda=3), dict(base_score=0.25),
                  dict(min_split_loss=0.5, min_child_weight=2.5, eta=0.05, **{"lambda": 3.5})):
        kw = {{"lambda": "reg_lambda", "eta": "learning_rate", "min_split_loss": "gamma"}.get(k, k): v for k, v in extra.items()}
        clf = fit(dev, X, y, n_estimators=4, **extra)
        assert_same_model(clf, xc.fit(X, y, n_estimators=4, **kw), what=f"{extra}: ")
        if "min_child_weight" in extra or "gamma" in extra:
            assert len(clf.trees_["left"]) < len(plain.trees_["left"])
    heavy = fit(dev, X, y, n_estimators=4, min_child_weight=5).trees_
    assert np.delete(heavy["sum_hessian"], heavy["root"][:-1]).min() >= 5
    given = fit(dev, X, y, n_estimators=1, base_score=0.25)
    assert given.base_score_ == np.float32(0.25) and given.base_margin_ == np.float32(np.log(0.25 / 0.75))


@pytest.mark.parametrize("shape", [(120, 6), (300, 20)])
def test_sampling(dev, shape):
    X, y = data(*shape, seed=sum(shape))
    base = dict(n_estimators=4, max_depth=6, random_state=11)
    for extra in (dict(subsample=0.8), dict(colsample_bytree=0.8), dict(subsample=0.8, colsample_bytree=0.8)):
        ref = xc.fit(X, y, **base, **extra)
        clf = fit(dev, X, y, **base, **extra)
        assert_same_model(clf, ref, what=f"{extra}: ")
        t = clf.trees_
        for tree in range(4):                                 # no split names a masked column
            lo, hi = t["root"][tree], t["root"][tree + 1]
            used = np.unique(t["feature"][lo:hi][t["left"][lo:hi] >= 0])
            assert np.isin(used, ref["live"][ref["col_masks"][tree]]).all(), f"{extra}: tree {tree} splits on a masked column"
        if "colsample_bytree" in extra:
            assert (~ref["col_masks"]).any(axis=1).all()
        if "subsample" in extra:
            assert (~ref["row_masks"]).any(axis=1).all()


def test_random_state(dev):
    X, y = variant_data()
    kw = dict(n_estimators=3, subsample=0.8, colsample_bytree=0.8)
    a, b, c, d = (fit(dev, X, y, random_state=rs, **kw) for rs in (1, 2, 1, None))
    assert_same_model(a, as_ref(c), what="the same random_state: ")
    assert_same_model(d, as_ref(fit(dev, X, y, random_state=0, **kw)), what="None is 0: ")
    assert any(a.trees_[k].shape != b.trees_[k].shape or not np.array_equal(bits(a.trees_[k]), bits(b.trees_[k])) for k in ("feature", "cond"))
    big = fit(dev, X, y, random_state=2 ** 64 - 1, **kw)
    assert_same_model(big, xc.fit(X, y, random_state=2 ** 64 - 1, **kw), what="a 64-bit seed: ")


def test_a_tree_without_sampled_rows(dev):
    """A tiny ``subsample`` on 40 rows leaves some tree without a sampled row: its root holds only unsampled rows and is a leaf of -0.0, with
    ``reg_lambda = 0`` too, where ``-G / (H + lambda)`` would be 0 / 0."""
    X, y = data(40, 4, seed=9)
    for lam in (0.0, 1.0):
        kw = dict(n_estimators=12, max_depth=4, subsample=0.02, reg_lambda=lam, random_state=1)
        ref = xc.fit(X, y, **kw)
        empty = np.flatnonzero(~ref["row_masks"].any(axis=1))
        assert len(empty) and ref["row_masks"].any(), "the restatement must hold a tree without rows and one with rows"
        clf = fit(dev, X, y, **kw)
        assert_same_model(clf, ref, what=f"lambda {lam}: ")
        for t in empty:
            node = clf.trees_["root"][t]
            assert clf.trees_["root"][t + 1] == node + 1 and clf.trees_["sum_hessian"][node] == 0
            assert bits(clf.trees_["cond"][node:node + 1])[0] == bits(np.float32([-0.0]))[0]
        assert np.isfinite(clf.train_margin_).all()


def test_saturation(dev):
    """A separable target with ``learning_rate = 1``, ``reg_lambda = 0``, ``min_child_weight = 0`` and 40 trees: the margins grow by about
    1 per tree until p rounds to 1 in float32 (g = 0 exactly, h = 0: the ``r = 1`` floor) or h falls below 2^-49 (the floor again).  With
    three rows of class 0 and ``subsample = 0.5`` some later tree samples saturated rows of class 1 only: ``gmax = 0``, one leaf of -0.0."""
    X, _ = data(48, 5, seed=21)
    y = (X[:, 0] > 0.1).astype(np.int64)
    kw = dict(n_estimators=40, max_depth=3, learning_rate=1.0, reg_lambda=0.0, min_child_weight=0.0)
    ref = xc.fit(X, y, **kw)
    assert ref["floored"].max() > 0, "the r = 1 floor is reached"
    clf = fit(dev, X, y, **kw)
    assert_same_model(clf, ref)
    assert all(np.isfinite(clf.trees_[k]).all() for k in ("cond",) + STATS) and np.isfinite(clf.train_margin_).all()
    proba = clf.predict_proba(X)
    assert np.isfinite(proba).all() and ((proba[:, 1] > 0.5) == (y == 1)).all()
    order = np.argsort(X[:, 0])
    y2 = np.ones(48, np.int64)
    y2[order[:3]] = 0
    kw2 = dict(kw, subsample=0.5, random_state=4)
    ref2 = xc.fit(X, y2, **kw2)
    zero_g = np.flatnonzero((ref2["gmax"] == 0) & ref2["row_masks"].any(axis=1))
    assert len(zero_g) and ref2["floored"].max() > 0, "no tree of the restatement has sampled rows and gmax = 0: choose another seed"
    for t in zero_g:                                          # such a tree is one leaf of -0.0 over a positive hessian sum
        node = ref2["root"][t]
        assert ref2["root"][t + 1] == node + 1 and ref2["sum_hessian"][node] > 0 and bits(ref2["cond"][node:node + 1])[0] == bits(np.float32([-0.0]))[0]
    clf2 = fit(dev, X, y2, **kw2)
    assert_same_model(clf2, ref2, what="gmax = 0: ")
    assert np.isfinite(clf2.train_margin_).all()


def test_labels_keep_their_order(dev):
    X, y = variant_data()
    ref = xc.fit(X, y, n_estimators=3)
    for labels in (np.array([3, 7]), np.array([7.5, -2.0]), np.array(["no", "yes"]), np.array(["b", "a"]), np.array([True, False])):
        yl = labels[y]
        clf = fit(dev, X, yl, n_estimators=3)
        assert np.array_equal(clf.classes_, np.unique(labels)) and clf.classes_.dtype == np.unique(labels).dtype
        flipped = np.unique(labels)[1] != labels[1]
        assert_same_model(clf, {**(xc.fit(X, 1 - y, n_estimators=3) if flipped else ref), "classes": np.unique(labels)}, what=f"{labels}: ")
        pred = clf.predict(X)
        assert pred.dtype == clf.classes_.dtype and np.isin(pred, clf.classes_).all() and (pred == yl).mean() > 0.8
    with pytest.raises(ValueError, match="exactly two classes"):
        fit(dev, X, np.arange(len(X)) % 3)


def test_float64_input_and_a_row_strided_cuda_view(dev):
    X, y = variant_data()
    ref = xc.fit(X, y, n_estimators=3)
    assert_same_model(fit(dev, X.astype(np.float64), y, n_estimators=3), ref, what="float64: ")
    wide = torch.zeros((2 * len(X), X.shape[1] + 3), dtype=torch.float32, device=dev)
    wide[::2, :X.shape[1]] = torch.from_numpy(X).to(dev)
    view = wide[::2, :X.shape[1]]
    assert not view.is_contiguous()
    clf = fit(dev, view, torch.from_numpy(y).to(dev), n_estimators=3)
    assert_same_model(clf, ref, what="strided view: ")
    for method in ("decision_function", "predict_proba", "predict"):
        got = getattr(clf, method)(view)
        assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(got.cpu().numpy(), getattr(clf, method)(X)), method


def test_prediction(dev):
    """``bbbp_gbt_predict`` adds the trees in ascending order and then the offset, the fit adds the offset first: the training rows'
    margins equal ``train_margin_`` within T float32 ulps of the largest partial sum, not bit for bit.  On fresh rows ``predict_proba``
    equals the restatement's, which sums in the kernel's order."""
    X, y = data(300, 20, seed=320)
    params = dict(n_estimators=6, max_depth=6, learning_rate=0.3)
    ref = xc.fit(X, y, **params)
    clf = fit(dev, X, y, **params)
    assert_same_model(clf, ref)
    T = params["n_estimators"]
    got = clf.decision_function(X)
    bound = T * np.spacing(np.float32(np.abs(ref["train_margin"]).max() + np.abs(ref["base_margin"])))
    err = np.abs(got.astype(np.float64) - clf.train_margin_.astype(np.float64)).max()
    print(f"decision_function(X_train) vs train_margin_: max difference {err:.3e}, bound {bound:.3e}")
    assert got.dtype == np.float32 and got.shape == (300,) and err <= bound
    fresh = np.round(np.random.default_rng(9).normal(size=(257, X.shape[1])), 2).astype(np.float32)
    proba = clf.predict_proba(fresh)
    assert proba.dtype == np.float32 and proba.shape == (257, 2)
    assert np.array_equal(bits(proba), bits(xc.predict_proba(ref, fresh)))
    assert np.array_equal(bits(proba[:, 0]), bits(np.float32(1) - proba[:, 1]))
    assert np.array_equal(bits(clf.decision_function(fresh)), bits(xc.predict_margin(ref, fresh, offset_last=True)))
    assert np.array_equal(clf.predict(fresh), clf.classes_[(proba[:, 1] > 0.5).astype(int)])
    assert np.array_equal(bits(xc.predict_margin(ref, X)), bits(ref["train_margin"]))
    edge = torch.tensor([0.0, -0.0, 1e-30, 17.0, -17.0, 87.0, -87.0, 88.0, -88.0, 1e9, -1e9, 16.5, -103.9], dtype=torch.float32, device=dev)
    from bbbp_amd import xgb
    assert np.array_equal(bits(xgb._proba_of_margin(edge).cpu().numpy()), bits(xc.proba_of_margin(edge.cpu().numpy())))
    wide = torch.from_numpy(np.random.default_rng(1).uniform(-110, 110, 200_000).astype(np.float32)).to(dev)
    assert np.array_equal(bits(xgb._proba_of_margin(wide).cpu().numpy()), bits(xc.proba_of_margin(wide.cpu().numpy()))), "sigmoid32: device vs numpy"


def test_one_column_that_alone_separates_y(dev):
    X, _ = variant_data()
    y = (X[:, 4] > 0.1).astype(np.int64)
    clf = fit(dev, X, y, n_estimators=3, max_depth=3)
    assert_same_model(clf, xc.fit(X, y, n_estimators=3, max_depth=3))
    assert clf.trees_["feature"][0] == 4 and np.all(X[:, 4][X[:, 4] > 0.1] >= clf.trees_["cond"][0])
    assert (clf.predict(X) == y).mean() == 1.0


def test_batch_invariance(dev):
    from bbbp_amd import xgb
    shapes = [(2, 1, 1, 256, dict(min_child_weight=0)), (40, 12, 6, 256, dict(subsample=0.7, random_state=3)), (65, 7, 30, 256, dict(min_child_weight=0)),
              (130, 9, 5, 16, dict(colsample_bytree=0.5)), (300, 20, 30, 256, dict(min_child_weight=0.5, subsample=0.8, colsample_bytree=0.8)),
              (64, 3, 8, 2, dict(reg_lambda=0))]
    problems = [data(n, d, seed=7 * n + d) for n, d, _, _, _ in shapes]
    clfs = [xgb.XGBClassifier(n_estimators=3, max_depth=depth, max_bin=mb, device=dev, **extra) for _, _, depth, mb, extra in shapes]
    alone = [xgb.XGBClassifier(**c.get_params()).fit(X, y) for c, (X, y) in zip(clfs, problems)]
    for run in range(2):
        xgb._fit_classifiers(clfs, problems)
        for i, (clf, one) in enumerate(zip(clfs, alone)):
            assert_same_model(clf, as_ref(one), what=f"run {run} problem {i}: ")
    assert_same_model(alone[4], xc.fit(*problems[4], n_estimators=3, max_depth=30, min_child_weight=0.5, subsample=0.8, colsample_bytree=0.8),
                      what="alone vs restatement: ")


def test_folds_and_refit_in_one_batch(dev):
    from bbbp_amd import xgb
    X, y = data(101, 6, seed=5)
    bounds = np.linspace(0, len(X), 6).astype(int)
    rows = [np.concatenate([np.arange(0, bounds[f]), np.arange(bounds[f + 1], len(X))]) for f in range(5)]
    params = dict(n_estimators=3, max_depth=30, learning_rate=0.1, subsample=0.8, colsample_bytree=0.8, random_state=6, device=dev)
    batch = xgb.fit_classifiers([(X, y, r) for r in rows] + [(X, y)], **params)
    for clf, r in zip(batch, rows + [np.arange(len(X))]):
        assert_same_model(clf, as_ref(xgb.XGBClassifier(**params).fit(X[r], y[r])), what=f"{len(r)} rows: ")
    host = {k: v for k, v in params.items() if k != "device"}
    assert_same_model(batch[0], xc.fit(X[rows[0]], y[rows[0]], **host), what="fold 0 vs restatement: ")


def test_stack_and_vote(dev):
    from bbbp_amd import ensemble, random_forest, xgb
    X, y = data(60, 8, seed=2)
    xp = dict(n_estimators=3, max_depth=3, subsample=0.8, random_state=1, device=dev)
    members = lambda: [("xgb", xgb.XGBClassifier(**xp)),  # noqa: E731
                       ("rf", random_forest.RandomForestClassifier(n_estimators=3, max_depth=3, random_state=0, device=dev))]
    assert ensemble._batched_path(members()[0][1]) == "xgb._fit_classifiers"
    stack = ensemble.StackingClassifier(members(), cv=3).fit(X, y)
    assert stack.fit_paths_["xgb"] == "xgb._fit_classifiers"
    proba = stack.predict_proba(X)
    assert proba.shape == (60, 2) and np.isfinite(proba).all() and (stack.predict(X) == y).mean() > 0.7
    full = stack.estimators_[0]
    assert_same_model(full, as_ref(xgb.XGBClassifier(**xp).fit(X, y)), what="the stack's refit: ")
    vote = ensemble.VotingClassifier(members(), voting="soft").fit(X, y)
    assert vote.fit_paths_["xgb"] == "xgb._fit_classifiers" and (vote.predict(X) == y).mean() > 0.7
    assert_same_model(vote.estimators_[0], as_ref(full), what="the vote's fit: ")
    # the fold clones equal single fits on the gathered rows
    from sklearn.model_selection import StratifiedKFold
    folds = list(StratifiedKFold(n_splits=3).split(X, y))
    Xd = torch.from_numpy(X).to(dev)
    clones = ensemble._fit_rows(xgb.XGBClassifier(**xp), Xd, y, [None] + [tr for tr, _ in folds])
    for clone, r in zip(clones, [np.arange(len(X))] + [tr for tr, _ in folds]):
        assert_same_model(clone, as_ref(xgb.XGBClassifier(**xp).fit(X[r], y[r])), what=f"fold clone of {len(r)} rows: ")


def test_randomized_search(dev):
    from sklearn.model_selection import ParameterSampler, StratifiedKFold
    from bbbp_amd import metrics, xgb
    X, y = data(150, 6, seed=8)
    dists = dict(n_estimators=[2, 3, 5], learning_rate=[0.1, 0.3], max_depth=[2, 3], subsample=[0.8, 1.0], colsample_bytree=[0.8, 1.0], reg_lambda=[1, 10],
                 gamma=[0, 0.1], min_child_weight=[1, 3])
    best, means, fitted = xgb.randomized_search_cv(X, y, dists, n_iter=6, cv=3, random_state=0, device=dev)
    points = list(ParameterSampler(dists, n_iter=6, random_state=0))
    folds = list(StratifiedKFold(n_splits=3).split(X, y))
    assert set(means) == {"accuracy", "precision"} and all(len(v) == 6 for v in means.values())
    for pi, pt in enumerate(points):
        acc, prec = [], []
        for tr, te in folds:
            pred = xgb.XGBClassifier(device=dev, **pt).fit(X[tr], y[tr]).predict(X[te])
            got = metrics.classification_scores(y[te], pred, pos_label=1, zero_division=0, device=dev)
            acc.append(got["Accuracy"][0, 0]); prec.append(got["Precision"][0, 0])
        assert means["accuracy"][pi] == float(np.mean(acc)) and means["precision"][pi] == float(np.mean(prec)), f"point {pi}: {pt}"
    assert best == points[int(np.argmax(means["accuracy"]))]
    assert_same_model(fitted, as_ref(xgb.XGBClassifier(device=dev, **best).fit(X, y)), what="the refit: ")
