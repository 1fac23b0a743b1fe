"""``bbbp_amd.cat.CatBoostClassifier`` on the GPU against its numpy restatement (``tests/catc_numpy.py``), bit for bit: splits, borders,
leaf values, leaf weights, the bias and the training rows' raw values; then the labels, the edge cases, prediction, batch invariance,
the stack and the randomized search.

The shapes are ``tests/test_gpu_cat.py``'s, the smallest at which the kernels can go wrong: two rows whose candidates run out, 256 leaves
for 40 rows (mostly empty parts), parts on either side of the 64-row boundary between the lane-against-lane form and the histogram form
(64 and 65 rows at the root, both forms inside one tree), features of at most 64 cuts (one cut per lane) and of more (four per lane),
the quantile rule, one border per feature, and more feature blocks than one with dropped constant columns.  The label is ``y >
median(y)`` of those recipes.  Every case runs without a bootstrap; ``n65``, ``n300`` and ``n1058_mixed`` also with the Bayesian
bootstrap at the temperatures 0.5 and 1.0."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import catc_numpy as cc  # noqa: E402
from test_gpu_cat import CASES, KEYS, bits, data, mixed_data  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 42
RUNS = [(name, None) for name in CASES] + [(name, temp) for name in ("n65", "n300", "n1058_mixed") for temp in (0.5, 1.0)]


def labels_of(y):
    return (y > np.median(y)).astype(np.int64)


def host_params(params):
    """The restatement's arguments for the classifier's: ``bootstrap_type="No"`` is no temperature."""
    out = {k: v for k, v in params.items() if k not in ("bootstrap_type", "device")}
    out.setdefault("bagging_temperature", None)
    return out


@functools.lru_cache(maxsize=None)
def case(name, temperature=None):
    n, d, T, depth, border_count, eta = CASES[name]
    X, y = mixed_data(n) if name == "n1058_mixed" else data(n, d, seed=n + d)
    t = labels_of(y)
    params = dict(iterations=T, depth=depth, border_count=border_count, learning_rate=eta)
    params.update(dict(bootstrap_type="No") if temperature is None else dict(bagging_temperature=temperature, random_seed=SEED))
    return X, t, params, cc.fit(X, t, **host_params(params))


def reference_of(clf):
    return {**clf.trees_, "bias": clf.bias_, "train_approx": clf.train_approx_}


def assert_same_model(clf, ref, what=""):
    for key in KEYS:
        got, want = np.asarray(clf.trees_[key]), np.asarray(ref[key])
        assert got.shape == want.shape, f"{what}{key}: shape {got.shape}, the restatement has {want.shape}"
        assert got.dtype == want.dtype, f"{what}{key}: dtype {got.dtype} != {want.dtype}"
        assert np.array_equal(bits(got), bits(want)), f"{what}{key}: first difference at {int(np.flatnonzero(bits(got) != bits(want))[0])}"
    assert np.float64(clf.bias_).tobytes() == np.float64(ref["bias"]).tobytes(), f"{what}bias"
    assert clf.train_approx_.dtype == np.float64 and np.array_equal(bits(clf.train_approx_), bits(ref["train_approx"])), f"{what}train_approx_"
    m = clf.model_.arrays
    assert np.array_equal(m["split_feature"], ref["split_feature"]) and np.array_equal(bits(m["split_border"]), bits(ref["split_border"]))
    assert np.array_equal(bits(m["leaf_values"]), bits(ref["leaf_values"])) and clf.model_.scale == 1.0 and not m["nan_true"].any()


def fit(dev, X, y, **params):
    from bbbp_amd import cat
    return cat.CatBoostClassifier(device=dev, **params).fit(X, y)


@pytest.mark.parametrize("name, temperature", RUNS)
def test_fit_equals_the_restatement_bit_for_bit(dev, name, temperature):
    X, t, params, ref = case(name, temperature)
    clf = fit(dev, X, t, **params)
    assert_same_model(clf, ref)
    assert clf.n_features_in_ == X.shape[1] and clf.tree_count_ == params["iterations"] and np.array_equal(clf.classes_, [0, 1])
    levels = np.diff(ref["tree_first_split"])
    if name == "n2":                          # one candidate: every tree has one level
        assert np.array_equal(levels, [1, 1, 1])
    else:
        assert np.all(levels == params["depth"])
    if name == "n40":                         # 256 leaves for 40 rows
        assert (ref["leaf_weights"] == 0).sum() >= 4 * (256 - 40)
    if name == "n300":                        # both forms in one tree: at some level a part of more than 64 rows and one of at most 64
        w = ref["leaf_weights"][:1 << levels[0]]
        parts = [np.bincount(np.arange(len(w)) & ((1 << lv) - 1), weights=w) for lv in range(1, levels[0])]       # bit i is split i
        assert any((p > 64).any() and ((p > 0) & (p <= 64)).any() for p in parts)
    if name == "n1058_mixed":                 # constant columns never split, features keep their original indices
        used = np.unique(ref["split_feature"])
        assert not np.isin(used % 5, [2]).any() and len(used) > 1
    if temperature is not None:               # the bootstrap shapes the structure: the weighted trees are others than the plain ones
        plain = case(name)[3]
        assert not np.array_equal(ref["split_feature"], plain["split_feature"]) or not np.array_equal(ref["split_bin"], plain["split_bin"])


def variant_data():
    X, y = data(120, 6, seed=3)
    return X, labels_of(y)


def test_temperature_zero_equals_no_bootstrap(dev):
    X, t, params, ref = case("n65")
    weighted = fit(dev, X, t, **{**host_params(params), "bagging_temperature": 0, "random_seed": 5})
    assert_same_model(weighted, ref, what="temperature 0: ")
    bayes = fit(dev, X, t, **{**host_params(params), "bagging_temperature": None, "bootstrap_type": "Bayesian", "random_seed": SEED})
    assert_same_model(bayes, case("n65", 1.0)[3], what="Bayesian without a temperature is temperature 1: ")


def test_string_labels_and_signed_labels(dev):
    X, t = variant_data()
    ref = cc.fit(X, t, iterations=3, depth=4, bagging_temperature=0.5, random_seed=1)
    for names in (np.array(["ham", "spam"]), np.array([-1, 1]), np.array([-1.0, 1.0])):
        clf = fit(dev, X, names[t], iterations=3, depth=4, bagging_temperature=0.5, random_seed=1)
        assert_same_model(clf, ref, what=f"{names!r}: ")
        assert np.array_equal(clf.classes_, names) and clf.classes_.dtype == names.dtype
        pred = clf.predict(X)
        assert pred.dtype == names.dtype and np.array_equal(pred, names[(ref["train_approx"] > 0).astype(int)])
        on_device = clf.predict(torch.from_numpy(X).to(dev))
        if names.dtype.kind in "if":
            assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), pred)
        else:
            assert np.array_equal(on_device, pred)


def test_one_positive_row_among_120(dev):
    X, _ = variant_data()
    t = np.zeros(120, np.int64); t[77] = 1
    ref = cc.fit(X, t, iterations=4, depth=4, learning_rate=0.3)
    clf = fit(dev, X, t, iterations=4, depth=4, learning_rate=0.3)
    assert_same_model(clf, ref)
    assert clf.bias_ == float(np.log(np.float64(1.0) / np.float64(119.0)))


def test_boost_from_average_false(dev):
    X, t = variant_data()
    clf = fit(dev, X, t, iterations=3, depth=3, boost_from_average=False)
    assert_same_model(clf, cc.fit(X, t, iterations=3, depth=3, boost_from_average=False))
    assert clf.bias_ == 0.0
    assert_same_model(fit(dev, X, t, iterations=3, depth=3, boost_from_average=True), cc.fit(X, t, iterations=3, depth=3), what="True: ")


def test_saturated_margins(dev):
    """Separable data, ``l2_leaf_reg=0`` at ``learning_rate=1``: the margins saturate and ``r`` sits at its floor of 1."""
    rng = np.random.default_rng(5)
    X = np.round(rng.normal(size=(60, 3)), 1).astype(np.float32)
    t = (X[:, 0] > 0).astype(np.int64)
    params = dict(iterations=40, depth=2, learning_rate=1.0, l2_leaf_reg=0)
    ref = cc.fit(X, t, **params)
    assert (cc.quantise(t.astype(np.float64), ref["train_approx"])[2] == 1).any()
    clf = fit(dev, X, t, **params)
    assert_same_model(clf, ref)
    assert np.isfinite(clf.trees_["leaf_values"]).all() and np.array_equal(clf.predict(X), t)


def test_float64_input_and_a_row_strided_cuda_view(dev):
    X, t = variant_data()
    ref = cc.fit(X, t, iterations=3, bagging_temperature=1.0, random_seed=2)
    params = dict(iterations=3, bagging_temperature=1.0, random_seed=2)
    assert_same_model(fit(dev, X.astype(np.float64), t, **params), ref, what="float64: ")
    wide = torch.zeros((2 * len(X), X.shape[1] + 3), dtype=torch.float32, device=dev)
    wide[::2, :X.shape[1]] = torch.from_numpy(X).to(dev)
    view = wide[::2, :X.shape[1]]
    assert not view.is_contiguous()
    clf = fit(dev, view, torch.from_numpy(t).to(dev), **params)
    assert_same_model(clf, ref, what="strided view: ")
    got = clf.predict_proba(view)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), clf.predict_proba(X))


def test_prediction(dev):
    """``predict`` sums in ``obl_sum_kernel``'s order, which is the fit's: the training rows' raw values equal ``train_approx_`` bit for bit;
    probabilities, classes and raw values of fresh rows equal the restatement's, for numpy and for CUDA queries; the device's sigmoid
    equals numpy's on a sweep and at the edges."""
    from bbbp_amd import boosters, cat
    X, t, params, ref = case("n300", 0.5)
    clf = fit(dev, X, t, **params)
    raw = clf.predict(X, prediction_type="RawFormulaVal")
    assert raw.dtype == np.float64 and np.array_equal(bits(raw), bits(clf.train_approx_)) and np.array_equal(bits(raw), bits(cc.predict(ref, X)))
    fresh = np.round(np.random.default_rng(9).normal(size=(257, X.shape[1])), 2).astype(np.float32)
    want = cc.predict_proba(ref, fresh)
    for query in (fresh, torch.from_numpy(fresh).to(dev)):
        host = (lambda a: a.cpu().numpy()) if isinstance(query, torch.Tensor) else (lambda a: a)
        proba = clf.predict_proba(query)
        assert isinstance(proba, type(query)) and (not isinstance(query, torch.Tensor) or proba.is_cuda)
        proba = host(proba)
        assert proba.dtype == np.float64 and proba.shape == (257, 2) and np.array_equal(bits(proba), bits(want))
        assert np.array_equal(bits(host(clf.predict(query, prediction_type="Probability"))), bits(want))
        assert np.array_equal(bits(host(clf.predict(query, prediction_type="RawFormulaVal"))), bits(cc.predict(ref, fresh)))
        assert np.array_equal(host(clf.predict(query)), cc.predict_class(ref, fresh).astype(np.int64))
        with np.errstate(divide="ignore"):                   # a logarithm is a library function: a few ulp, not bits
            assert np.allclose(host(clf.predict_log_proba(query)), np.log(want), rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="prediction_type"):
        clf.predict(fresh, prediction_type="LogProbability")
    back = boosters.CatBoostTrees.from_json(clf.get_model_json(), device=dev)
    assert np.array_equal(bits(back.predict(fresh)), bits(cc.predict(ref, fresh)))
    edge = np.array([0.0, -0.0, 1e-300, -1e-300, 36.0, -36.0, 40.0, -40.0, 700.0, -700.0, 745.0, -745.0, 1e6, -1e6])
    sweep = np.concatenate([edge, np.random.default_rng(1).uniform(-720, 720, 200_000), np.random.default_rng(2).normal(scale=6, size=100_000)])
    p1 = cc.sigmoid64(sweep)
    got = cat._proba_of_raw(torch.from_numpy(sweep).to(dev)).cpu().numpy()
    assert np.array_equal(bits(got[:, 1]), bits(p1)) and np.array_equal(bits(got[:, 0]), bits(1.0 - p1)), "sigmoid64: device vs numpy"
    assert cat._proba_of_raw(torch.empty(0, dtype=torch.float64, device=dev)).shape == (0, 2)


def test_batch_invariance(dev):
    from bbbp_amd import cat
    shapes = [(2, 1, 3, 254, None), (40, 12, 8, 254, 0.5), (65, 7, 6, 254, 1.0), (130, 9, 5, 15, 0.5), (300, 20, 6, 254, None), (64, 3, 4, 1, 0.25)]
    problems = [(X, labels_of(y)) for X, y in (data(n, d, seed=7 * n + d) for n, d, _, _, _ in shapes)]
    clfs = [cat.CatBoostClassifier(iterations=2 + (i % 2), depth=depth, border_count=bc, learning_rate=0.2, bagging_temperature=temp,
                                   random_seed=SEED if i != 3 else 7, device=dev) for i, (_, _, depth, bc, temp) in enumerate(shapes)]
    alone = [cat.CatBoostClassifier(**c.get_params()).fit(X, t) for c, (X, t) in zip(clfs, problems)]
    for run in range(2):
        cat._fit_classifiers(clfs, problems)
        for i, (clf, one) in enumerate(zip(clfs, alone)):
            assert_same_model(clf, reference_of(one), what=f"run {run} problem {i}: ")
    assert_same_model(alone[3], cc.fit(*problems[3], iterations=3, depth=5, border_count=15, learning_rate=0.2, bagging_temperature=0.5, random_seed=7),
                      what="alone vs restatement: ")


def test_folds_and_refit_in_one_batch(dev):
    from bbbp_amd import cat
    X, y = data(101, 6, seed=5)
    t = labels_of(y)
    bounds = np.linspace(0, len(X), 6).astype(int)
    rows = [np.concatenate([np.arange(0, bounds[f]), np.arange(bounds[f + 1], len(X))]) for f in range(5)]
    params = dict(iterations=3, depth=5, learning_rate=0.1, bagging_temperature=0.5, random_seed=6, device=dev)
    batch = cat.fit_classifiers([(X, t, r) for r in rows] + [(X, t)], **params)
    for clf, r in zip(batch, rows + [np.arange(len(X))]):
        assert_same_model(clf, reference_of(cat.CatBoostClassifier(**params).fit(X[r], t[r])), what=f"{len(r)} rows: ")
    assert_same_model(batch[0], cc.fit(X[rows[0]], t[rows[0]], **host_params(params)), what="fold 0 vs restatement: ")


def test_stack_and_vote(dev):
    from sklearn.model_selection import StratifiedKFold
    from bbbp_amd import cat, ensemble, linear_model
    X, y = data(200, 6, seed=2)
    t = labels_of(y)
    cp = dict(iterations=3, depth=3, learning_rate=0.3, bagging_temperature=0.5, random_seed=1, device=dev)
    members = lambda: [("cat", cat.CatBoostClassifier(**cp)), ("lr", linear_model.LogisticRegression(device=dev))]  # noqa: E731
    assert ensemble._batched_path(members()[0][1]) == "cat._fit_classifiers"
    stack = ensemble.StackingClassifier(members(), cv=3).fit(X, t)
    assert stack.fit_paths_["cat"] == "cat._fit_classifiers"
    proba = stack.predict_proba(X)
    assert proba.shape == (200, 2) and np.isfinite(proba).all() and (stack.predict(X) == t).mean() > 0.7
    full = stack.estimators_[0]
    assert_same_model(full, reference_of(cat.CatBoostClassifier(**cp).fit(X, t)), what="the stack's refit: ")
    vote = ensemble.VotingClassifier(members(), voting="soft").fit(X, t)
    assert vote.fit_paths_["cat"] == "cat._fit_classifiers" and (vote.predict(X) == t).mean() > 0.7
    assert_same_model(vote.estimators_[0], reference_of(full), what="the vote's fit: ")
    # the batched fold fits equal the one-at-a-time fits on the gathered rows
    folds = list(StratifiedKFold(n_splits=3).split(X, t))
    Xd = torch.from_numpy(X).to(dev)
    clones = ensemble._fit_rows(cat.CatBoostClassifier(**cp), Xd, t, [None] + [tr for tr, _ in folds])
    for clone, r in zip(clones, [np.arange(len(X))] + [tr for tr, _ in folds]):
        assert_same_model(clone, reference_of(cat.CatBoostClassifier(**cp).fit(X[r], t[r])), what=f"fold clone of {len(r)} rows: ")


def test_randomized_search(dev):
    from sklearn.model_selection import ParameterSampler, StratifiedKFold
    from bbbp_amd import cat, metrics
    X, y = data(150, 5, seed=8)
    t = labels_of(y)
    dists = dict(iterations=[2, 3, 5], learning_rate=[0.1, 0.3], depth=[2, 3], l2_leaf_reg=[1, 5], border_count=[32, 254], bagging_temperature=[0.5, 1.0])
    best, means, fitted = cat.randomized_search_cv(X, t, dists, n_iter=4, cv=3, random_state=0, device=dev, random_seed=SEED)
    points = list(ParameterSampler(dists, n_iter=4, random_state=0))
    folds = list(StratifiedKFold(n_splits=3).split(X, t))
    assert set(means) == {"accuracy", "precision"} and all(len(v) == 4 for v in means.values())
    for pi, pt in enumerate(points):
        acc, prec = [], []
        for tr, te in folds:
            pred = cat.CatBoostClassifier(device=dev, random_seed=SEED, **pt).fit(X[tr], t[tr]).predict(X[te])
            got = metrics.classification_scores(t[te], pred, pos_label=1, zero_division=0, device=dev)
            acc.append(got["Accuracy"][0, 0]); prec.append(got["Precision"][0, 0])
        assert means["accuracy"][pi] == float(np.mean(acc)) and means["precision"][pi] == float(np.mean(prec)), f"point {pi}: {pt}"
    assert best == points[int(np.argmax(means["accuracy"]))]
    assert_same_model(fitted, reference_of(cat.CatBoostClassifier(device=dev, random_seed=SEED, **best).fit(X, t)), what="the refit: ")
