"""GPU: ``bbbp_amd.metrics`` against its numpy restatement (tests/metrics_numpy.py).  The device computes integers and sums in a fixed
order, so the confusion counts, U2, P and N are asserted exactly and the squared-error sums, and with them all ten scores, bit for bit
(``==`` on the bytes).  Shapes: word tails (63, 64, 65), tile tails and more than one pair tile per column (257, 1025), one row; one and
five columns; one segment, and three with one empty, one holding a single class and rows left out; float32 and float64 scores."""
import functools
import warnings

import numpy as np
import pytest
import torch

import metrics_numpy as R
from bbbp_amd import metrics

pytestmark = pytest.mark.gpu

NS, MS, GS = [1, 2, 63, 64, 65, 257, 1025], [1, 5], [1, 3]
KEYS = metrics.KEYS


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0, R.bits(a)), np.where(np.isnan(b), 0, R.bits(b)))      # == on the bytes; a NaN equals a NaN


@functools.lru_cache(maxsize=None)
def _reference(n, M, G, dtype, ties=0.0, one_class=False):
    y, pred, scores, groups = R.problem(n, M, G, ties=ties, dtype=np.dtype(dtype), left_out=G > 1, one_class=one_class)
    rs = np.random.RandomState(n + M)
    target = rs.randn(n) * 2.0 + 1.0
    fitted = (target[None, :] + rs.randn(M, n) * 0.5).astype(dtype)
    ref = {"y": y, "pred": pred, "scores": scores, "groups": groups, "target": target, "fitted": fitted,
           "counts": R.confusion_counts(y, pred, groups), "pairs": R.pair_counts(y, scores, groups),
           "cls": R.classification_scores(y, pred, scores, groups), "hard": R.classification_scores(y, pred, None, groups),
           "sums": R.squared_error_sums(target, fitted, groups), "reg": R.regression_scores(target, fitted, groups)}
    for v in ref.values():
        for a in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return ref


def _check_all(dev, r, scores=None, fitted=None):
    scores = r["scores"] if scores is None else scores
    fitted = r["fitted"] if fitted is None else fitted
    y, pred, groups = r["y"], r["pred"], r["groups"]
    counts = metrics.confusion_counts(y, pred, groups=groups, device=dev)
    assert counts.dtype == np.int64 and np.array_equal(counts, r["counts"])
    by_threshold = metrics.confusion_counts(y, scores, groups=groups, threshold=0.5, device=dev)
    assert np.array_equal(by_threshold, r["counts"])
    pairs = metrics.auc_pair_counts(y, scores, groups=groups, device=dev) if len(np.unique(y)) == 2 else None
    if pairs is not None:
        assert pairs.dtype == np.int64 and np.array_equal(pairs, r["pairs"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # the batched calls do not warn
        got = metrics.classification_scores(y, pred, scores, groups=groups, device=dev)
        hard = metrics.classification_scores(y, pred, groups=groups, device=dev)
        reg = metrics.regression_scores(r["target"], fitted, groups=groups, device=dev)
    for k in KEYS:
        assert got[k].dtype == np.float64 and _same(got[k], r["cls"][k]), k
        assert _same(hard[k], r["hard"][k]), k
    sse, ystat = metrics.squared_error_sums(r["target"], fitted, groups=groups, device=dev)
    assert _same(sse, r["sums"][0]) and _same(ystat, r["sums"][1])
    assert _same(reg["MSE"], r["reg"]["MSE"]) and _same(reg["R2"], r["reg"]["R2"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
def test_integers_and_scores_equal_the_restatement(dev, n, M, G, dtype):
    r = _reference(n, M, G, dtype)
    if G == 3 and n >= 63:
        assert r["counts"][:, 1].sum() == 0 and r["counts"][:, 2, :2].sum() == 0 and (r["groups"] == -1).any()
        assert np.isnan(r["cls"]["F1 Score"][:, 1]).all() and np.isnan(r["cls"]["ROC AUC"][:, 2]).all()
    _check_all(dev, r)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,M,G", [(65, 5, 3), (1025, 5, 1)])
def test_device_tensors_and_row_strided_views_are_read_in_place(dev, n, M, G, dtype):
    r = _reference(n, M, G, "float64" if dtype == torch.float64 else "float32")
    big = torch.full((M, n + 7), float("nan"), dtype=dtype, device=dev)
    scores = big[:, 3:3 + n]
    scores.copy_(torch.from_numpy(np.array(r["scores"])))
    fit_big = torch.full((M, n + 5), float("inf"), dtype=dtype, device=dev)
    fitted = fit_big[:, 1:1 + n]
    fitted.copy_(torch.from_numpy(np.array(r["fitted"])))
    assert scores.stride(0) == n + 7 and not scores.is_contiguous()
    _check_all(dev, r, scores, fitted)
    got = metrics.classification_scores(torch.from_numpy(np.array(r["y"])).to(dev), torch.from_numpy(np.array(r["pred"])).to(dev), scores,
                                        groups=r["groups"])
    for k in KEYS:
        assert _same(got[k], r["cls"][k]), k


@pytest.mark.parametrize("n,M,G", [(257, 5, 3), (1025, 1, 1)])
def test_scores_with_ninety_percent_ties(dev, n, M, G):
    r = _reference(n, M, G, "float64", ties=0.9)
    assert len(np.unique(r["scores"])) < 0.2 * r["scores"].size
    _check_all(dev, r)


@pytest.mark.parametrize("n,G", [(65, 1), (257, 3)])
def test_y_true_of_one_class(dev, n, G):
    r = _reference(n, 5, G, "float64", one_class=True)
    assert r["y"].min() == 1
    _check_all(dev, r)
    assert np.isnan(r["cls"]["ROC AUC"]).all() and (r["cls"]["MCC"][:, 0] == 0).all()


def test_signed_zeros_compare_equal_and_labels_may_be_any_pair(dev):
    y = np.array([-1, 1, -1, 1, 1, -1])
    s = np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0])
    assert np.array_equal(metrics.auc_pair_counts(y, s, device=dev)[0, 0], R.pair_counts(y == 1, s)[0, 0])
    assert metrics.roc_auc_score(y, s, device=dev) == float(metrics.auc_from_pairs(*R.pair_counts(y == 1, s)[0, 0]))
    p = np.array([-1, 1, 1, 1, -1, -1])
    want = R.classification_scores(y == 1, p == 1)
    got = metrics.classification_scores(y, p, device=dev)
    flipped = metrics.classification_scores(y, p, pos_label=-1, device=dev)
    want_flipped = R.classification_scores(y == -1, p == -1)
    for k in KEYS[:7]:
        assert _same(got[k], want[k]) and _same(flipped[k], want_flipped[k]), k
    assert _same(got["ROC AUC"], want["ROC AUC"]) and _same(flipped["ROC AUC"], want["ROC AUC"])      # the AUC's positive is the greater label
    names = np.array(["no", "yes", "no", "yes", "yes", "no"])
    assert metrics.f1_score(names, np.where(p == 1, "yes", "no"), pos_label="yes", device=dev) == float(want["F1 Score"][0, 0])
    assert np.array_equal(metrics.confusion_matrix(y, p, device=dev), R.confusion_counts(y == 1, p == 1)[0, 0].reshape(2, 2))


def test_more_than_one_row_tile_of_confusion_counts(dev):
    """16 384 rows are one tile of the confusion kernel: one row more takes the slab path and its sum pass."""
    n = metrics.TILE_ROWS + 1
    rs = np.random.RandomState(4)
    y, p, g = rs.randint(0, 2, n), rs.randint(0, 2, (2, n)), rs.randint(-1, 3, n)
    before = dict(metrics._LAUNCHES)
    assert np.array_equal(metrics.confusion_counts(y, p, groups=g, device=dev), R.confusion_counts(y, p, g))
    assert metrics._LAUNCHES["confusion"] - before["confusion"] == 1 and metrics._LAUNCHES["sum"] - before["sum"] == 1


def test_contraction_canary_a_fused_multiply_add_would_change_the_mse_bits(dev):
    """Precondition: on this problem fusing ``d * d + acc`` into one rounding changes the bits of a squared-error sum, so bit equality
    of the GPU result shows that the kernel does not contract them."""
    r = _reference(1025, 5, 1, "float64")                    # four or five rows per lane: with 257 a lane adds one square to 0.0 and fusing changes nothing
    fused = R.squared_error_sums(r["target"], r["fitted"], None, fused=True)
    assert (R.bits(fused[0]) != R.bits(r["sums"][0])).any()
    assert np.abs(fused[0] - r["sums"][0]).max() <= 1025 * 2.0 ** -52 * r["sums"][0].max()
    sse, ystat = metrics.squared_error_sums(r["target"], r["fitted"], device=dev)
    assert _same(sse, r["sums"][0]) and _same(ystat, r["sums"][1])
    assert not _same(sse, fused[0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_scores_raise(dev, bad):
    r = _reference(257, 5, 3, "float64")
    scores, fitted = np.array(r["scores"]), np.array(r["fitted"])
    row = int(np.flatnonzero(r["groups"] == 0)[-1])
    scores[3, row] = fitted[3, row] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.classification_scores(r["y"], r["pred"], scores, groups=r["groups"], device=dev)
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.confusion_counts(r["y"], scores, groups=r["groups"], threshold=0.5, device=dev)
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.regression_scores(r["target"], fitted, groups=r["groups"], device=dev)
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.roc_auc_score(r["y"], scores[3], device=dev)
    target = np.array(r["target"])
    target[row] = bad
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.regression_scores(target, r["fitted"], device=dev)


def test_scalar_functions_equal_scikit_learn(dev):
    import sklearn.metrics as skm
    r = _reference(257, 1, 1, "float64")
    y, p, s = r["y"], r["pred"][0], r["scores"][0]
    for name in ("accuracy_score", "balanced_accuracy_score", "precision_score", "recall_score", "f1_score", "matthews_corrcoef", "cohen_kappa_score"):
        assert getattr(metrics, name)(y, p, device=dev) == getattr(skm, name)(y, p), name
    assert np.array_equal(metrics.confusion_matrix(y, p, device=dev), skm.confusion_matrix(y, p))
    b = skm.roc_auc_score(y, s)
    assert abs(metrics.roc_auc_score(y, s, device=dev) - b) <= (len(y) + 6) * 2.0 ** -53 * b
    t, f = r["target"], r["fitted"][0]
    mse, r2 = skm.mean_squared_error(t, f), skm.r2_score(t, f)
    n = len(t)
    assert abs(metrics.mean_squared_error(t, f, device=dev) - mse) <= (2 * n + 2) * 2.0 ** -53 * mse       # bounds: tests/test_metrics_cpu.py
    assert abs(metrics.r2_score(t, f, device=dev) - r2) <= (4 * n + 8) * 2.0 ** -53 * (1 - r2) + 2.0 ** -52 * abs(r2)
    with pytest.warns(metrics.UndefinedMetricWarning):
        assert metrics.precision_score(y, np.zeros_like(p), device=dev) == 0.0
    assert metrics.precision_score(y, np.zeros_like(p), zero_division=1, device=dev) == 1.0


def test_evaluate_models_equals_scikit_learn_on_the_same_predictions(dev):
    """Two fitted package models on a 257 x 20 problem: the seven count scores bit for bit, the AUC within its bound."""
    import sklearn.metrics as skm
    from bbbp_amd import linear_model, naive_bayes
    rs = np.random.RandomState(0)
    n, d = 257, 20
    y = (rs.rand(n) < 0.45).astype(np.int64)
    X = rs.randn(n, d) + 0.8 * y[:, None] * (rs.rand(d) < 0.5)
    models = {"BernoulliNB": naive_bayes.BernoulliNB(device=dev).fit(X, y), "LogisticRegression": linear_model.LogisticRegression(device=dev).fit(X, y)}
    before = dict(metrics._LAUNCHES)
    table = metrics.evaluate_models(models, X, y)
    launches = {k: metrics._LAUNCHES[k] - before[k] for k in before}
    assert launches == {"confusion": 1, "pairs": 1, "sum": 1, "sq_sums": 0}, launches
    assert list(table) == list(models)
    for name, model in models.items():
        p, s = model.predict(X), model.predict_proba(X)[:, 1]
        want = {"Accuracy": skm.accuracy_score(y, p), "Balanced Accuracy": skm.balanced_accuracy_score(y, p), "Precision": skm.precision_score(y, p),
                "Recall": skm.recall_score(y, p), "F1 Score": skm.f1_score(y, p), "MCC": skm.matthews_corrcoef(y, p),
                "Cohen's Kappa": skm.cohen_kappa_score(y, p)}
        assert 0.5 < want["Accuracy"] < 1.0
        for k, v in want.items():
            assert np.float64(table[name][k]).tobytes() == np.float64(v).tobytes(), (name, k)
        b = skm.roc_auc_score(y, s)
        assert abs(table[name]["ROC AUC"] - b) <= (n + 6) * 2.0 ** -53 * b

    class Hard:                                                  # no predict_proba: the hard predictions are the scores, as evaluate_model
        def predict(self, X):
            return models["BernoulliNB"].predict(X)
    p = models["BernoulliNB"].predict(X)
    got = metrics.evaluate_models([Hard()], X, y, names=["hard"])["hard"]
    b = skm.roc_auc_score(y, p)
    assert abs(got["ROC AUC"] - b) <= (n + 6) * 2.0 ** -53 * b and got["F1 Score"] == skm.f1_score(y, p)
