"""CPU: the host side of ``bbbp_amd.metrics`` and the numpy restatement of its device side against scikit-learn 1.7.

* ``scores_from_counts`` reproduces scikit-learn's seven count scores bit for bit on a seeded sweep of two-class problems.
* The restatement's AUC, ``U2 / (2 P N)`` rounded once, against ``roc_auc_score`` within ``(n + 6) 2^-53 b`` (derived below).
* The restatement's MSE and R2 against scikit-learn within the summation bounds derived beside their constants.
* The wrappers' argument checks: every ``NotImplementedError`` / ``ValueError`` path that needs no device.
"""
import warnings

import numpy as np
import pytest
import sklearn.metrics as skm

import metrics_numpy as R
from bbbp_amd import metrics

U = 2.0 ** -53
COUNT_KEYS = ("Accuracy", "Balanced Accuracy", "Precision", "Recall", "F1 Score", "MCC", "Cohen's Kappa")


def _sklearn_seven(y, p, pos_label, zero_division):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return {"Accuracy": skm.accuracy_score(y, p), "Balanced Accuracy": skm.balanced_accuracy_score(y, p),
                "Precision": skm.precision_score(y, p, pos_label=pos_label, zero_division=zero_division),
                "Recall": skm.recall_score(y, p, pos_label=pos_label, zero_division=zero_division),
                "F1 Score": skm.f1_score(y, p, pos_label=pos_label, zero_division=zero_division),
                "MCC": skm.matthews_corrcoef(y, p), "Cohen's Kappa": skm.cohen_kappa_score(y, p)}


def _sweep():
    """2 400 seeded two-class problems, n from 2 to 400; every tenth of each special kind."""
    rs = np.random.RandomState(20250130)
    for it in range(2400):
        n = int(rs.randint(2, 401))
        y, p = rs.randint(0, 2, n), (rs.rand(n) < rs.rand()).astype(np.int64)
        kind = it % 12
        if kind == 0:
            p[:] = 0                            # constant predictions of either class
        elif kind == 1:
            p[:] = 1
        elif kind == 2:
            p = y.copy()                        # perfect
        elif kind == 3:
            p = 1 - y                           # fully inverted
        elif kind == 4:
            p[y == 1] = 0                       # tp = 0
        elif kind == 5:
            y[:] = 1                            # y_true of one class
        elif kind == 6:
            y[:] = 0
        yield it, y, p


def test_count_scores_equal_scikit_learn_bit_for_bit():
    seen = 0
    for it, y, p in _sweep():
        zero_division = ("warn", 0, 1)[it % 3]
        if it % 2:                              # labels {-1, 1} and {0, 1}
            y, p = 2 * y - 1, 2 * p - 1
        got = metrics.scores_from_counts(R.confusion_counts(y == 1, p == 1)[0, 0], zero_division)
        want = _sklearn_seven(y, p, 1, zero_division)
        for key in COUNT_KEYS:
            a, b = np.float64(got[key]), np.float64(want[key])
            assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (it, key, a, b)
        seen += 1
    assert seen >= 2000


def test_count_scores_are_elementwise_and_empty_is_nan():
    counts = np.array([[[3, 1, 2, 4], [0, 0, 0, 0]], [[0, 0, 0, 7], [5, 0, 0, 0]]])
    got = metrics.scores_from_counts(counts)
    for key in COUNT_KEYS:
        assert got[key].shape == (2, 2) and got[key].dtype == np.float64
        assert np.isnan(got[key][0, 1])
        for at in [(0, 0), (1, 0), (1, 1)]:
            one = metrics.scores_from_counts(counts[at])[key]
            assert R.bits(one) == R.bits(got[key][at]) or (np.isnan(one) and np.isnan(got[key][at]))
    with pytest.raises(ValueError):
        metrics.scores_from_counts(np.zeros((2, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        metrics.scores_from_counts(np.zeros(4))
    with pytest.raises(ValueError):
        metrics.scores_from_counts(np.array([1, 1, 1, 1]), zero_division=0.5)


def test_degenerate_cases_follow_scikit_learn():
    """Pinned to scikit-learn 1.7: balanced accuracy with a class absent from y_true is the recall of the class that is there (the NaN
    recall is dropped with a warning); MCC with a zero factor is 0; precision without a predicted positive is ``zero_division``; kappa
    of one label is NaN."""
    y, p = np.array([1, 1, 1, 1]), np.array([1, 0, 1, 1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert skm.balanced_accuracy_score(y, p) == 0.75
    got = metrics.scores_from_counts(R.confusion_counts(y, p)[0, 0])
    assert got["Balanced Accuracy"] == 0.75 and got["MCC"] == 0.0
    got = metrics.scores_from_counts(np.array([3, 0, 2, 0]), zero_division=1)
    assert got["Precision"] == 1.0 and got["Recall"] == 0.0 and got["F1 Score"] == 0.0
    assert np.isnan(metrics.scores_from_counts(np.array([0, 0, 0, 5]))["Cohen's Kappa"])
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        assert np.isnan(skm.cohen_kappa_score([1] * 5, [1] * 5))


def _auc_cases():
    rs = np.random.RandomState(7)
    for it in range(600):
        n = int(rs.randint(2, 3001)) if it % 20 == 0 else int(rs.randint(2, 401))
        y = rs.randint(0, 2, n)
        if y.min() == y.max():
            y[0] = 1 - y[0]
        kind = it % 8
        s = rs.rand(n) + 0.3 * y
        if kind == 0:
            s = np.full(n, 0.5)                                         # all equal
        elif kind == 1:
            s = rs.choice([0.25, 0.75], n)                              # two distinct values
        elif kind == 2:
            s = rs.choice([0.0, -0.0, 1.0], n)                          # +-0.0 compare equal
        elif kind == 3:
            s = rs.choice([5e-324, 2.5e-310, 1e308, -1e308, 0.0], n)    # denormals and huge values
        elif kind == 4:
            s = s.astype(np.float32)
        elif kind == 5:
            s = (s > 0.6).astype(np.float64)                            # hard 0/1 "scores"
        elif kind == 6:
            s = np.round(s * 4) / 4                                     # heavily tied
        yield it, y, s


def test_auc_of_the_restatement_against_scikit_learn():
    """|a - b| <= (n + 6) 2^-53 b.  a is the exact value U2 / (2 P N) rounded once (relative error 2^-53).  b is scikit-learn's trapezoid
    sum: at most n + 1 non-negative terms width * (h0 + h1) / 2, each of three roundings on exact or once-rounded operands, summed in
    some order: a sum of k non-negative terms is off by at most (k - 1) 2^-53 relatively, the terms by 3 2^-53, fpr and tpr by one
    division each -- n + 5 roundings, and one more for a.  A wrong pair count moves the value by at least 1 / (2 P N) >= 2 / n^2.
    Largest deviation seen in this sweep: 2 ulp."""
    worst = 0.0
    for it, y, s in _auc_cases():
        n = len(y)
        pairs = R.pair_counts(y, s)[0, 0]
        a = float(metrics.auc_from_pairs(*pairs))
        with np.errstate(all="ignore"):                                  # scikit-learn differences 1e308 and -1e308 on its way
            b = skm.roc_auc_score(y, s)
        assert abs(a - b) <= (n + 6) * U * b, (it, a, b)
        if b > 0:
            worst = max(worst, abs(a - b) / np.spacing(b))
        if it % 8 == 5:                                                  # hard predictions: the pair count follows from the confusion counts
            u2, pos, neg = metrics.pairs_from_counts(R.confusion_counts(y, s)[0, 0])
            assert (int(u2), int(pos), int(neg)) == tuple(int(v) for v in pairs)
    print(f"largest |AUC - roc_auc_score| seen: {worst:.1f} ulp")
    assert worst <= 8


def test_auc_of_one_class_is_nan():
    assert np.isnan(metrics.auc_from_pairs(0, 5, 0)) and np.isnan(metrics.auc_from_pairs(0, 0, 5))
    assert metrics.auc_from_pairs(2 * 3 * 4, 3, 4) == 1.0


def test_regression_sums_of_the_restatement_against_scikit_learn():
    """MSE: both sides add the same n non-negative terms fl(fl(y - p)^2) in different orders (relative error (n - 1) 2^-53 each) and
    divide once: |a - b| <= (2 n + 2) 2^-53 b.  R2 = 1 - q, q = num / den: num as above; den's terms fl(fl(y - m)^2) carry three
    roundings on top of the exact (y - m)^2 and the two means differ by at most 2 n 2^-53 max|y|, which moves den by n delta^2 only (the
    first-order term sums to zero) -- asserted below to stay under 2^-53 den; so each q is within (2 n + 4) 2^-53 and the difference of
    the R2 within (4 n + 8) 2^-53 q + 2^-52 |R2| (the last for the two subtractions)."""
    rs = np.random.RandomState(3)
    for it in range(200):
        n = int(rs.randint(2, 1200))
        y = rs.randn(n) * 2.0 + 1.0
        p = (y + rs.randn(n) * 0.5).astype(np.float32 if it % 2 else np.float64)
        sse, ystat = R.squared_error_sums(y, p)
        got = metrics.regression_from_sums(sse, ystat)
        mse, r2 = skm.mean_squared_error(y, p.astype(np.float64)), skm.r2_score(y, p.astype(np.float64))
        assert abs(got["MSE"][0, 0] - mse) <= (2 * n + 2) * U * mse
        den = float(np.sum((y - y.mean()) ** 2))
        assert n * (2 * n * U * np.abs(y).max()) ** 2 <= U * den
        q = sse[0, 0] / den
        assert abs(got["R2"][0, 0] - r2) <= (4 * n + 8) * U * q + 2 * U * abs(r2)


def test_regression_degenerate_cases_follow_scikit_learn():
    y = np.full(9, 2.5)
    for p in (y.copy(), y + 1.0):
        got = metrics.regression_from_sums(*R.squared_error_sums(y, p))
        assert got["R2"][0, 0] == skm.r2_score(y, p) and got["MSE"][0, 0] == skm.mean_squared_error(y, p)
    got = metrics.regression_from_sums(np.zeros((1, 2)), np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0]]))
    assert np.isnan(got["MSE"][0, 0]) and np.isnan(got["R2"][0, 0]) and got["MSE"][0, 1] == 0.0 and np.isnan(got["R2"][0, 1])


def test_the_restatement_sums_in_the_stated_order():
    rs = np.random.RandomState(5)
    t = rs.randn(700)
    inc = rs.rand(700) < 0.8
    lanes = [0.0] * 256
    for i, (v, k) in enumerate(zip(t, inc)):
        if k:
            lanes[i % 256] = lanes[i % 256] + v
    waves = []
    for w in range(4):
        v = lanes[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            v = [v[k] + v[k + off] if k + off < len(v) else v[k] for k in range(len(v))]
        waves.append(v[0])
    assert ((waves[0] + waves[1]) + waves[2]) + waves[3] == R.fixed_order_sum(t, inc)


Y = np.array([0, 1, 1, 0, 1])
P = np.array([0, 1, 0, 0, 1])


@pytest.mark.parametrize("call", [
    lambda: metrics.accuracy_score(Y, P, sample_weight=np.ones(5)),
    lambda: metrics.accuracy_score(Y, P, normalize=False),
    lambda: metrics.balanced_accuracy_score(Y, P, adjusted=True),
    lambda: metrics.balanced_accuracy_score(Y, P, sample_weight=np.ones(5)),
    lambda: metrics.precision_score(Y, P, average="macro"),
    lambda: metrics.recall_score(Y, P, average=None),
    lambda: metrics.f1_score(Y, P, average="weighted"),
    lambda: metrics.f1_score(Y, P, sample_weight=np.ones(5)),
    lambda: metrics.f1_score(Y, P, labels=[0, 1]),
    lambda: metrics.matthews_corrcoef(Y, P, sample_weight=np.ones(5)),
    lambda: metrics.cohen_kappa_score(Y, P, weights="linear"),
    lambda: metrics.cohen_kappa_score(Y, P, sample_weight=np.ones(5)),
    lambda: metrics.roc_auc_score(Y, P * 0.5, max_fpr=0.1),
    lambda: metrics.roc_auc_score(Y, P * 0.5, sample_weight=np.ones(5)),
    lambda: metrics.roc_auc_score(Y, P * 0.5, average="weighted"),
    lambda: metrics.roc_auc_score(Y, np.zeros((5, 2))),
    lambda: metrics.confusion_matrix(Y, P, normalize="all"),
    lambda: metrics.confusion_matrix(Y, P, labels=[1, 0]),
    lambda: metrics.mean_squared_error(Y, P, sample_weight=np.ones(5)),
    lambda: metrics.mean_squared_error(Y, P, multioutput="raw_values"),
    lambda: metrics.r2_score(Y, P, multioutput="variance_weighted"),
    lambda: metrics.r2_score(Y, P, force_finite=False),
    lambda: metrics.f1_score(np.zeros((5, 2)), P),
    lambda: metrics.f1_score(Y, np.zeros((5, 2))),
    lambda: metrics.mean_squared_error(np.zeros((5, 2)), np.zeros((5, 2))),
])
def test_what_is_not_built_is_refused_by_name(call):
    with pytest.raises(NotImplementedError):
        call()


@pytest.mark.parametrize("call", [
    lambda: metrics.f1_score(Y, np.array([0, 1, 2, 0, 1])),                              # more than two classes
    lambda: metrics.accuracy_score(np.array([0, 1, 2, 0, 1]), P),
    lambda: metrics.f1_score(Y, P, pos_label=2),                                         # pos_label not among the classes
    lambda: metrics.precision_score(Y, P, zero_division=0.5),
    lambda: metrics.f1_score(Y, P[:4]),                                                  # lengths
    lambda: metrics.f1_score(np.array([0.0, np.nan, 1.0, 0.0, 1.0]), P),                 # NaN in y_true
    lambda: metrics.classification_scores(Y, P, device="cpu"),                           # no CPU path
    lambda: metrics.classification_scores(Y, P, groups=np.array([0, 0, -2, 1, 1])),
    lambda: metrics.classification_scores(Y, P, groups=np.array([0, 0, 70, 1, 1])),      # BBBP_METRICS_MAX_GROUPS
    lambda: metrics.classification_scores(Y, P, groups=np.array([0.0, 0, 0, 1, 1])),
    lambda: metrics.classification_scores(Y, np.zeros((2, 2, 5))),
    lambda: metrics.confusion_counts(Y, P * 0.5, threshold=np.nan),
    lambda: metrics.regression_scores(Y, P, device="cpu"),
    lambda: metrics.regression_scores(np.array(["a", "b"]), np.zeros(2)),
    lambda: metrics.evaluate_models([], np.zeros((5, 2)), Y),
])
def test_invalid_arguments_raise_value_error(call):
    with pytest.raises(ValueError):
        call()


def test_roc_auc_of_one_class_warns_and_is_nan_without_a_device():
    with pytest.warns(metrics.UndefinedMetricWarning):
        assert np.isnan(metrics.roc_auc_score(np.ones(5), np.linspace(0, 1, 5)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(skm.roc_auc_score(np.ones(5), np.linspace(0, 1, 5)))
    from sklearn.exceptions import UndefinedMetricWarning
    assert metrics.UndefinedMetricWarning is UndefinedMetricWarning


def test_the_package_exports_the_module_and_the_eight_keys():
    import bbbp_amd
    assert bbbp_amd.metrics is metrics and "metrics" in bbbp_amd.__all__
    assert metrics.KEYS == ("Accuracy", "Balanced Accuracy", "Precision", "Recall", "F1 Score", "MCC", "Cohen's Kappa", "ROC AUC")
