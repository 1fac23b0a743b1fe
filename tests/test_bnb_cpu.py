"""CPU: the numpy restatement of Bernoulli naive Bayes (tests/bnb_numpy.py) and the host bookkeeping of bbbp_amd.naive_bayes, pinned to
scikit-learn 1.7's ``BernoulliNB``, ``GridSearchCV`` and ``learning_curve``.  The host paths run on the restatement's ``count`` / ``jll``
callables here; tests/test_gpu_bnb.py holds the device's callables to the same restatement bit for bit.

The bound on a joint log-likelihood.  Both sides form, per row and class, the float64 sum of the same terms: ``w_kj`` for the set
features j (at most d of them; scikit-learn's products ``1.0 * w_kj`` and ``0.0 * w_kj`` are exact and a zero term changes no partial
sum) and ``c_k`` last -- the same float64 ``c_k`` on both sides, since the tables are bit-equal (test 1).  Recursive summation of m terms
in ANY order has the error bound ``gamma_(m-1) sum|x_i|`` with ``gamma_k = k u / (1 - k u)``, ``u = 2^-53`` (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2); a fused multiply-add by an exact 1.0 rounds once like the addition.  With m <= d + 1
each side is within ``gamma_d S`` of the exact sum, ``S = sum over set j of |w_kj| + |c_k|``, so the two differ by at most
``2 gamma_d S <= 2 (d + 2) u S`` (``d u`` is far below 1/2 for any d here, so ``gamma_d <= (d + 2) u``).
"""
import warnings

import numpy as np
import pytest

import bnb_numpy as N

SHAPES = [(1000, 100), (257, 65), (64, 7)]
ALPHAS = (0.01, 0.5, 1, 2)
BINARIZE = (0, 0.5, 1)
PRIORS = [dict(fit_prior=True), dict(fit_prior=False), dict(class_prior=[0.3, 0.7])]
MACCS_GRID = {"alpha": [0.01, 0.1, 0.5, 1.0, 2.0], "binarize": [0.0, 0.5, 1.0]}          # model_maccs.py:257-267
OPT_GRID = {"alpha": [0.5, 0.8, 1.0]}                                                    # model_opt_20250130.py:507-510


def _sk(**kw):
    from sklearn.naive_bayes import BernoulliNB
    return BernoulliNB(**kw)


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("n,d", SHAPES)
def test_attributes_equal_sklearn_bit_for_bit(n, d):
    X, y = N.fingerprint_problem(n, d)
    for alpha in ALPHAS:
        for b in BINARIZE:
            for prior in PRIORS:
                sk = _sk(alpha=alpha, binarize=b, **prior).fit(X, y)
                fit = N.Fit(X, y, alpha, b, **prior)
                what = f"alpha {alpha} binarize {b} {prior}"
                assert _bits_equal(sk.feature_count_, fit.fc.astype(np.float64)) and _bits_equal(sk.class_count_, fit.cc.astype(np.float64)), what
                assert _bits_equal(sk.feature_log_prob_, fit.flp), what
                assert _bits_equal(sk.class_log_prior_, fit.prior), what


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_jll_within_the_summation_bound_and_labels_equal(n, d, dtype):
    """Tests 2 and 3: every jll entry within ``2 (d + 2) 2^-53 (sum |w| over the set bits + |c|)`` of scikit-learn's; labels equal on
    every row whose two values differ by more than the sum of their bounds, and at most 1 % of the rows are that close -- counted on
    scikit-learn's values alone."""
    X, y = N.fingerprint_problem(n, d, dtype=dtype)
    for alpha in ALPHAS:
        for b in BINARIZE:
            sk = _sk(alpha=alpha, binarize=b).fit(X, y)
            fit = N.Fit(X, y, alpha, b)
            want, got = sk.predict_joint_log_proba(X), fit.jll(X)
            bound = N.jll_bound(N.binarise(X, b), fit.w, fit.c)
            gap = np.abs(want - got)
            print(f"n {n} d {d} {dtype} alpha {alpha} binarize {b}: max |jll - sklearn| {gap.max():.3e}, smallest bound {bound.min():.3e}")
            assert (gap <= bound).all()
            close = np.abs(want[:, 0] - want[:, 1]) <= bound.sum(axis=1)
            assert close.sum() <= 0.01 * n, "the inputs leave too many rows undecided for scikit-learn itself"
            assert np.array_equal(sk.predict(X)[~close], fit.predict(X)[~close])


def test_labels_of_any_sortable_kind_and_ties_go_to_the_first_class():
    X, y = N.fingerprint_problem(64, 7)
    names = np.where(y == 1, "yes", "no")
    fit = N.Fit(X, names, 1.0, 0.0)
    assert np.array_equal(fit.predict(X), _sk().fit(X, names).predict(X))
    # a constructed exact tie: equal tables and constants for both classes
    w, c = np.tile(fit.w[:1], (2, 1)), np.tile(fit.c[:1], 2)
    s = N.jll(N.binarise(X, 0.0), w, c)
    assert (s[:, 0] == s[:, 1]).all() and (np.argmax(s, axis=1) == 0).all()


def test_float32_threshold_is_rounded_to_the_arrays_dtype():
    """0.1 is not a float32: ``np.float32(0.1)`` lies above it.  scikit-learn compares a float32 X with ``np.float32(threshold)`` (numpy's
    rule for a Python float), so the value ``np.float32(0.1)`` itself is NOT above the threshold 0.1, though as a double it is."""
    t32 = np.float32(0.1)
    assert float(t32) > 0.1
    below, above = np.nextafter(t32, np.float32(-1)), np.nextafter(t32, np.float32(1))
    col = np.array([below, t32, above, 0.0, 1.0, -1.0], dtype=np.float32)
    X32 = np.stack([col, col[::-1]], axis=1)
    from sklearn.preprocessing import binarize
    want = binarize(X32, threshold=0.1).astype(bool)
    assert want[:, 0].tolist() == [False, False, True, False, True, False]
    assert np.array_equal(N.binarise(X32, 0.1), want)
    # the same values as float64 compare with the double 0.1: float32(0.1) is above it
    X64 = X32.astype(np.float64)
    want64 = binarize(X64, threshold=0.1).astype(bool)
    assert want64[:, 0].tolist() == [False, True, True, False, True, False]
    assert np.array_equal(N.binarise(X64, 0.1), want64)
    # and a fitted model's counts follow the rule
    y = np.array([0, 1, 0, 1, 0, 1])
    sk = _sk(binarize=0.1).fit(X32, y)
    assert np.array_equal(sk.feature_count_, N.Fit(X32, y, 1.0, 0.1).fc.astype(np.float64))


def _problem_300():
    return N.fingerprint_problem(300, 20, seed=3)


@pytest.mark.parametrize("grid", [MACCS_GRID, OPT_GRID, [OPT_GRID, {"binarize": [0.5], "fit_prior": [True, False]}], {}],
                         ids=["maccs", "opt", "list", "empty"])          # empty: the other model_opt* scripts' grid
def test_grid_search_equals_sklearn(grid):
    from sklearn.model_selection import GridSearchCV
    from bbbp_amd import naive_bayes as NB
    X, y = _problem_300()
    sk = GridSearchCV(_sk(), grid, cv=5, scoring="f1").fit(X, y)
    best, scores, fitted = NB.grid_search_cv(X, y, grid, cv=5, backend=N.backend)
    assert best == sk.best_params_
    assert np.abs(np.asarray(scores) - sk.cv_results_["mean_test_score"]).max() <= 1e-12
    assert [dict(p) for p in sk.cv_results_["params"]][int(np.argmax(scores))] == best
    # the restatement's plain loops of single fits agree with the batched bookkeeping exactly
    rbest, rscores, rfit = N.grid_search(X, y, grid, cv=5)
    assert rbest == best and np.abs(np.asarray(rscores) - np.asarray(scores)).max() <= 1e-15
    assert _bits_equal(fitted.feature_log_prob_, rfit.flp) and _bits_equal(fitted.feature_log_prob_, sk.best_estimator_.feature_log_prob_)
    assert _bits_equal(fitted.class_log_prior_, sk.best_estimator_.class_log_prior_) and np.array_equal(fitted.classes_, sk.classes_)


@pytest.mark.parametrize("scoring", ["f1", "accuracy"])
def test_learning_curve_equals_sklearn(scoring):
    from sklearn.model_selection import learning_curve
    from bbbp_amd import naive_bayes as NB
    X, y = _problem_300()
    params = dict(alpha=0.5, binarize=0.5)
    sizes, tr, te = learning_curve(_sk(**params), X, y, cv=6, train_sizes=np.linspace(.1, 1, 5), shuffle=False,
                                   **({"scoring": "f1"} if scoring == "f1" else {}))
    got = NB.learning_curve(params, X, y, cv=6, train_sizes=np.linspace(.1, 1, 5), scoring=scoring, backend=N.backend)
    assert np.array_equal(got[0], sizes) and got[1].shape == tr.shape == (5, 6)
    assert np.abs(got[1] - tr).max() <= 1e-12 and np.abs(got[2] - te).max() <= 1e-12
    ref = N.learning_curve(params, X, y, cv=6, train_sizes=np.linspace(.1, 1, 5), scoring=scoring)
    assert np.array_equal(ref[0], sizes) and np.abs(ref[1] - got[1]).max() <= 1e-15 and np.abs(ref[2] - got[2]).max() <= 1e-15


def test_fit_masks_on_the_restatement_equals_single_fits():
    from bbbp_amd import naive_bayes as NB
    X, y = _problem_300()
    rows = [None, np.arange(299, 100, -2), np.array([0, 1]), np.arange(256, 300)]
    rows[3] = np.concatenate([rows[3], [0, 1]])
    models = NB.fit_masks(X, y, rows, [0.0, 0.5, 0.0], [0.5, 2], backend=N.backend)
    assert len(models) == 4 * 3 * 2
    at = 0
    for r in rows:
        Xr, yr = (X, y) if r is None else (X[r], y[r])
        for b in (0.0, 0.5, 0.0):
            for a in (0.5, 2):
                sk, m = _sk(alpha=a, binarize=b).fit(Xr, yr), models[at]
                assert m.alpha == a and m.binarize == b
                assert _bits_equal(m.feature_count_, sk.feature_count_) and _bits_equal(m.class_count_, sk.class_count_)
                assert _bits_equal(m.feature_log_prob_, sk.feature_log_prob_) and _bits_equal(m.class_log_prior_, sk.class_log_prior_)
                at += 1


def test_estimator_surface_without_a_gpu():
    from sklearn.base import clone
    from bbbp_amd import naive_bayes as NB
    import bbbp_amd
    assert bbbp_amd.naive_bayes is NB
    prior = [0.4, 0.6]
    est = NB.BernoulliNB(alpha=0.5, binarize=0.25, fit_prior=False, class_prior=prior)
    twin = clone(est)
    assert twin.get_params() == est.get_params() and twin.class_prior == prior and twin is not est
    assert est.set_params(alpha=2).alpha == 2
    with pytest.raises(ValueError, match="unknown parameters"):
        est.set_params(gamma=1)
    with pytest.raises(RuntimeError, match="not fitted"):
        est.predict(np.zeros((2, 2)))
    # from_sklearn adopts the tables without touching the GPU
    X, y = N.fingerprint_problem(64, 7)
    sk = _sk(alpha=0.5, binarize=0.5).fit(X, y)
    got = NB.BernoulliNB.from_sklearn(sk)
    fit = N.Fit(X, y, 0.5, 0.5)
    assert _bits_equal(got._w, fit.w) and _bits_equal(got._c, fit.c) and got.n_features_in_ == 7 and got.binarize == 0.5


def test_refusals_by_name():
    """Everything the arguments alone decide is a ValueError before the GPU is touched (this machine has none)."""
    import scipy.sparse as sp
    import torch
    from bbbp_amd import naive_bayes as NB
    X, y = (np.array(a) for a in N.fingerprint_problem(64, 7))
    B = NB.BernoulliNB
    with pytest.raises(ValueError, match="3 classes in y, exactly two are supported"):
        B().fit(X, np.arange(64) % 3)
    with pytest.raises(ValueError, match="1 classes in y"):
        B().fit(X, np.zeros(64))
    with pytest.raises(ValueError, match="sample_weight is not supported"):
        B().fit(X, y, sample_weight=np.ones(64))
    with pytest.raises(ValueError, match="sample_weight is not supported"):
        B().score(X, y, sample_weight=np.ones(64))
    with pytest.raises(ValueError, match="partial_fit is not supported"):
        B().partial_fit(X, y, classes=[0, 1])
    with pytest.raises(ValueError, match="binarize=None is not supported"):
        B(binarize=None)
    with pytest.raises(ValueError, match="binarize must be a finite number"):
        B(binarize=float("nan"))
    with pytest.raises(ValueError, match="sparse input is not supported"):
        B().fit(sp.csr_matrix(X), y)
    with pytest.raises(ValueError, match="sparse input is not supported"):
        B().fit(torch.from_numpy(X).to_sparse(), y)
    for prior in ([0.5], [0.2, 0.3, 0.5], [0.0, 1.0], [-1.0, 2.0], [float("nan"), 1.0], "ab"):
        with pytest.raises(ValueError, match="class_prior must be two positive numbers"):
            B(class_prior=prior)
    for alpha in (-0.1, float("inf"), float("nan"), [1.0, 2.0], np.ones(7), "1", None, True):
        with pytest.raises(ValueError, match="alpha must be one finite number >= 0"):
            B(alpha=alpha)
    with pytest.raises(ValueError, match="alpha must be one finite number"):
        B().set_params(alpha=-1)
    for fn in (lambda: B(device="cpu"), lambda: NB.fit_masks(X, y, [None], [0.0], [1.0], device="cpu"),
               lambda: NB.grid_search_cv(X, y, OPT_GRID, device="cpu"), lambda: NB.learning_curve({}, X, y, device="cpu"),
               lambda: NB.BernoulliNB.from_sklearn(_sk().fit(X, y), device="cpu")):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn()
    with pytest.raises(ValueError, match="expected a 2-D"):
        B().fit(X[0], y)
    with pytest.raises(ValueError, match="X has 64 rows, y has 63"):
        B().fit(X, y[:63])
    # row subsets
    zeros = np.flatnonzero(y == 0)
    with pytest.raises(ValueError, match="lacks one of the two classes"):
        NB.fit_masks(X, y, [None, zeros], [0.0], [1.0])
    with pytest.raises(ValueError, match="repeats a row"):
        NB.fit_masks(X, y, [np.array([0, 1, 1])], [0.0], [1.0])
    with pytest.raises(ValueError, match="is empty or leaves"):
        NB.fit_masks(X, y, [np.array([0, 64])], [0.0], [1.0])
    with pytest.raises(ValueError, match="alpha must be one finite number"):
        NB.fit_masks(X, y, [None], [0.0], [[1.0, 2.0]])
    with pytest.raises(ValueError, match="binarize=None"):
        NB.fit_masks(X, y, [None], [None], [1.0])
    with pytest.raises(ValueError, match="unsupported grid keys"):
        NB.grid_search_cv(X, y, {"class_prior": [None]})
    with pytest.raises(ValueError, match="scoring must be 'f1' or 'accuracy'"):
        NB.learning_curve({}, X, y, scoring="roc_auc")
    # a fit whose tables are not finite: feature 0 is set in every row of class 1 and alpha is too small to keep log(1 - p) finite
    Xs = np.array(X)
    Xs[:, 0] = np.where(y == 1, 1.0, -1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not np.isfinite(_sk(alpha=1e-20).fit(Xs, y).predict_joint_log_proba(Xs)).all()      # what scikit-learn hands out there
    with pytest.raises(ValueError, match="the fitted tables are not finite"):
        NB.fit_masks(Xs, y, [None], [0.0], [1e-20], backend=N.backend)
    with pytest.raises(ValueError, match="the fitted tables are not finite"):
        NB.fit_masks(Xs, y, [None], [0.0], [0.0], backend=N.backend)
