"""CPU: the logistic-regression oracle (tests/logreg_oracle.py) is pinned to scikit-learn by the convexity bound; every logreg entry point's
argument checks and LogisticRegression's Python argument handling work without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
import logreg_oracle as O

ERR_ARG = 1
PROBLEMS = [(200, 10, 0.7), (333, 100, 0.5), (130, 17, 0.7), (65, 100, 0.5), (63, 3, 3.0)]       # the last one is separable


@pytest.mark.parametrize("C", [0.1, 1.0, 10.0])
@pytest.mark.parametrize("n,d,sep", PROBLEMS)
def test_oracle_against_sklearn(n, d, sep, C):
    """|theta_oracle - theta_sklearn|_2 <= 2 |g(theta_oracle) - g(theta_sklearn)|_2 / lambda_min(H(theta_sklearn)) for scikit-learn's
    lbfgs and newton-cholesky at tol = 1e-12, both gradients recomputed by the oracle; and the oracle's own stop is optimal to tol."""
    X, y = O.make_data(n, d, sep, 1)
    classes, t = O.targets(y)
    theta, n_iter, status = O.newton(X, t, C, tol=1e-12, max_iter=100)
    gmax = np.abs(O.gradient(X, t, theta, C)).max()
    print(f"n {n} d {d} C {C}: oracle iterations {n_iter}, status {status}, max |g| {gmax:.3g}")
    assert status == 0 and 0 < n_iter <= 30 and gmax <= 1e-12
    for solver in ("lbfgs", "newton-cholesky"):
        sk, ref = O.sklearn_fit(n, d, sep, C, solver)
        assert np.array_equal(sk.classes_, classes)
        dist, bound = float(np.linalg.norm(theta - ref)), O.distance_bound(X, t, theta, ref, C)
        print(f"    {solver}: |d theta| {dist:.3g}, bound {bound:.3g}, scikit-learn's max |g| {np.abs(O.gradient(X, t, ref, C)).max():.3g}")
        assert dist <= bound


def test_oracle_evaluation():
    """The gradient and Hessian are the derivatives of the loss (central differences), everything stays finite at |z| = 800, and the
    residual keeps its digits where 1 / (1 + exp(-z)) - t cancels."""
    X, y = O.make_data(65, 17, 0.7, 1)
    _, t = O.targets(y)
    rs = np.random.RandomState(0)
    theta = 0.3 * rs.randn(18)
    f, g, H = O.evaluate(X, t, theta, 1.0)
    h = 1e-5
    for k in (0, 5, 17):
        e = np.zeros(18)
        e[k] = h
        fp, gp, _ = O.evaluate(X, t, theta + e, 1.0)
        fm, gm, _ = O.evaluate(X, t, theta - e, 1.0)
        assert abs((fp - fm) / (2 * h) - g[k]) <= 1e-8
        assert np.abs((gp - gm) / (2 * h) - H[k]).max() <= 1e-8
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-16
    z = O.rows(X, t, theta)[0]
    big = theta * (800.0 / np.abs(z).max())
    fb, gb, Hb = O.evaluate(X, t, big, 1.0)
    assert np.isfinite(fb) and np.isfinite(gb).all() and np.isfinite(Hb).all()
    zz, loss, r, w = O.rows(np.array([[40.0]]), np.array([1.0]), np.array([1.0, 0.0]))
    assert abs(r[0] + np.exp(-40.0)) <= 4 * O.U53 * np.exp(-40.0) and 1.0 / (1.0 + np.exp(-40.0)) - 1.0 == 0.0


def test_oracle_solver_rules():
    """max_iter stops with status 1 after that many accepted steps; without the intercept theta has d entries; a start that is already
    optimal takes no step."""
    X, y = O.make_data(63, 3, 3.0, 1)
    _, t = O.targets(y)
    theta, n_iter, status = O.newton(X, t, 10.0, tol=1e-10, max_iter=2)
    assert (n_iter, status) == (2, 1) and np.abs(theta).max() > 0
    theta, n_iter, status = O.newton(X, t, 1.0, tol=1e-10, fit_intercept=False)
    assert status == 0 and theta.shape == (3,) and np.abs(O.gradient(X, t, theta, 1.0, False)).max() <= 1e-10
    assert O.newton(X, t, 1.0, tol=100.0)[1:] == (0, 0)


def _problem(**kw):
    base = dict(X=4096, x_dtype=1, ld=100, n=130, d=100, t=4096, C=1.0, tol=1e-4, fit_intercept=1, max_iter=100, theta=4096, trial=4096, state=4096,
                flags=4096)
    base.update(kw)
    return _lib.LogregProblem(**base)


BAD_PROBLEMS = ((dict(n=0), b"positive"), (dict(d=0), b"positive"), (dict(n=-1), b"positive"), (dict(d=256), b"exceeds"), (dict(x_dtype=2), b"dtype"),
                (dict(x_dtype=-1), b"dtype"), (dict(X=None), b"null"), (dict(t=None), b"null"), (dict(theta=None), b"null"), (dict(trial=None), b"null"),
                (dict(state=None), b"null"), (dict(flags=None), b"null"), (dict(ld=99), b"leading"), (dict(C=0.0), b"C "), (dict(C=-1.0), b"C "),
                (dict(C=float("inf")), b"C "), (dict(C=float("nan")), b"C "), (dict(tol=0.0), b"tol"), (dict(tol=-1e-4), b"tol"),
                (dict(tol=float("nan")), b"tol"), (dict(tol=float("inf")), b"tol"), (dict(fit_intercept=2), b"fit_intercept"),
                (dict(max_iter=0), b"max_iter"))


def test_logreg_entry_points_validate_before_touching_the_gpu():
    """Pointers are the fake address 4096: validation comes first and none is dereferenced."""
    L = _lib.lib()
    rounds = lambda r=4, **kw: L.bbbp_logreg_rounds(None, ctypes.byref(_problem(**kw)), 1, r)  # noqa: E731
    evaluate = lambda **kw: L.bbbp_logreg_eval(None, ctypes.byref(_problem(**kw)))  # noqa: E731
    for bad, word in BAD_PROBLEMS:
        assert rounds(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
        assert evaluate(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert rounds(r=0) == ERR_ARG and b"rounds" in L.bbbp_last_error()
    assert rounds(r=(1 << 16) + 1) == ERR_ARG and b"rounds" in L.bbbp_last_error()
    assert L.bbbp_logreg_rounds(None, None, 1, 4) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_logreg_rounds(None, ctypes.byref(_problem()), 0, 4) == ERR_ARG and b"n_problems" in L.bbbp_last_error()
    two = (_lib.LogregProblem * 2)(_problem(), _problem(C=-1.0))                  # the second of a batch is examined too
    assert L.bbbp_logreg_rounds(None, two, 2, 4) == ERR_ARG and b"problem 1" in L.bbbp_last_error()
    assert L.bbbp_logreg_eval(None, None) == ERR_ARG and b"null" in L.bbbp_last_error()

    dec = lambda X=4096, x_dtype=0, ld=100, m=7, d=100, theta=4096, fit=1, out=4096: L.bbbp_logreg_decision(None, X, x_dtype, ld, m, d, theta, fit, out)  # noqa: E731
    for bad, word in ((dict(m=0), b"positive"), (dict(d=0), b"positive"), (dict(d=256, ld=256), b"exceeds"), (dict(x_dtype=2), b"dtype"), (dict(X=None), b"null"),
                      (dict(theta=None), b"null"), (dict(out=None), b"null"), (dict(ld=99), b"leading"), (dict(fit=2), b"fit_intercept")):
        assert dec(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad

    # the state's size and layout depend on n and d alone
    nbytes = L.bbbp_logreg_state_bytes
    assert nbytes(0, 3) == 0 and b"positive" in L.bbbp_last_error()
    assert nbytes(3, 0) == 0 and nbytes(3, 256) == 0 and b"exceeds" in L.bbbp_last_error()
    assert nbytes(1, 1) > 0 and nbytes(333, 100) % 8 == 0
    assert nbytes(513, 65) - nbytes(512, 65) >= 3 * 4096 * 8                     # one more row slab: three more 64 x 64 tile partials
    off = (ctypes.c_long * 6)()
    assert L.bbbp_logreg_state_layout(130, 17, off) == 0
    assert list(off)[2:5] == [off[2], off[2] + 130, off[2] + 260] and off[5] * 8 + 8 * 18 * 19 // 2 <= nbytes(130, 17)
    assert L.bbbp_logreg_state_layout(130, 17, None) == ERR_ARG and L.bbbp_logreg_state_layout(0, 17, off) == ERR_ARG


def test_logistic_regression_argument_handling():
    from bbbp_amd.linear_model import LogisticRegression, grid_search_cv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LogisticRegression(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LogisticRegression().fit(torch.zeros(8, 4), [0, 1] * 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"C": [1.0]}, device="cpu")
    for kw in (dict(penalty="l1"), dict(penalty="elasticnet"), dict(penalty=None), dict(class_weight="balanced"), dict(class_weight={0: 2.0}),
               dict(multi_class="multinomial"), dict(multi_class="ovr"), dict(solver="liblinear"), dict(solver="saga"), dict(dual=True), dict(l1_ratio=0.5),
               dict(warm_start=True), dict(n_jobs=2), dict(C=0), dict(C=-1.0), dict(C="1"), dict(C=float("inf")), dict(C=True), dict(tol=0.0),
               dict(tol=None), dict(max_iter=0), dict(max_iter=-1), dict(max_iter=2.5), dict(fit_intercept=1)):
        with pytest.raises(ValueError):
            LogisticRegression(**kw)
    with pytest.raises(ValueError, match="penalty"):
        LogisticRegression(penalty="l1")
    clf = LogisticRegression(C=10, tol=1e-6, max_iter=7, fit_intercept=False, solver="newton-cholesky")
    assert (clf.C, clf.tol, clf.max_iter, clf.fit_intercept, clf.penalty, clf.solver) == (10.0, 1e-6, 7, False, "l2", "newton-cholesky")
    assert LogisticRegression().solver == "lbfgs"
    with pytest.raises(ValueError, match="sample weights"):
        LogisticRegression().fit(np.zeros((4, 2)), [0, 1, 0, 1], sample_weight=np.ones(4))
    with pytest.raises(ValueError, match="classes"):
        LogisticRegression().fit(np.zeros((6, 2)), [0, 1, 2, 0, 1, 2])
    with pytest.raises(ValueError, match="classes"):
        LogisticRegression().fit(np.zeros((6, 2)), np.zeros(6))
    with pytest.raises(ValueError, match="1-D"):
        LogisticRegression().fit(np.zeros((4, 2)), np.zeros((4, 2)))
    for method in ("decision_function", "predict", "predict_proba", "predict_log_proba"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(LogisticRegression(), method)(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="grid keys"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"C": [1.0], "solver": ["lbfgs"]})
    with pytest.raises(ValueError, match="penalty"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"C": [1.0], "penalty": ["l1"]})
    with pytest.raises(ValueError, match="C must"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, [{"C": [1.0]}, {"C": [0.0], "penalty": ["l2"]}])
    with pytest.raises(ValueError, match="empty"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, [])
    with pytest.raises(ValueError, match="classes"):
        grid_search_cv(np.zeros((10, 2)), np.arange(10), {"C": [1.0]})
    with pytest.raises(ValueError, match="rows"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 4, {"C": [1.0]})
