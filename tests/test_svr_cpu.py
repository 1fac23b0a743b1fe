"""CPU: the SVR oracle (tests/svr_oracle.py) is pinned to scikit-learn's libsvm epsilon-SVR; bbbp_svr_smo's argument checks and SVR's
Python argument handling work without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
import svr_oracle as O

ERR_ARG = 1
NOISE = 0.3
# (n, d, kernel, C, epsilon)
CASES = [(300, 10, "rbf", 1.0, 0.1), (300, 10, "rbf", 10.0, 0.05), (130, 7, "rbf", 0.1, 0.5), (200, 10, "linear", 0.1, 0.2), (333, 100, "rbf", 1.0, 0.1)]


@pytest.mark.parametrize("n,d,kind,C,epsilon", CASES)
def test_oracle_against_sklearn(n, d, kind, C, epsilon):
    """The same support set; intercept_ and 200 held-out predictions within 4 x scikit-learn's own scatter (at least 10 tol), measured by
    svr_oracle.sklearn_reference.  dual_coef_ is not pinned: along a flat direction of the dual two correct runs differ by far more than
    their predictions do.  The solution the oracle stops at is optimal to tol by its own recomputation from alpha."""
    sk, want, tolerance = O.sklearn_reference(n, d, NOISE, kind, C, epsilon)
    X, t = O.make_data(n, d, NOISE, 1)
    Q, _ = O.make_data(200, d, NOISE, 2)
    g = O.gamma_scale(X)
    assert abs(g - sk._gamma) <= 1e-15 * g
    m = O.fit(X, t, C, epsilon, kind, g, tol=1e-3)
    got = O.predict(Q, X, m, kind, g)
    print(f"n {n} d {d} {kind} C {C} epsilon {epsilon}: tolerance {tolerance:.3g}, iterations {m['n_iter_']} (scikit-learn {int(np.ravel(sk.n_iter_)[0])}), "
          f"prediction difference {np.abs(got - want).max():.3g}, intercept difference {abs(m['intercept_'][0] - sk.intercept_[0]):.3g}")
    assert m["converged"]
    assert np.array_equal(m["support_"], sk.support_)
    assert abs(m["intercept_"][0] - sk.intercept_[0]) <= tolerance
    assert np.abs(got - want).max() <= tolerance
    _check_optimal(O.kernel(X, X, kind, g), t, m, C, epsilon, 1e-3)


def _check_optimal(K, t, m, C, epsilon, tol):
    alpha, n = m["alpha"], len(t)
    assert alpha.shape == (2 * n,) and (alpha >= 0.0).all() and (alpha <= C).all()
    assert abs(alpha[:n].sum() - alpha[n:].sum()) <= 2 * n * C * O.U53 * 4
    gap, G = O.violation(K, t, alpha, C, epsilon)
    assert gap <= tol * (1 + 1e-6) + 1e-9
    s = O.signs(n)
    want = O.rho_rule(s, G, alpha, C)                                   # svc_oracle's rule, numpy's own sum, G recomputed from alpha
    assert abs(-m["intercept_"][0] - want) <= 1e-9
    assert np.array_equal(m["dual_coef_"][0], (alpha[:n] - alpha[n:])[m["support_"]])


def test_oracle_optimality_at_a_tight_tolerance_and_epsilon_zero():
    X, t = O.make_data(130, 7, NOISE, 1)
    g = O.gamma_scale(X)
    K = O.kernel(X, X, "rbf", g)
    for C, epsilon, tol in ((1.0, 0.1, 1e-8), (1.0, 0.0, 1e-3), (0.1, 0.5, 1e-8)):
        alpha, rho, n_iter, ok = O.smo(K, t, C, epsilon, tol)
        assert ok and n_iter > 0
        _check_optimal(K, t, O.attributes(alpha, rho, n_iter, ok), C, epsilon, tol)
    assert len(O.attributes(*O.smo(K, t, 1.0, 0.0))["support_"]) == 130       # epsilon = 0: every row off its target is a support vector


def test_rho_tree_is_rho_rule_to_rounding():
    """The kernel's fixed summation order against numpy's pairwise sum, with and without free variables, below and above 1024 rows."""
    rs = np.random.RandomState(7)
    for n in (1, 63, 1024, 1025, 2500):
        s, G = O.signs(n), rs.randn(2 * n)
        for alpha in (rs.rand(2 * n) * (rs.rand(2 * n) < 0.5), np.where(rs.rand(2 * n) < 0.5, 0.0, 1.0)):
            got, want = O.rho_tree(s, G, alpha, 1.0), O.rho_rule(s, G, alpha, 1.0)
            free = (alpha > 0) & (alpha < 1.0)
            assert abs(got - want) <= 2 * (2 * n + 1) * O.U53 * max(np.abs(G[free]).sum() / max(free.sum(), 1), abs(want))


def test_oracle_ties_keep_the_later_index():
    """Every (row, target) twice: a row and its copy tie exactly in both selections of the first iteration (G = epsilon -+ t, and a kernel
    value depends on its two rows' values only), and libsvm's scans keep the later index: the moved pair are the later copies.  At
    alpha = 0 the first half alone is I_up and the second alone I_low, so the first iteration cannot tie a variable k with k + n; the
    selection is a later arg-max over the 2n ordering, in which k + n wins an exact tie with k."""
    X, t = O.make_data(40, 4, NOISE, 3)
    X2, t2 = np.concatenate([X, X]), np.concatenate([t, t])
    K = O.kernel(X2, X2, "rbf", 0.25)
    alpha, _, n_iter, ok = O.smo(K, t2, 1.0, 0.1, max_iter=1)
    assert n_iter == 1 and not ok
    moved = np.flatnonzero(alpha > 0)
    assert len(moved) == 2 and moved[0] in range(40, 80) and moved[1] in range(80 + 40, 160)
    assert O.smo(K, t2, 1.0, 0.1, max_iter=5)[2] == 5
    v = np.full(160, -1.0)
    v[[3, 80 + 3]] = 0.5                                 # variable 3 and variable 3 + n with the same bits
    assert O._later_argmax(v) == 80 + 3


def _problem(**kw):
    base = dict(K=4096, ldk=100, rows=None, t=4096, alpha=4096, grad=4096, diag=4096, rho=4096, n_iter=4096, done=4096, n=100, C=1.0, epsilon=0.1,
                tol=1e-3)
    base.update(kw)
    return _lib.SvrProblem(**base)


def test_svr_smo_validates_before_touching_the_gpu():
    """Pointers are the fake address 4096: validation comes first and none is dereferenced."""
    L = _lib.lib()
    one = lambda iters=100, **kw: L.bbbp_svr_smo(None, ctypes.byref(_problem(**kw)), 1, iters)  # noqa: E731
    for bad, word in ((dict(n=0), b"positive"), (dict(n=-3), b"positive"), (dict(n=(1 << 30) + 1), b"at most"), (dict(K=None), b"null"), (dict(t=None), b"null"),
                      (dict(alpha=None), b"null"), (dict(grad=None), b"null"), (dict(diag=None), b"null"), (dict(rho=None), b"null"),
                      (dict(n_iter=None), b"null"), (dict(done=None), b"null"), (dict(ldk=99), b"leading"), (dict(rows=4096, ldk=0), b"leading"),
                      (dict(C=0.0), b"C "), (dict(C=-1.0), b"C "), (dict(C=float("inf")), b"C "), (dict(C=float("nan")), b"C "), (dict(tol=0.0), b"tol"),
                      (dict(tol=float("nan")), b"tol"), (dict(tol=float("inf")), b"tol"), (dict(epsilon=-1e-300), b"epsilon"),
                      (dict(epsilon=float("inf")), b"epsilon"), (dict(epsilon=float("nan")), b"epsilon")):
        assert one(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert one(iters=0) == ERR_ARG and b"iters" in L.bbbp_last_error()
    assert one(iters=(1 << 20) + 1) == ERR_ARG and b"iters" in L.bbbp_last_error()
    assert L.bbbp_svr_smo(None, None, 1, 100) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_svr_smo(None, ctypes.byref(_problem()), 0, 100) == ERR_ARG and b"n_problems" in L.bbbp_last_error()
    two = (_lib.SvrProblem * 2)(_problem(), _problem(epsilon=-1.0))              # the second of a batch is examined too
    assert L.bbbp_svr_smo(None, two, 2, 100) == ERR_ARG and b"problem 1" in L.bbbp_last_error()
    many = (_lib.SvrProblem * 40)(*([_problem()] * 39 + [_problem(C=0.0)]))      # and one behind the first launch's 32
    assert L.bbbp_svr_smo(None, many, 40, 100) == ERR_ARG and b"problem 39" in L.bbbp_last_error()
    assert ctypes.sizeof(_lib.SvrProblem) == 112                                 # 32 descriptors travel as kernel arguments: 3 584 bytes


def test_svr_argument_handling():
    from bbbp_amd.svm import SVC, SVR, fit_svr_folds, grid_search_cv_svr
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SVR(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SVR().fit(torch.zeros(8, 4), np.arange(8.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_svr_folds(np.zeros((10, 2)), np.arange(10.0), [np.arange(5)], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid_search_cv_svr(np.zeros((10, 2)), np.arange(10.0), {"C": [1.0]}, device="cpu")
    for kw, word in ((dict(kernel="poly"), "kernel"), (dict(kernel="sigmoid"), "kernel"), (dict(kernel="precomputed"), "kernel"), (dict(degree=2), "degree"),
                     (dict(coef0=1.0), "coef0"), (dict(epsilon=-0.1), "epsilon"), (dict(epsilon=float("nan")), "epsilon"), (dict(epsilon=float("inf")), "epsilon"),
                     (dict(epsilon="0.1"), "epsilon"), (dict(epsilon=True), "epsilon"), (dict(C=0), "C must"), (dict(C=-1.0), "C must"),
                     (dict(C=float("inf")), "C must"), (dict(gamma="big"), "gamma"), (dict(gamma=0.0), "gamma"), (dict(tol=0.0), "tol"),
                     (dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"), (dict(nu=0.5), "nu")):
        with pytest.raises(ValueError, match=word):
            SVR(**kw)
    m = SVR("linear", 10, 0.0, "auto", 1e-4, 7, shrinking=True)                  # scikit-learn's positional order; shrinking: accepted and ignored
    assert (m.kernel, m.C, m.epsilon, m.gamma, m.tol, m.max_iter, m.shrinking) == ("linear", 10, 0.0, "auto", 1e-4, 7, True)
    with pytest.raises(ValueError, match="sample_weight"):
        SVR().fit(np.zeros((4, 2)), np.zeros(4), sample_weight=np.ones(4))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="NaN or infinity"):
            SVR().fit(np.zeros((4, 2)), np.array([0.0, bad, 1.0, 2.0]))
    with pytest.raises(ValueError, match="1-D"):
        SVR().fit(np.zeros((4, 2)), np.zeros((4, 1)))
    with pytest.raises(ValueError, match="real"):
        SVR().fit(np.zeros((2, 2)), np.array(["a", "b"]))
    with pytest.raises(RuntimeError, match="not fitted"):
        SVR().predict(np.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="not fitted"):
        SVR().predict_device(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="classes"):                             # the classifier still refuses a continuous y
        SVC().fit(np.zeros((6, 2)), np.linspace(0.0, 1.0, 6))
    with pytest.raises(ValueError, match="grid keys"):
        grid_search_cv_svr(np.zeros((10, 2)), np.arange(10.0), {"C": [1.0], "degree": [2]})
    with pytest.raises(ValueError, match="kernel"):
        grid_search_cv_svr(np.zeros((10, 2)), np.arange(10.0), {"kernel": ["poly"]})
    with pytest.raises(ValueError, match="epsilon"):
        grid_search_cv_svr(np.zeros((10, 2)), np.arange(10.0), [{"C": [1.0]}, {"epsilon": [-1.0]}])
    with pytest.raises(ValueError, match="empty"):
        grid_search_cv_svr(np.zeros((10, 2)), np.arange(10.0), [])
    with pytest.raises(ValueError, match="rows"):
        grid_search_cv_svr(np.zeros((10, 2)), np.arange(9.0), {"C": [1.0]})
    with pytest.raises(ValueError, match="unsupported parameters"):
        fit_svr_folds(np.zeros((10, 2)), np.arange(10.0), [np.arange(5)], degree=3)
    with pytest.raises(ValueError, match="NaN or infinity"):
        fit_svr_folds(np.zeros((3, 2)), np.array([0.0, np.nan, 1.0]), [np.arange(2)])


def test_svr_clones_and_round_trips_its_parameters():
    from sklearn.base import clone
    from bbbp_amd.svm import SVR
    assert clone(SVR(C=3)).get_params() == dict(kernel="rbf", C=3, epsilon=0.1, gamma="scale", tol=1e-3, max_iter=-1, device="cuda", shrinking=False)
    m = SVR(kernel="linear", epsilon=0.0, gamma=0.5, max_iter=9)
    c = clone(m)
    assert c is not m and c.get_params() == m.get_params() and not hasattr(c, "support_")
    assert m.set_params(C=2.0, epsilon=0.3) is m and (m.C, m.epsilon) == (2.0, 0.3)
    with pytest.raises(ValueError, match="unknown parameters"):
        m.set_params(degree=2)
    with pytest.raises(ValueError, match="epsilon"):
        m.set_params(epsilon=-1.0)
    assert m.epsilon == 0.3                                                      # a refused value is not kept
