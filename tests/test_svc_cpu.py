"""CPU: the SVC oracle (tests/svc_oracle.py) is pinned to scikit-learn's libsvm without shrinking; every svm entry point's argument checks
and SVC's Python argument handling work without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
import svc_oracle as O

ERR_ARG = 1
# (n, d, sep, kernel, C): the RBF problems of the GPU parity test, and the linear problem at the C values whose iteration counts stay small
CASES = [(200, 10, 0.7, "rbf", 0.1), (200, 10, 0.7, "rbf", 1.0), (200, 10, 0.7, "rbf", 10.0), (333, 100, 0.5, "rbf", 1.0), (333, 100, 0.5, "rbf", 10.0),
         (200, 10, 0.7, "linear", 0.1), (200, 10, 0.7, "linear", 1.0)]


@pytest.mark.parametrize("n,d,sep,kind,C", CASES)
def test_oracle_against_sklearn(n, d, sep, kind, C):
    """The same support set; dual_coef_, intercept_ and 200 held-out decision values within 4 x scikit-learn's own scatter (at least
    10 tol), measured by svc_oracle.sklearn_reference."""
    sk, want, tolerance = O.sklearn_reference(n, d, sep, kind, C)
    X, y = O.make_data(n, d, sep, 1)
    Q, _ = O.make_data(200, d, sep, 2)
    g = O.gamma_scale(X)
    assert abs(g - sk._gamma) <= 1e-15 * g
    m = O.fit(X, y, C, kind, g, tol=1e-3)
    got = O.decision(Q, X, m, kind, g)
    print(f"n {n} d {d} {kind} C {C}: tolerance {tolerance:.3g}, iterations {m['n_iter_']} (scikit-learn {int(np.ravel(sk.n_iter_)[0])}), "
          f"decision difference {np.abs(got - want).max():.3g}")
    assert m["converged"] and np.array_equal(m["classes_"], sk.classes_)
    assert np.array_equal(m["support_"], sk.support_)
    assert np.abs(m["dual_coef_"] - sk.dual_coef_).max() <= tolerance
    assert abs(m["intercept_"][0] - sk.intercept_[0]) <= tolerance
    assert np.abs(got - want).max() <= tolerance
    # the solution the oracle stops at is optimal to tol by its own recomputation
    ys = np.where(y == m["classes_"][0], 1.0, -1.0)
    gap, G = O.violation(O.kernel(X, X, kind, g), ys, m["alpha"], C)
    assert gap <= 1e-3 * (1 + 1e-6) + 1e-9
    assert abs(O.rho_rule(ys, G, m["alpha"], C) - m["intercept_"][0]) <= 1e-9


def test_oracle_ties_keep_the_later_index():
    """Duplicated rows tie exactly in both selections: libsvm's scans keep the later index, so the later copy moves first."""
    X, y = O.make_data(40, 4, 1.0, 3)
    X2, y2 = np.concatenate([X, X]), np.concatenate([y, y])
    K = O.kernel(X2, X2, "rbf", 0.25)
    alpha, _, n_iter, ok = O.smo(K, np.where(y2 == -1.0, 1.0, -1.0), 1.0, max_iter=1)
    assert n_iter == 1 and not ok
    moved = np.flatnonzero(alpha > 0)
    assert len(moved) == 2 and (moved >= 40).all()
    assert O.smo(K, y2, 1.0, max_iter=5)[2] == 5


def _kdesc(**kw):
    base = dict(n=130, d=100, kernel=1, gamma=0.01, X=4096, x_dtype=1, ldx=100, mu=4096, norms=4096, K=4096, ldk=130)
    base.update(kw)
    return _lib.SvmKernelDesc(**base)


def _ddesc(**kw):
    base = dict(m=130, n_sv=300, d=100, kernel=1, gamma=0.01, Q=4096, q_dtype=0, ldq=100, SV=4096, sv_dtype=1, ldsv=100, mu=4096, q_norm=4096,
                sv_norm=4096, coef=4096, intercept=0.5, out=4096, slices=0)
    base.update(kw)
    return _lib.SvmDecisionDesc(**base)


def _problem(**kw):
    base = dict(K=4096, ldk=100, rows=None, y=4096, alpha=4096, grad=4096, diag=4096, rho=4096, n_iter=4096, done=4096, n=100, C=1.0, tol=1e-3)
    base.update(kw)
    return _lib.SvmProblem(**base)


def test_svm_entry_points_validate_before_touching_the_gpu():
    """Pointers are the fake address 4096: validation comes first and none is dereferenced."""
    L = _lib.lib()
    mat = lambda **kw: L.bbbp_svm_kernel_matrix(None, ctypes.byref(_kdesc(**kw)))  # noqa: E731
    for bad, word in ((dict(n=0), b"positive"), (dict(d=0), b"positive"), (dict(kernel=2), b"kernel"), (dict(kernel=-1), b"kernel"), (dict(x_dtype=2), b"dtype"),
                      (dict(X=None), b"null"), (dict(K=None), b"null"), (dict(ldx=99), b"leading"), (dict(ldk=129), b"leading"), (dict(gamma=0.0), b"gamma"),
                      (dict(gamma=-1.0), b"gamma"), (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"), (dict(norms=None), b"norms")):
        assert mat(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert L.bbbp_svm_kernel_matrix(None, None) == ERR_ARG

    one = lambda iters=100, **kw: L.bbbp_svm_smo(None, ctypes.byref(_problem(**kw)), 1, iters)  # noqa: E731
    for bad, word in ((dict(n=0), b"positive"), (dict(K=None), b"null"), (dict(y=None), b"null"), (dict(alpha=None), b"null"), (dict(grad=None), b"null"),
                      (dict(diag=None), b"null"), (dict(rho=None), b"null"), (dict(n_iter=None), b"null"), (dict(done=None), b"null"), (dict(ldk=99), b"leading"),
                      (dict(rows=4096, ldk=0), b"leading"), (dict(C=0.0), b"C "), (dict(C=float("inf")), b"C "), (dict(tol=0.0), b"tol"),
                      (dict(tol=float("nan")), b"tol")):
        assert one(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert one(iters=0) == ERR_ARG and b"iters" in L.bbbp_last_error()
    assert one(iters=(1 << 20) + 1) == ERR_ARG and b"iters" in L.bbbp_last_error()
    assert L.bbbp_svm_smo(None, None, 1, 100) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_svm_smo(None, ctypes.byref(_problem()), 0, 100) == ERR_ARG and b"n_problems" in L.bbbp_last_error()
    two = (_lib.SvmProblem * 2)(_problem(), _problem(C=-1.0))                    # the second of a batch is examined too
    assert L.bbbp_svm_smo(None, two, 2, 100) == ERR_ARG and b"problem 1" in L.bbbp_last_error()

    ws = lambda **kw: L.bbbp_svm_decision_workspace_bytes(ctypes.byref(_ddesc(**kw)))  # noqa: E731
    assert ws() == 5 * 130 * 8                                  # one partial per (tile of 64 support vectors, query)
    assert ws(slices=7) == ws(slices=1) == ws()                 # the slice count moves work, not the unit of summation
    assert ws(n_sv=64, m=1) == 8 and ws(n_sv=65, m=1) == 16
    run = lambda ws_bytes=0, **kw: L.bbbp_svm_decision(None, ctypes.byref(_ddesc(**kw)), None, ws_bytes)  # noqa: E731
    for bad, word in ((dict(m=0), b"positive"), (dict(n_sv=0), b"positive"), (dict(d=0), b"positive"), (dict(kernel=3), b"kernel"), (dict(q_dtype=2), b"dtype"),
                      (dict(sv_dtype=-1), b"dtype"), (dict(slices=65), b"slices"), (dict(slices=-1), b"slices"), (dict(gamma=0.0), b"gamma")):
        assert ws(**bad) == 0 and word in L.bbbp_last_error(), bad
        assert run(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    for bad, word in ((dict(Q=None), b"null"), (dict(SV=None), b"null"), (dict(coef=None), b"null"), (dict(out=None), b"null"), (dict(q_norm=None), b"norms"),
                      (dict(sv_norm=None), b"norms"), (dict(ldq=99), b"leading"), (dict(ldsv=99), b"leading")):
        assert run(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert L.bbbp_svm_decision(None, None, None, 0) == ERR_ARG
    assert run() == 3 and b"workspace" in L.bbbp_last_error()   # BBBP_ERR_WORKSPACE, still before any HIP call
    assert run(kernel=0, q_norm=None, sv_norm=None, mu=None) == 3      # the linear kernel needs no norms


def test_svc_argument_handling():
    from bbbp_amd.svm import SVC, grid_search_cv, kernel_matrix
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SVC(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SVC().fit(torch.zeros(8, 4), [0, 1] * 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"C": [1.0]}, device="cpu")
    for kw in (dict(probability=True), dict(class_weight="balanced"), dict(class_weight={0: 2.0}), dict(kernel="poly"), dict(kernel="sigmoid"),
               dict(kernel="precomputed"), dict(degree=2), dict(coef0=1.0), dict(decision_function_shape="ovo"), dict(C=0), dict(C=-1.0),
               dict(C="1"), dict(C=float("inf")), dict(C=True), dict(gamma="big"), dict(gamma=0.0), dict(gamma=-1.0), dict(tol=0.0), dict(tol=None),
               dict(max_iter=0), dict(max_iter=-2), dict(max_iter=2.5)):
        with pytest.raises(ValueError):
            SVC(**kw)
    with pytest.raises(ValueError, match="probability"):
        SVC(probability=True)
    clf = SVC(C=10, kernel="linear", gamma="auto", tol=1e-4, max_iter=7, shrinking=True)          # shrinking: accepted and ignored
    assert (clf.C, clf.kernel, clf.gamma, clf.tol, clf.max_iter) == (10.0, "linear", "auto", 1e-4, 7)
    with pytest.raises(ValueError, match="classes"):
        SVC().fit(np.zeros((6, 2)), [0, 1, 2, 0, 1, 2])
    with pytest.raises(ValueError, match="classes"):
        SVC().fit(np.zeros((6, 2)), np.zeros(6))
    with pytest.raises(ValueError, match="1-D"):
        SVC().fit(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(RuntimeError, match="not fitted"):
        SVC().decision_function(np.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="not fitted"):
        SVC().predict(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="kernel"):
        kernel_matrix(torch.zeros(4, 2), "poly")
    with pytest.raises(ValueError, match="grid keys"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"C": [1.0], "degree": [2]})
    with pytest.raises(ValueError, match="kernel"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, {"C": [1.0], "kernel": ["poly"]})
    with pytest.raises(ValueError, match="C must"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 5, [{"C": [1.0]}, {"C": [0.0], "kernel": ["linear"]}])
    with pytest.raises(ValueError, match="classes"):
        grid_search_cv(np.zeros((10, 2)), np.arange(10), {"C": [1.0]})
    with pytest.raises(ValueError, match="rows"):
        grid_search_cv(np.zeros((10, 2)), [0, 1] * 4, {"C": [1.0]})
