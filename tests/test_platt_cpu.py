"""CPU: the numpy restatement of libsvm's sigmoid_train (tests/platt_numpy.py) against scikit-learn's independent L-BFGS fit of the same
objective and against fixed points worked out by hand; the argument checks of the three svm_proba entry points and of svm.PlattSVC /
svm.platt_scale, none of which needs a GPU; the fold rule."""
import ctypes

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
import platt_numpy as P
from platt_numpy import make_dec, theta_bound

ERR_ARG = 1


@pytest.mark.parametrize("n,kind,ratio,seed", [(40, "mixed", 0.5, 0), (200, "mixed", 0.5, 1), (600, "mixed", 0.5, 2), (200, "mixed", 0.9, 3),
                                               (100, "separable", 0.5, 4), (300, "large", 0.5, 5)])
def test_restatement_against_sklearn_lbfgs(n, kind, ratio, seed):
    """sklearn.calibration._sigmoid_calibration minimises the same function of the same targets by L-BFGS.  Both results are approximate
    minimisers of a strictly convex function, so they differ by at most (|g(theta_1)| + |g(theta_2)|) / lambda_min(H).  The last assertion
    is no precision claim: it keeps the comparison from being vacuous (a restatement with other targets or another sign would see a large
    gradient at scikit-learn's result, and with it a large bound; such mistakes move theta by 0.1 or more)."""
    from sklearn.calibration import _sigmoid_calibration
    dec, y = make_dec(n, kind, seed, ratio)
    A, B, n_iter, status, g, H = P.sigmoid_train(dec, y)
    a, b = _sigmoid_calibration(dec, (y > 0).astype(np.float64))
    limit = theta_bound(dec, y, (A, B), (a, b), H)
    diff = float(np.hypot(A - a, B - b))
    print(f"n {n} {kind} {ratio}: A {A:.6g} B {B:.6g}, {n_iter} iterations, |theta - sklearn| {diff:.3g}, bound {limit:.3g}")
    assert status == P.CONVERGED and np.abs(g).max() < P.EPS
    assert diff <= limit
    assert limit <= 1e-2 * max(1.0, float(np.hypot(A, B)))


def test_fixed_points_by_hand():
    # n = 1: the start is the minimum.  y = +1: t = 2/3, B0 = log(1/2), p = 1 / (1 + 1/2) = t; y = -1: t = 1/3, B0 = log 2, p = 1/3
    for y, B0 in ((1.0, np.log(0.5)), (-1.0, np.log(2.0))):
        A, B, n_iter, status, g, _ = P.sigmoid_train(np.array([0.3]), np.array([y]))
        assert (A, n_iter, status) == (0.0, 0, P.CONVERGED) and B == B0 and np.abs(g).max() < 1e-15
    # one class only, n rows of +1: t = (n + 1) / (n + 2) everywhere, B0 = log(1 / (n + 1)) gives p = (n + 1) / (n + 2) = t: the start again
    for n in (1, 7, 300):
        dec, y = make_dec(n, "mixed", 6, ratio=1.0)
        A, B, n_iter, status, g, _ = P.sigmoid_train(dec, y)
        assert (y > 0).all() and (A, n_iter, status) == (0.0, 0, P.CONVERGED) and B == np.log(1.0 / (n + 1.0))
        A, B, n_iter, status, _, _ = P.sigmoid_train(dec, -y)
        assert (A, n_iter, status) == (0.0, 0, P.CONVERGED) and B == np.log(n + 1.0)
    # all dec equal to c: F depends on f = A c + B alone and its minimum is p = mean(t), f* = log((1 - mean t) / mean t).  c = 0: dec
    # carries no gradient, only B moves.  c != 0: the Hessian is singular up to sigma and the regularised Newton step is the
    # minimum-norm one, along (c, 1): A moves by c times what B moves by -- up to the cancellation in h22 g1 - h21 g2, whose two products
    # of size |c| s |g2| (s = sum p q <= n / 4) leave sigma |c| |g2|: a relative error of a few 2^-52 s / sigma
    y = np.r_[np.ones(20), -np.ones(10)]
    t, _, _ = P.targets(y)
    want = np.log((1.0 - t.mean()) / t.mean())
    B0 = np.log(11.0 / 21.0)
    A, B, _, status, _, _ = P.sigmoid_train(np.zeros(30), y)
    assert status == P.CONVERGED and A == 0.0 and abs(B - want) <= 1e-5 / (30 * t.mean() * (1 - t.mean())) * 2      # |g_B| < 1e-5 over F''
    for c in (2.0, -0.5):
        A, B, _, status, _, _ = P.sigmoid_train(np.full(30, c), y)
        assert status == P.CONVERGED and abs(A * c + B - want) <= 1e-5 / (30 * t.mean() * (1 - t.mean())) * 2
        assert B != B0 and abs(A - c * (B - B0)) <= 8 * P.U52 * (30 / 4) / P.SIGMA * abs(c * (B - B0))


def _oof(**kw):
    base = dict(K=4096, ldk=130, n_rows=130, rows=4096, y=4096, alpha=4096, rho=4096, n=104, held=4096, n_held=26, out=4096)
    base.update(kw)
    return _lib.SvmOofDesc(**base)


def _platt(**kw):
    base = dict(dec=4096, y=4096, n=130, ab=4096, info=4096)
    base.update(kw)
    return _lib.SvmPlattProblem(**base)


def test_proba_entry_points_validate_before_touching_the_gpu():
    """Pointers are the fake address 4096: validation comes first and none is dereferenced."""
    L = _lib.lib()
    oof = lambda **kw: L.bbbp_svm_oof_decision(None, ctypes.byref(_oof(**kw)), 1)  # noqa: E731
    for bad, word in ((dict(K=None), b"null"), (dict(y=None), b"null"), (dict(alpha=None), b"null"), (dict(rho=None), b"null"), (dict(out=None), b"null"),
                      (dict(held=None), b"null"), (dict(n=0), b"positive"), (dict(n=-3), b"positive"), (dict(n=131), b"n_rows"), (dict(n_rows=0), b"positive"),
                      (dict(n_held=-1), b"n_held"), (dict(n_held=131), b"n_held"), (dict(ldk=129), b"leading"), (dict(ldk=103), b"leading")):
        assert oof(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert L.bbbp_svm_oof_decision(None, None, 1) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_svm_oof_decision(None, ctypes.byref(_oof()), 0) == ERR_ARG and b"n_folds" in L.bbbp_last_error()
    assert L.bbbp_svm_oof_decision(None, ctypes.byref(_oof()), -1) == ERR_ARG and b"n_folds" in L.bbbp_last_error()
    two = (_lib.SvmOofDesc * 2)(_oof(), _oof(alpha=None))                         # the second of a batch is examined too
    assert L.bbbp_svm_oof_decision(None, two, 2) == ERR_ARG and b"fold 1" in L.bbbp_last_error()

    fit = lambda **kw: L.bbbp_svm_platt_fit(None, ctypes.byref(_platt(**kw)), 1)  # noqa: E731
    for bad, word in ((dict(dec=None), b"null"), (dict(y=None), b"null"), (dict(ab=None), b"null"), (dict(info=None), b"null"), (dict(n=0), b"positive"),
                      (dict(n=-1), b"positive")):
        assert fit(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert L.bbbp_svm_platt_fit(None, None, 1) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_svm_platt_fit(None, ctypes.byref(_platt()), 0) == ERR_ARG and b"n_problems" in L.bbbp_last_error()
    assert L.bbbp_svm_platt_fit(None, ctypes.byref(_platt()), -2) == ERR_ARG and b"n_problems" in L.bbbp_last_error()
    two = (_lib.SvmPlattProblem * 2)(_platt(), _platt(n=0))
    assert L.bbbp_svm_platt_fit(None, two, 2) == ERR_ARG and b"problem 1" in L.bbbp_last_error()

    proba = lambda dec=4096, m=5, A=-1.0, B=0.0, out=4096: L.bbbp_svm_platt_proba(None, dec, m, A, B, out)  # noqa: E731
    assert proba(dec=None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert proba(out=None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert proba(m=-1) == ERR_ARG and b"negative" in L.bbbp_last_error()
    for bad in (dict(A=float("nan")), dict(B=float("inf")), dict(A=float("-inf"))):
        assert proba(**bad) == ERR_ARG and b"finite" in L.bbbp_last_error(), bad
    assert proba(m=0) == 0 and proba(m=0, dec=None, out=None) == 0                # nothing to do, nothing launched


def test_plattsvc_argument_handling():
    from sklearn.base import clone
    from bbbp_amd.svm import SVC, PlattSVC, platt_scale
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PlattSVC(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PlattSVC().fit(torch.zeros(8, 4), [0, 1] * 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        platt_scale(np.zeros(4), np.ones(4), device="cpu")
    for kw in (dict(cv=1), dict(cv=0), dict(cv=-5), dict(cv=2.5), dict(cv=True), dict(cv=None), dict(random_state=1.5), dict(random_state="0"),
               dict(random_state=None), dict(random_state=True), dict(random_state=-1), dict(class_weight="balanced"), dict(class_weight={0: 2.0}),
               dict(probability=True), dict(degree=2), dict(decision_function_shape="ovo"), dict(kernel="poly"), dict(C=0), dict(C="1"), dict(gamma="big"),
               dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            PlattSVC(**kw)
    with pytest.raises(ValueError, match="class_weight"):
        PlattSVC(class_weight="balanced")
    with pytest.raises(ValueError, match="unsupported"):
        PlattSVC(coef0=1.0)
    X, y = np.zeros((6, 2)), np.array([0, 1] * 3)
    with pytest.raises(ValueError, match="cv=7"):
        PlattSVC(cv=7).fit(X, y)
    with pytest.raises(ValueError, match="classes"):
        PlattSVC().fit(X, np.zeros(6))
    for folds in ([[0, 1, 2], [3, 4]], [[0, 1, 2], [2, 3, 4, 5]], [[0, 1, 2], [3, 4, 6]], [[0, 1, 2, 3, 4, 5, 6]], [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]],
                  [], [[[0, 1, 2]], [[3, 4, 5]]], [[-1, 0, 1, 2], [3, 4, 5]]):
        with pytest.raises(ValueError, match="folds"):
            PlattSVC().fit(X, y, folds=folds)
    with pytest.raises(RuntimeError, match="not fitted"):
        PlattSVC().predict_proba(np.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="not fitted"):
        PlattSVC().predict_log_proba(np.zeros((2, 4)))
    # parameters round-trip as given
    clf = PlattSVC(C=3, cv=4)
    twin = clone(clf)
    assert type(twin) is PlattSVC and twin.get_params() == clf.get_params() == dict(C=3, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, cv=4,
                                                                                   random_state=0, device="cuda")
    assert clf.set_params(C=10.0, random_state=7) is clf and (clf.C, clf.random_state) == (10.0, 7)
    with pytest.raises(ValueError, match="unknown"):
        clf.set_params(degree=3)
    with pytest.raises(ValueError, match="cv"):
        clf.set_params(cv=1)
    assert clf.cv == 4 and isinstance(clf, SVC)
    # SVC itself is as it was, and its message names the new class
    with pytest.raises(ValueError, match="probability") as err:
        SVC(probability=True)
    assert "PlattSVC" in str(err.value)


def test_fold_rule():
    """libsvm's fold boundaries i n // cv over a permutation that depends on random_state and n alone."""
    from bbbp_amd.svm import platt_folds
    folds = platt_folds(23, 5, 0)
    assert [len(f) for f in folds] == [4, 5, 4, 5, 5]
    assert np.array_equal(np.sort(np.concatenate(folds)), np.arange(23))
    assert np.array_equal(np.concatenate(folds), np.random.RandomState(0).permutation(23))
    again = platt_folds(23, 5, 0)
    assert all(np.array_equal(a, b) for a, b in zip(folds, again))
    assert not np.array_equal(np.concatenate(platt_folds(23, 5, 1)), np.concatenate(folds))
    for n, cv in ((5, 5), (5, 2), (130, 7), (200, 3)):
        parts = platt_folds(n, cv, 3)
        assert [len(p) for p in parts] == [(i + 1) * n // cv - i * n // cv for i in range(cv)]
        assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(n))
