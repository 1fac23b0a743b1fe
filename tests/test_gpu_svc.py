"""GPU: svm's kernel matrix, SMO solver and decision function against the numpy oracle of tests/svc_oracle.py, and svm.SVC /
grid_search_cv against scikit-learn within the scatter scikit-learn's own runs show (svc_oracle.sklearn_reference).

Bounds.  u = 2^-53.  A float64 sum of t products in any order is within t u sum |a b| of the exact value (first order; t + 1 below for the
higher orders); the oracle's own sum carries the same bound, so two such sums differ by at most 2 (t + 1) u sum |a b|.  The RBF value
exp(-gamma s) inherits gamma x (the error of s) relatively; the error of s is B of tests/knn_oracle.py for the two rows, and exp, the
product gamma s and the oracle's own evaluation stay within 8 u."""
import functools
import warnings

import numpy as np
import pytest
import torch

from bbbp_amd import svm
from bbbp_amd.svm import SVC, grid_search_cv, kernel_matrix
from knn_oracle import bound, make_points
import svc_oracle as O

pytestmark = pytest.mark.gpu

U53 = O.U53
NS = (1, 63, 65, 130, 333)
DS = (1, 3, 17, 100, 167)
POOL_D = 200                     # operands are [:n, :d] views of a pool this wide: the row stride differs from d


@functools.lru_cache(maxsize=None)
def _pool():
    X = make_points(333, POOL_D, 41)                 # exact in float32: both dtypes see the same numbers
    return X, torch.from_numpy(X).cuda(), torch.from_numpy(X.astype(np.float32)).cuda()


def _check_matrix(K, X, kind, gamma, what):
    n = X.shape[0]
    assert K.shape == (n, n) and K.dtype == torch.float64
    assert torch.equal(K, K.t()), f"{what}: not bitwise symmetric"
    got, want = K.cpu().numpy(), O.kernel(X, X, kind, gamma)
    if kind == "linear":
        limit = 2.0 * (X.shape[1] + 1) * U53 * (np.abs(X) @ np.abs(X).T)
    else:
        assert (np.diag(got) == 1.0).all(), f"{what}: the diagonal is not exactly 1"
        limit = (gamma * bound(X, X) + 8.0 * U53) * want
    err = np.abs(got - want)
    assert (err <= limit).all(), f"{what}: worst error / bound = {(err / (limit + 1e-300)).max():.3g}"


@pytest.mark.parametrize("d", DS)
def test_kernel_matrix_against_oracle(dev, d):
    X64, d64, d32 = _pool()
    for n in NS:
        X = X64[:n, :d]
        gamma = 1.0 if n == 1 else O.gamma_scale(X)
        for name, pool in (("f64", d64), ("f32", d32)):
            Xd = pool[:n, :d]
            assert n == 1 or Xd.stride(0) == POOL_D
            for kind in ("linear", "rbf"):
                K, _, _ = kernel_matrix(Xd, kind, gamma)
                _check_matrix(K, X, kind, gamma, f"n {n} d {d} {name} {kind}")


def test_kernel_matrix_large_mean(dev):
    """X = 1e6 + 1e-3 randn: an uncentred expansion of the squared distances is wrong by ~1 against values of ~1e-4."""
    X = 1e6 + 1e-3 * np.random.RandomState(5).randn(300, 50)
    gamma = O.gamma_scale(X)
    Xd = torch.from_numpy(X).cuda()
    for kind in ("rbf", "linear"):
        _check_matrix(kernel_matrix(Xd, kind, gamma)[0], X, kind, gamma, f"large mean {kind}")
    assert 0.0 < kernel_matrix(Xd, "rbf", gamma)[0].min().item() < 0.9          # the values are not all 1: the distances are resolved


def test_kernel_matrix_refuses_a_matrix_larger_than_free_memory(dev):
    """2 000 000 rows as a zero-stride view of one: the 32 TB matrix is refused before anything is allocated or launched."""
    X = torch.zeros(1, 4, dtype=torch.float64, device="cuda").expand(2_000_000, 4)
    before = torch.cuda.memory_allocated()
    for kind in ("linear", "rbf"):
        with pytest.raises(ValueError, match="does not fit in free device memory"):
            kernel_matrix(X, kind, 1.0)
    assert torch.cuda.memory_allocated() == before


def test_launch_length_shrinks_with_n(dev, monkeypatch):
    """Beyond svm.ITERS_REFERENCE_N rows the iterations per launch shrink in proportion (here with the reference lowered to 50 rows, so
    that 200 rows get a quarter of the count); the result is that of the default launches, bit for bit."""
    X, y = O.make_data(200, 10, 0.7, 1)
    want = SVC().fit(X, y)
    calls = []
    real = svm._lib.lib().bbbp_svm_smo
    monkeypatch.setattr(svm, "ITERS_REFERENCE_N", 50)
    monkeypatch.setattr(svm, "ITERS_PER_LAUNCH", 100)
    L = svm._lib.lib()
    monkeypatch.setattr(L, "bbbp_svm_smo", lambda st, arr, n, iters: calls.append(iters) or real(st, arr, n, iters))
    got = SVC().fit(X, y)
    assert calls and set(calls) == {25} and len(calls) == -(-want.n_iter_ // 25) + (want.n_iter_ % 25 == 0)
    assert np.array_equal(got.alpha_, want.alpha_) and got.n_iter_ == want.n_iter_ and got.intercept_[0] == want.intercept_[0]


def test_kernel_matrix_refuses_non_finite_input(dev):
    X = _pool()[0][:65, :17].copy()
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[64, 16] = bad
        for kind in ("linear", "rbf"):
            with pytest.raises(ValueError, match="NaN or infinity"):
                SVC(kernel=kind).fit(Xb, np.arange(65) % 2)
    clf = SVC().fit(X, np.arange(65) % 2)
    Q = X[:5].copy()
    Q[2, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        clf.decision_function(Q)
    with pytest.raises(ValueError, match="features"):
        clf.decision_function(X[:5, :16])


# (n, d, sep) per kernel; the linear problem only with C <= 1: 175 to 3 403 iterations there, 26 000 or more at C = 10
SOLVER_CASES = [(kind, n, d, sep, C, tol) for kind, n, d, sep, Cs in (("rbf", 200, 10, 0.7, (0.1, 1.0, 10.0)), ("rbf", 333, 100, 0.5, (0.1, 1.0, 10.0)),
                                                                        ("linear", 200, 10, 0.7, (0.1, 1.0)))
                for C in Cs for tol in (1e-3, 1e-8)]


@pytest.mark.parametrize("kind,n,d,sep,C,tol", SOLVER_CASES)
def test_solver_optimality(dev, kind, n, d, sep, C, tol):
    """Optimality recomputed in numpy from the GPU's own alpha, with the oracle's direct-difference kernel: independent of the path."""
    X, y = O.make_data(n, d, sep, 1)
    clf = SVC(C=C, kernel=kind, tol=tol).fit(X, y)
    alpha, ys = clf.alpha_, np.where(y == clf.classes_[0], 1.0, -1.0)
    assert alpha.shape == (n,) and (alpha >= 0.0).all() and (alpha <= C).all()
    assert abs((ys * alpha).sum()) <= n * C * U53 * 4
    gap, G = O.violation(O.kernel(X, X, kind, clf._gamma), ys, alpha, C)
    print(f"{kind} n {n} C {C} tol {tol}: {clf.n_iter_} iterations, m - M = {gap:.3g}")
    assert gap <= tol * (1 + 1e-6) + 1e-9
    assert abs(clf.intercept_[0] - O.rho_rule(ys, G, alpha, C)) <= 1e-9
    assert np.array_equal(clf.support_, O.support_order(alpha, ys)) and clf.support_.dtype == np.int32
    assert np.array_equal(clf.dual_coef_, (-ys * alpha)[clf.support_][None, :]) and clf.intercept_.shape == (1,)
    assert np.array_equal(clf.n_support_, [(ys[clf.support_] > 0).sum(), (ys[clf.support_] < 0).sum()])
    assert np.array_equal(clf.support_vectors_, X[clf.support_]) and np.array_equal(clf.classes_, [-1.0, 1.0])
    assert abs(clf._gamma - O.gamma_scale(X)) <= 1e-14 * clf._gamma and clf.n_iter_ > 0 and clf.fit_status_ == 0


@functools.lru_cache(maxsize=None)
def _fitted(kind):
    n, d, sep = (333, 100, 0.5) if kind == "rbf" else (200, 10, 0.7)
    X, y = O.make_data(n, d, sep, 1)
    return X, SVC(C=1.0, kernel=kind).fit(X, y)


@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_decision_function(dev, kind):
    """Against a numpy float64 sum over the GPU's own dual_coef_ and support_vectors_.  Bound: every kernel value's own bound (module
    docstring) times |coef|, plus the n_SV-term sum bound of both sides, plus the rounding of the intercept's addition."""
    X, clf = _fitted(kind)
    sv, coef, b, g = clf.support_vectors_, clf.dual_coef_[0], clf.intercept_[0], clf._gamma
    mu = X.mean(axis=0)
    Qall, _ = O.make_data(130, X.shape[1], 0.5, 2)
    for m in (1, 63, 65, 130):
        Q = Qall[:m]
        Kq = O.kernel(Q, sv, kind, g)
        want = Kq @ coef + b
        if kind == "linear":
            kerr = 2.0 * (Q.shape[1] + 1) * U53 * (np.abs(Q) @ np.abs(sv).T)
        else:
            B = 4.0 * (Q.shape[1] + 4) * U53 * (((Q - mu) ** 2).sum(axis=1)[:, None] + ((sv - mu) ** 2).sum(axis=1)[None, :])      # knn_oracle.bound about the training mean
            kerr = (g * B + 8.0 * U53) * Kq
        limit = kerr @ np.abs(coef) + 2.0 * (len(coef) + 2) * U53 * (np.abs(Kq) @ np.abs(coef)) + 2.0 * U53 * np.abs(want)
        Qd = torch.from_numpy(Q).cuda()
        first = clf.decision_function(Qd)
        assert first.is_cuda and first.dtype == torch.float64 and first.shape == (m,)
        for s in (0, 1, 2, 7, 0):
            assert torch.equal(clf.decision_function(Qd, slices=s), first), f"{kind} m {m}: slices {s} differs"
        err = np.abs(first.cpu().numpy() - want)
        assert (err <= limit).all(), f"{kind} m {m}: worst error / bound = {(err / limit).max():.3g}"
        got = clf.decision_function(Q)
        assert isinstance(got, np.ndarray) and np.array_equal(got, first.cpu().numpy())
        assert np.array_equal(clf.predict(Q), clf.classes_[(got > 0).astype(int)])
        assert np.array_equal(clf.decision_function(Q.astype(np.float32).astype(np.float64)), clf.decision_function(Q.astype(np.float32)))


@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_batch_independence(dev, kind):
    """The C values of one batch equal the same problems solved alone, bit for bit -- also when the launches are cut short, and when a
    problem addresses its rows through an index list into a larger matrix."""
    X, y = O.make_data(200, 10, 0.7, 1)
    ys = np.where(y == -1.0, 1.0, -1.0)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(ys).cuda()
    K = kernel_matrix(Xd, kind, O.gamma_scale(X))[0]
    Cs = (0.1, 1.0, 10.0) if kind == "rbf" else (0.1, 1.0)

    def run(problems, **kw):
        out = svm._solve(problems, **kw)
        return [(p.alpha.clone(), p.grad.clone(), p.rho.clone(), it, ok) for p, (it, ok) in zip(problems, out)]

    def same(a, b):
        return all(torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v for u, v in zip(a, b))

    together = run([svm._Problem(K, yd, C, 1e-3) for C in Cs])
    assert all(ok for *_, ok in together)
    for C, want in zip(Cs, together):
        assert same(run([svm._Problem(K, yd, C, 1e-3)])[0], want), f"{kind} C {C}: alone differs from the batch"
    assert all(same(a, b) for a, b in zip(run([svm._Problem(K, yd, C, 1e-3) for C in Cs]), together)), "a repeat run differs"
    assert all(same(a, b) for a, b in zip(run([svm._Problem(K, yd, C, 1e-3) for C in reversed(Cs)]), reversed(together)))
    assert all(same(a, b) for a, b in zip(run([svm._Problem(K, yd, C, 1e-3) for C in Cs], iters_per_launch=37), together)), "short launches differ"
    # a fold as a row list into the shared matrix = the fold's own matrix
    rows = np.flatnonzero(np.arange(200) % 5 != 2)
    rd = torch.from_numpy(rows).cuda()
    sub = K[rd][:, rd].contiguous()
    own = run([svm._Problem(sub, yd[rd].contiguous(), C, 1e-3) for C in Cs])
    listed = run([svm._Problem(K, yd[rd].contiguous(), C, 1e-3, rd.to(torch.int32)) for C in Cs])
    assert all(same(a, b) for a, b in zip(own, listed)), "a row list differs from the sub-matrix"
    assert torch.equal(kernel_matrix(Xd[rd], "linear")[0], kernel_matrix(Xd, "linear")[0][rd][:, rd])


GRID = [{"C": [0.1, 1, 10], "kernel": ["rbf"]}, {"C": [0.1, 1], "kernel": ["linear"]}]      # the reference's grid without (linear, C = 10)


@functools.lru_cache(maxsize=None)
def _grid_run():
    X, y = O.make_data(200, 10, 0.7, 1)
    return X, y, grid_search_cv(X, y, GRID, cv=5)


def test_grid_search_cv_equals_single_fits(dev):
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    X, y, (best, scores, fitted) = _grid_run()
    points = [dict(C=C, kernel=k) for g in GRID for C in g["C"] for k in g["kernel"]]
    want = np.zeros((len(points), 5))
    for fi, (tr, te) in enumerate(StratifiedKFold(n_splits=5).split(X, y)):
        for pi, pt in enumerate(points):
            want[pi, fi] = f1_score(y[te], SVC(**pt).fit(X[tr], y[tr]).predict(X[te]))
    assert scores == [float(v) for v in want.mean(axis=1)]
    assert best == points[int(np.argmax(scores))]
    single = SVC(**best).fit(X, y)
    assert np.array_equal(fitted.alpha_, single.alpha_) and fitted.n_iter_ == single.n_iter_ and (fitted.C, fitted.kernel) == (best["C"], best["kernel"])


def test_grid_search_cv_against_sklearn(dev):
    """scikit-learn's scores within one flipped prediction per fold: a flip moves F1 = 2 TP / D, D = 2 TP + FP + FN, by at most 2 / (D - 1),
    and D is at least the number P of positives in the fold's test rows."""
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from sklearn.svm import SVC as SkSVC
    X, y, (best, scores, _) = _grid_run()
    sk = GridSearchCV(SkSVC(), GRID, cv=5, scoring="f1").fit(X, y)
    want = sk.cv_results_["mean_test_score"]
    slack = np.mean([2.0 / ((y[te] == 1.0).sum() - 1) for _, te in StratifiedKFold(n_splits=5).split(X, y)])
    print(f"scores {scores}\nscikit-learn {list(want)}\nslack {slack:.3g}")
    assert len(scores) == len(want) == 5 and np.abs(np.asarray(scores) - want).max() <= slack
    assert best == sk.best_params_ == sk.cv_results_["params"][int(np.argmax(scores))]


@pytest.mark.parametrize("n,d,sep,C", [(333, 100, 0.5, 1.0), (333, 100, 0.5, 10.0), (200, 10, 0.7, 1.0)])
def test_svc_against_sklearn(dev, n, d, sep, C):
    sk, want, tolerance = O.sklearn_reference(n, d, sep, "rbf", C)
    X, y = O.make_data(n, d, sep, 1)
    Q, _ = O.make_data(200, d, sep, 2)
    clf = SVC(C=C).fit(X, y)
    got = clf.decision_function(Q)
    clear = np.abs(want) > tolerance
    print(f"n {n} d {d} C {C}: tolerance {tolerance:.3g}, largest difference {np.abs(got - want).max():.3g}, {np.count_nonzero(~clear)} queries exempt, "
          f"{clf.n_iter_} iterations (scikit-learn {int(np.ravel(sk.n_iter_)[0])})")
    assert np.abs(got - want).max() <= tolerance
    assert np.count_nonzero(~clear) <= 0.02 * len(want)
    assert np.array_equal(clf.predict(Q)[clear], sk.predict(Q)[clear])
    assert np.array_equal(clf.classes_, sk.classes_) and abs(clf._gamma - sk._gamma) <= 1e-14 * sk._gamma


def test_max_iter_stops_with_a_warning(dev):
    from sklearn.exceptions import ConvergenceWarning
    X, y = O.make_data(333, 100, 0.5, 1)
    with pytest.warns(ConvergenceWarning):
        clf = SVC(max_iter=5).fit(X, y)
    assert clf.n_iter_ == 5 and clf.fit_status_ == 1 and 0 < len(clf.support_) <= 10
    assert clf.decision_function(X[:7]).shape == (7,)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert SVC(max_iter=100000).fit(X, y).n_iter_ == SVC().fit(X, y).n_iter_


@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_ties_keep_the_later_index(dev, kind):
    """Every row twice: both selections of the first iteration tie exactly between a row and its copy (G = -1 everywhere, and a kernel
    value depends on its two rows' values only), and libsvm's scans keep the later one.  The oracle makes the same first move.  With the
    linear kernel a row and its copy stay exchangeable bit for bit (K[i][i] = K[i][i'] = K[i'][i']), so the first 25 moves agree too; the
    RBF expansion gives K[i][i'] = 1 - O(2^-53) beside a diagonal of exactly 1, which breaks later ties by rounding, not by index."""
    from sklearn.exceptions import ConvergenceWarning
    X, y = O.make_data(40, 4, 1.0, 3)
    X2, y2 = np.concatenate([X, X]), np.concatenate([y, y])
    for max_iter in (1, 25) if kind == "linear" else (1,):
        with pytest.warns(ConvergenceWarning):
            clf = SVC(kernel=kind, gamma=0.25, max_iter=max_iter).fit(X2, y2)
        want = O.fit(X2, y2, 1.0, kind, 0.25, max_iter=max_iter)
        assert clf.n_iter_ == max_iter and np.array_equal(clf.support_, want["support_"])
        if max_iter == 1:
            assert len(clf.support_) == 2 and (clf.support_ >= 40).all()


def test_labels_of_any_kind_and_cuda_input(dev):
    X, y = O.make_data(130, 17, 0.7, 4)
    labels = np.where(y > 0, "pos", "neg")
    a, b = SVC().fit(X, y), SVC().fit(torch.from_numpy(X).cuda(), labels)
    assert list(b.classes_) == ["neg", "pos"] and np.array_equal(a.alpha_, b.alpha_)
    assert np.array_equal(b.predict(X) == "pos", a.predict(X) > 0)
    assert (a.predict(X) == y).mean() > 0.8
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a.decision_function(torch.zeros(2, 17))
