"""GPU: bbbp_svr_smo against the numpy oracle of tests/svr_oracle.py bit for bit, and svm.SVR / fit_svr_folds / grid_search_cv_svr against
single fits bit for bit and against scikit-learn within the scatter scikit-learn's own runs show (svr_oracle.sklearn_reference).

The solver's register form holds 1, 2 or 4 base rows per thread of a 1024-thread work-group, and beyond 4096 rows the state stays in
global memory: the sizes below stand on both sides of 1024, 2048 and 4096."""
import functools
import warnings

import numpy as np
import pytest
import torch

from bbbp_amd import ensemble, svm
from bbbp_amd.svm import SVR, fit_svr_folds, grid_search_cv_svr, kernel_matrix
import svr_oracle as O

pytestmark = pytest.mark.gpu

U53 = O.U53
NOISE = 0.3
RBF_CASES = [(300, 10, 1.0, 0.1), (300, 10, 10.0, 0.05), (130, 7, 0.1, 0.5), (333, 100, 1.0, 0.1)]          # (n, d, C, epsilon) of tests/test_svr_cpu.py


def _gamma(X):
    return O.gamma_scale(X) if X.shape[0] > 1 else 1.0


def _run(problems, **kw):
    out = svm._solve_svr(problems, **kw)
    return [(p.alpha.clone(), p.grad.clone(), p.rho.clone(), it, ok) for p, (it, ok) in zip(problems, out)]


def _same(a, b):
    return all(torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v for u, v in zip(a, b))


# (n, d, kernel, C, epsilon).  The linear problems keep C small where their iteration counts grow with it (333 x 100 at C = 1: 314 000).
SOLVER_CASES = [(1, 7, "rbf", 1.0, 0.1), (1, 7, "linear", 1.0, 0.1), (2, 7, "rbf", 1.0, 0.1), (2, 7, "linear", 1.0, 0.1), (63, 7, "rbf", 1.0, 0.1),
                (63, 7, "linear", 1.0, 0.1), (65, 7, "rbf", 1.0, 0.1), (65, 7, "linear", 1.0, 0.1), (130, 7, "rbf", 0.1, 0.5), (130, 7, "linear", 1.0, 0.1),
                (333, 100, "rbf", 1.0, 0.1), (333, 100, "linear", 0.1, 0.1), (300, 10, "rbf", 1.0, 0.0), (200, 10, "linear", 0.1, 0.0),
                (1024, 20, "rbf", 1.0, 0.1), (1025, 20, "rbf", 1.0, 0.1), (1100, 20, "rbf", 1.0, 0.1), (1100, 20, "linear", 0.1, 0.1),
                (2048, 20, "rbf", 1.0, 0.3), (2049, 20, "rbf", 1.0, 0.3), (2049, 20, "linear", 0.1, 0.3), (4096, 20, "rbf", 1.0, 0.3),
                (4097, 20, "rbf", 1.0, 0.3)]


@pytest.mark.parametrize("n,d,kind,C,epsilon", SOLVER_CASES)
def test_solver_equals_the_oracle_bit_for_bit(dev, n, d, kind, C, epsilon):
    """The oracle runs on the GPU's own kernel matrix, copied to the host: the same iteration count, and alpha and rho with equal bits."""
    X, t = O.make_data(n, d, NOISE, 1)
    K = kernel_matrix(torch.from_numpy(X).cuda(), kind, _gamma(X))[0]
    pr = svm._SvrProblem(K, torch.from_numpy(t).cuda(), C, epsilon, 1e-3)
    (n_iter, done), = svm._solve_svr([pr])
    alpha, rho, want_iter, ok = O.smo(K.cpu().numpy(), t, C, epsilon, 1e-3)
    got = pr.alpha.cpu().numpy()
    at_bound = int((got == C).sum())
    print(f"n {n} d {d} {kind} C {C} epsilon {epsilon}: {n_iter} iterations (oracle {want_iter}), {int((got > 0).sum())} of {2 * n} variables above 0, "
          f"{at_bound} at C")
    assert done and ok and n_iter == want_iter
    assert np.array_equal(got, alpha), f"alpha differs in {int((got != alpha).sum())} places, by at most {np.abs(got - alpha).max():.3g}"
    assert float(pr.rho.item()) == rho
    if (n, kind, C) == (130, "rbf", 0.1):
        assert at_bound >= 0.8 * int((got > 0).sum())            # the case with most variables at the bound


# (n, d, kernel, C, epsilon)
OPTIMALITY_CASES = [(300, 10, "rbf", 1.0, 0.1), (300, 10, "rbf", 10.0, 0.05), (333, 100, "rbf", 1.0, 0.1), (130, 7, "rbf", 0.1, 0.5), (200, 10, "linear", 0.1, 0.2),
                    (300, 10, "rbf", 1.0, 0.0)]


@pytest.mark.parametrize("tol", [1e-3, 1e-8])
@pytest.mark.parametrize("n,d,kind,C,epsilon", OPTIMALITY_CASES)
def test_solver_optimality(dev, n, d, kind, C, epsilon, tol):
    """Optimality recomputed in numpy from the GPU's own alpha, with the oracle's direct-difference kernel: independent of the path."""
    X, t = O.make_data(n, d, NOISE, 1)
    m = SVR(kind, C, epsilon, tol=tol).fit(X, t)
    alpha = m.alpha_
    assert alpha.shape == (2 * n,) and (alpha >= 0.0).all() and (alpha <= C).all()
    assert abs(alpha[:n].sum() - alpha[n:].sum()) <= 2 * n * C * U53 * 4
    gap, G = O.violation(O.kernel(X, X, kind, m._gamma), t, alpha, C, epsilon)
    print(f"{kind} n {n} C {C} epsilon {epsilon} tol {tol}: {m.n_iter_} iterations, m - M = {gap:.3g}")
    assert gap <= tol * (1 + 1e-6) + 1e-9
    assert abs(-m.intercept_[0] - O.rho_rule(O.signs(n), G, alpha, C)) <= 1e-9
    coef = alpha[:n] - alpha[n:]
    assert np.array_equal(m.support_, np.flatnonzero(coef != 0)) and m.support_.dtype == np.int32
    assert np.array_equal(m.dual_coef_, coef[m.support_][None, :]) and m.intercept_.shape == (1,)
    assert np.array_equal(m.n_support_, [len(m.support_)]) and np.array_equal(m.support_vectors_, X[m.support_])
    assert abs(m._gamma - O.gamma_scale(X)) <= 1e-14 * m._gamma and m.n_iter_ > 0 and m.fit_status_ == 0 and m.n_features_in_ == d


@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_batch_independence(dev, kind):
    """C x epsilon problems over one matrix equal the same problems alone, bit for bit -- also when the launches are cut to 7 iterations
    (the state survives the launch boundary), in reversed batch order, and through a row list into a larger matrix."""
    X, t = O.make_data(200, 10, NOISE, 1)
    Xd, td = torch.from_numpy(X).cuda(), torch.from_numpy(t).cuda()
    K = kernel_matrix(Xd, kind, O.gamma_scale(X))[0]
    grid = [(C, e) for C in ((0.1, 1.0) if kind == "rbf" else (0.05, 0.1)) for e in (0.05, 0.3)]
    make = lambda pts=grid, K=K, td=td, rows=None: [svm._SvrProblem(K, td, C, e, 1e-3, rows) for C, e in pts]  # noqa: E731
    together = _run(make())
    assert all(ok for *_, ok in together) and len({it for *_, it, _ in together}) > 1
    for pt, want in zip(grid, together):
        assert _same(_run(make([pt]))[0], want), f"{kind} {pt}: alone differs from the batch"
    assert all(_same(a, b) for a, b in zip(_run(make()), together)), "a repeat run differs"
    assert all(_same(a, b) for a, b in zip(_run(make(grid[::-1])), together[::-1])), "the reversed batch differs"
    assert all(_same(a, b) for a, b in zip(_run(make(), iters_per_launch=7), together)), "launches of 7 iterations differ"
    # a fold as a row list into the shared matrix = the fold's own matrix
    rows = np.flatnonzero(np.arange(200) % 5 != 2)
    rd = torch.from_numpy(rows).cuda()
    sub, ts = K[rd][:, rd].contiguous(), td[rd].contiguous()
    own = _run(make(K=sub, td=ts))
    listed = _run(make(td=ts, rows=rd.to(torch.int32)))
    assert all(_same(a, b) for a, b in zip(own, listed)), "a row list differs from the sub-matrix"
    assert all(_same(a, b) for a, b in zip(_run(make(td=ts, rows=rd.to(torch.int32)), iters_per_launch=7), listed))


def test_a_batch_of_mixed_sizes(dev):
    """Problems of different register forms in one call (130, 1100, 130, 2049 and 4097 rows) and more than one launch's 32 descriptors:
    each equals itself alone."""
    mats = {}
    for n in (130, 1100, 2049, 4097):
        X, t = O.make_data(n, 20, NOISE, 1)
        mats[n] = (kernel_matrix(torch.from_numpy(X).cuda(), "rbf", O.gamma_scale(X))[0], torch.from_numpy(t).cuda())
    make = lambda n, C=1.0: svm._SvrProblem(*mats[n], C, 0.3, 1e-3)  # noqa: E731
    order = (130, 1100, 130, 2049, 4097)
    together = _run([make(n) for n in order], max_iter=300)
    for n, want in zip(order, together):
        assert _same(_run([make(n)], max_iter=300)[0], want), f"n {n}: alone differs from the mixed batch"
    Cs = [0.05 + 0.05 * q for q in range(40)]
    many = _run([make(130, C) for C in Cs])
    assert all(ok for *_, ok in many)
    for q in (0, 31, 32, 39):
        assert _same(_run([make(130, Cs[q])])[0], many[q]), f"problem {q} of 40 differs from itself alone"


def _assert_same_model(a, b, Q):
    assert np.array_equal(a.alpha_, b.alpha_) and a.n_iter_ == b.n_iter_ and a.intercept_[0] == b.intercept_[0] and a.fit_status_ == b.fit_status_
    assert np.array_equal(a.support_, b.support_) and np.array_equal(a.dual_coef_, b.dual_coef_)
    assert np.array_equal(a.support_vectors_, b.support_vectors_) and a._gamma == b._gamma
    assert np.array_equal(a.predict(Q), b.predict(Q))


@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_fit_svr_folds_equals_single_fits(dev, kind):
    from sklearn.model_selection import KFold
    X, t = O.make_data(203, 10, NOISE, 1)
    Q, _ = O.make_data(50, 10, NOISE, 2)
    params = dict(kernel=kind, C=1.0 if kind == "rbf" else 0.1, epsilon=0.1)
    folds = list(KFold(n_splits=5, shuffle=True, random_state=42).split(X))      # the reference's folds
    models = fit_svr_folds(X, t, folds, **params)
    assert len(models) == 5
    for (tr, _), m in zip(folds, models):
        _assert_same_model(m, SVR(**params).fit(X[tr], t[tr]), Q)
    for a, b in zip(fit_svr_folds(X.astype(np.float32), t, [tr for tr, _ in folds], **params), fit_svr_folds(X.astype(np.float32).astype(np.float64), t, folds, **params)):
        assert np.array_equal(a.alpha_, b.alpha_)                                # plain index arrays; float32 rows are the same numbers


GRID = [{"C": [0.1, 1, 10], "epsilon": [0.05], "gamma": ["scale", 0.3]}, {"C": [0.1], "epsilon": [0.5], "kernel": ["linear"]}]


@functools.lru_cache(maxsize=None)
def _grid_run():
    X, t = O.make_data(200, 10, NOISE, 1)
    return X, t, grid_search_cv_svr(X, t, GRID, cv=5)


def _grid_points():
    from sklearn.model_selection import ParameterGrid
    return list(ParameterGrid(GRID))


def test_grid_search_cv_svr_equals_single_fits(dev):
    from sklearn.metrics import r2_score
    from sklearn.model_selection import KFold
    X, t, (best, scores, fitted) = _grid_run()
    points = _grid_points()
    want = np.zeros((len(points), 5))
    for fi, (tr, te) in enumerate(KFold(n_splits=5).split(X)):
        for pi, pt in enumerate(points):
            want[pi, fi] = r2_score(t[te], SVR(**pt).fit(X[tr], t[tr]).predict(X[te]))
    assert scores == [float(v) for v in want.mean(axis=1)]
    assert best == points[int(np.argmax(scores))]
    _assert_same_model(fitted, SVR(**best).fit(X, t), X[:20])
    assert (fitted.C, fitted.epsilon, fitted.kernel) == (best["C"], best["epsilon"], best.get("kernel", "rbf"))


def test_grid_search_cv_svr_against_sklearn(dev):
    """The chosen point is scikit-learn's.  Margin: a prediction that moves by at most delta moves a fold's R^2 = 1 - SSE / SST by at most
    (2 delta sum |e_i| + m delta^2) / SST, e the m residuals of scikit-learn's own fit on the fold; both the best and the second-best point
    may move, towards each other.  delta is the largest tolerance svr_oracle.sklearn_reference measures over the grid's points (on its
    300 x 10 problem: the same data family, half as many rows again as a fold).  The grid is chosen so that scikit-learn's best and
    second-best mean R^2 differ by more than twice the mean over the folds of that bound."""
    from sklearn.model_selection import GridSearchCV, KFold
    from sklearn.svm import SVR as SkSVR
    X, t, (best, scores, _) = _grid_run()
    sk = GridSearchCV(SkSVR(), GRID, cv=5).fit(X, t)
    want = sk.cv_results_["mean_test_score"]
    points = _grid_points()
    assert sk.cv_results_["params"] == points
    delta = max(O.sklearn_reference(300, 10, NOISE, pt.get("kernel", "rbf"), float(pt["C"]), pt["epsilon"])[2] for pt in points)
    order = np.argsort(want)
    slack = []
    for pi in order[-2:]:
        per_fold = []
        for tr, te in KFold(n_splits=5).split(X):
            e = t[te] - SkSVR(**points[pi]).fit(X[tr], t[tr]).predict(X[te])
            per_fold.append((2 * delta * np.abs(e).sum() + len(te) * delta ** 2) / ((t[te] - t[te].mean()) ** 2).sum())
        slack.append(float(np.mean(per_fold)))
    margin = want[order[-1]] - want[order[-2]]
    print(f"scores {scores}\nscikit-learn {list(want)}\ndelta {delta:.3g}, slack {slack}, margin {margin:.3g}, largest score difference {np.abs(np.asarray(scores) - want).max():.3g}")
    assert margin > sum(slack), "the grid does not separate its two best points by more than the measured tolerance allows"
    assert best == sk.best_params_
    for pi, bound in zip(order[-2:], slack):
        assert abs(scores[pi] - want[pi]) <= bound


@pytest.mark.parametrize("n,d,C,epsilon", RBF_CASES)
def test_svr_against_sklearn(dev, n, d, C, epsilon):
    sk, want, tolerance = O.sklearn_reference(n, d, NOISE, "rbf", C, epsilon)
    X, t = O.make_data(n, d, NOISE, 1)
    Q, _ = O.make_data(200, d, NOISE, 2)
    m = SVR(C=C, epsilon=epsilon).fit(X, t)
    got = m.predict(Q)
    print(f"n {n} d {d} C {C} epsilon {epsilon}: tolerance {tolerance:.3g}, largest difference {np.abs(got - want).max():.3g}, intercept difference "
          f"{abs(m.intercept_[0] - sk.intercept_[0]):.3g}, {m.n_iter_} iterations (scikit-learn {int(np.ravel(sk.n_iter_)[0])}), "
          f"{len(m.support_)} support vectors (scikit-learn {len(sk.support_)})")
    assert np.abs(got - want).max() <= tolerance
    assert abs(m.intercept_[0] - sk.intercept_[0]) <= tolerance
    assert abs(m._gamma - sk._gamma) <= 1e-14 * sk._gamma


@functools.lru_cache(maxsize=None)
def _fitted(kind, f32):
    n, d = (333, 100) if kind == "rbf" else (200, 10)
    X, t = O.make_data(n, d, NOISE, 1)
    if f32:
        X = X.astype(np.float32)
    return X, (SVR() if kind == "rbf" else SVR("linear", 0.1, 0.2)).fit(X, t)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_decision_path(dev, kind, f32):
    """predict against a numpy float64 sum over the GPU's own dual_coef_ and support_vectors_, with test_gpu_svc.test_decision_function's
    bound: every kernel value's own bound times |coef|, plus the n_SV-term sum bound of both sides, plus the rounding of the intercept's
    addition.  float32 and float64 rows, CUDA and numpy input, and queries that are a column slice of a wider matrix."""
    X, m = _fitted(kind, f32)
    sv, coef, b, g = m.support_vectors_.astype(np.float64), m.dual_coef_[0], m.intercept_[0], m._gamma
    assert m.support_vectors_.dtype == X.dtype
    mu = X.astype(np.float64).mean(axis=0)
    Qall, _ = O.make_data(130, X.shape[1], NOISE, 2)
    Qall = Qall.astype(X.dtype)
    wide = torch.zeros(130, X.shape[1] + 13, dtype=torch.from_numpy(Qall).dtype, device="cuda")
    wide[:, :X.shape[1]] = torch.from_numpy(Qall).cuda()
    for rows in (1, 63, 65, 130):
        Q = Qall[:rows].astype(np.float64)
        Kq = O.kernel(Q, sv, kind, g)
        want = Kq @ coef + b
        if kind == "linear":
            kerr = 2.0 * (Q.shape[1] + 1) * U53 * (np.abs(Q) @ np.abs(sv).T)
        else:
            B = 4.0 * (Q.shape[1] + 4) * U53 * (((Q - mu) ** 2).sum(axis=1)[:, None] + ((sv - mu) ** 2).sum(axis=1)[None, :])
            kerr = (g * B + 8.0 * U53) * Kq
        limit = kerr @ np.abs(coef) + 2.0 * (len(coef) + 2) * U53 * (np.abs(Kq) @ np.abs(coef)) + 2.0 * U53 * np.abs(want)
        Qd = torch.from_numpy(Qall[:rows]).cuda()
        first = m.predict(Qd)
        assert first.is_cuda and first.dtype == torch.float64 and first.shape == (rows,)
        err = np.abs(first.cpu().numpy() - want)
        assert (err <= limit).all(), f"{kind} rows {rows}: worst error / bound = {(err / limit).max():.3g}"
        got = m.predict(Qall[:rows])
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, first.cpu().numpy())
        padded = wide[:rows, :X.shape[1]]
        assert rows == 1 or padded.stride(0) == X.shape[1] + 13
        assert torch.equal(m.predict(padded), first) and torch.equal(m.predict_device(Qall[:rows]), first)
        for s in (1, 2, 7):
            assert torch.equal(m.predict_device(Qd, slices=s), first)
    with pytest.raises(ValueError, match="features"):
        m.predict(Qall[:5, :-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(torch.zeros(2, X.shape[1]))


def test_no_support_vectors_predicts_the_intercept(dev):
    """A tube wider than the targets' range: alpha stays 0, no iteration runs and predict returns -rho, the midpoint of the bounds."""
    X, t = O.make_data(65, 7, NOISE, 1)
    m = SVR(epsilon=100.0).fit(X, t)
    assert m.n_iter_ == 0 and m.fit_status_ == 0 and len(m.support_) == 0 and m.dual_coef_.shape == (1, 0) and m.support_vectors_.shape == (0, 7)
    assert abs(m.intercept_[0] - (t.max() + t.min()) / 2) <= 2 * U53 * 100.0            # the roundings of epsilon -+ t at |epsilon -+ t| < 128
    assert np.array_equal(m.predict(X[:5]), np.full(5, m.intercept_[0]))


def test_max_iter_stops_with_a_warning(dev):
    from sklearn.exceptions import ConvergenceWarning
    X, t = O.make_data(333, 100, NOISE, 1)
    with pytest.warns(ConvergenceWarning):
        m = SVR(max_iter=5).fit(X, t)
    assert m.n_iter_ == 5 and m.fit_status_ == 1 and 0 < len(m.support_) <= 10
    assert m.predict(X[:7]).shape == (7,)
    want = O.smo(kernel_matrix(torch.from_numpy(X).cuda(), "rbf", O.gamma_scale(X))[0].cpu().numpy(), t, 1.0, 0.1, max_iter=5)
    assert np.array_equal(m.alpha_, want[0]) and -m.intercept_[0] == want[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert SVR(max_iter=100000).fit(X, t).n_iter_ == SVR().fit(X, t).n_iter_


def test_stacking_regressor_takes_svr_as_a_base_learner(dev):
    """ensemble.StackingRegressor clones and fits SVR like any scikit-learn regressor; the result is the stack assembled by hand from
    single fits: the full-data model, the out-of-fold column of unshuffled KFold(5), and the final linear model on it."""
    from sklearn.model_selection import KFold
    X, t = O.make_data(203, 10, NOISE, 1)
    Q, _ = O.make_data(50, 10, NOISE, 2)
    stack = ensemble.StackingRegressor([("svr", SVR())]).fit(X, t)
    meta = np.zeros((203, 1))
    for tr, te in KFold(n_splits=5).split(X):
        meta[te, 0] = SVR().fit(X[tr], t[tr]).predict(X[te])
    final = ensemble.StackedEnsemble(0.0).fit(meta, t)
    base = SVR().fit(X, t)
    assert np.array_equal(stack.estimators_[0][1].alpha_, base.alpha_)
    assert np.array_equal(stack.final_estimator_.coef_, final.coef_) and stack.final_estimator_.intercept_ == final.intercept_
    assert np.array_equal(stack.predict(Q), final.predict(base.predict(Q)[:, None]))
    ridge = ensemble.StackingRegressor([("svr", SVR(C=3)), ("svr_linear", SVR("linear", 0.1))], final_estimator=ensemble.StackedEnsemble(1.0)).fit(X, t)
    assert ridge.predict(Q).shape == (50,) and ridge.estimators_[0][1].C == 3 and ridge.final_estimator_.alpha == 1.0


@pytest.mark.parametrize("kind", ["rbf", "linear"])
def test_ties_keep_the_later_index(dev, kind):
    """Every (row, target) twice: both selections of the first iteration tie exactly between a row and its copy, and the first move is the
    oracle's: the later copies, variable i in [40, 80) of the first half and j in [120, 160) of the second.  With the linear kernel a row
    and its copy stay exchangeable bit for bit, so the first 25 moves agree too (test_gpu_svc.test_ties_keep_the_later_index)."""
    from sklearn.exceptions import ConvergenceWarning
    X, t = O.make_data(40, 4, NOISE, 3)
    X2, t2 = np.concatenate([X, X]), np.concatenate([t, t])
    for max_iter in (1, 25) if kind == "linear" else (1,):
        with pytest.warns(ConvergenceWarning):
            m = SVR(kind, gamma=0.25, max_iter=max_iter).fit(X2, t2)
        want = O.fit(X2, t2, 1.0, 0.1, kind, 0.25, max_iter=max_iter)
        assert m.n_iter_ == max_iter and np.array_equal(m.support_, want["support_"])
        assert np.array_equal(np.flatnonzero(m.alpha_ > 0), np.flatnonzero(want["alpha"] > 0))
        if max_iter == 1:
            moved = np.flatnonzero(m.alpha_ > 0)
            assert len(moved) == 2 and moved[0] in range(40, 80) and moved[1] in range(120, 160)


def test_targets_of_any_real_kind_and_cuda_input(dev):
    X, t = O.make_data(130, 17, NOISE, 4)
    a = SVR().fit(X, t)
    b = SVR().fit(torch.from_numpy(X).cuda(), torch.from_numpy(t).cuda())
    c = SVR().fit(X, list(t))
    assert np.array_equal(a.alpha_, b.alpha_) and np.array_equal(a.alpha_, c.alpha_)
    ints = SVR().fit(X, np.round(3 * t).astype(np.int64))
    assert np.array_equal(ints.alpha_, SVR().fit(X, np.round(3 * t)).alpha_)
    assert 1.0 - ((a.predict(X) - t) ** 2).sum() / ((t - t.mean()) ** 2).sum() > 0.5
    with pytest.raises(ValueError, match="rows"):
        SVR().fit(X, t[:-1])
    Xb = X.copy()
    Xb[3, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        SVR().fit(Xb, t)
