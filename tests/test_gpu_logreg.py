"""GPU: linear_model.LogisticRegression (csrc/logreg.hip) against the numpy oracle (tests/logreg_oracle.py) and scikit-learn.

Shapes: n in {1, 7, 63, 65, 130, 333} (below, across and beyond one 64-row block of the row pass), d in {1, 3, 17, 100, 167, 255} (one to
four 64-column tiles of the Gram matrix; p = d + 1 <= 112 is factored in LDS, beyond that in device memory), plus n = 600, the smallest
size class with more than one 512-row slab of the Gram matrix.  Operands are [:n, :d] views of a wider pool, float32 and float64, with
values exact in float32.  Every bound is derived in logreg_oracle; u = 2^-53."""
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy.special import expit

import logreg_oracle as O
from bbbp_amd import linear_model as LM

pytestmark = pytest.mark.gpu

U = O.U53
EVAL_SHAPES = [(1, 1), (7, 3), (63, 17), (65, 100), (130, 167), (333, 255), (333, 100), (130, 1), (600, 17), (600, 167)]
FIT_PROBLEMS = [(200, 10, 0.7), (333, 100, 0.5), (63, 3, 3.0), (130, 167, 0.5), (333, 255, 0.5), (600, 17, 0.7), (7, 1, 0.7)]
SKLEARN_PROBLEMS = [(200, 10, 0.7), (333, 100, 0.5), (63, 3, 3.0)]


def view(X, dev, dtype=torch.float64):
    """X as the [:n, :d] corner of a wider device matrix (unit inner stride, a larger row stride)."""
    n, d = X.shape
    pool = torch.full((n + 3, d + 5), 7.0, dtype=dtype, device=dev)
    pool[:n, :d] = torch.from_numpy(np.ascontiguousarray(X)).to(dev).to(dtype)
    v = pool[:n, :d]
    assert v.stride(0) == d + 5
    return v


@functools.lru_cache(maxsize=None)
def data32(n, d, sep=0.7, seed=1):
    """make_data with X rounded to float32, so that both dtypes hold the same numbers."""
    X, y = O.make_data(n, d, sep, seed)
    if n == 1:
        y = np.array([1.0])
    return X.astype(np.float32).astype(np.float64), y


def quiet_fit(clf, X, y):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return clf.fit(X, y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,d", EVAL_SHAPES)
def test_evaluation_against_the_oracle(dev, n, d, dtype):
    """z, r, w, loss, gradient and Hessian at a given theta, at moderate z and with theta scaled until |z| reaches 800, with and without
    the intercept: within B_z = 2 (d + 2) u (|x|.|w| + |b|) for z; the loss, r and w 1-, 1/4- and 0.0963-Lipschitz in z plus 8 u relative;
    a sum of m terms adds 2 (m + 1) u sum |term|."""
    X, y = data32(n, d)
    t = np.where(y > 0, 1.0, 0.0)
    Xv = view(X, dev, dtype)
    theta0 = 0.3 * np.random.RandomState(n + d).randn(d + 1)
    zmax = np.abs(O.rows(X, t, theta0)[0]).max()
    for theta, C, fit_intercept in ((theta0, 1.0, True), (theta0 * (800.0 / zmax), 0.1, True), (theta0, 10.0, False)):
        got = LM._evaluate(Xv, t, theta, C, fit_intercept, dev)
        z, _, r, w = O.rows(X, t, theta, fit_intercept)
        f, g, H = O.evaluate(X, t, theta, C, fit_intercept)
        B = O.eval_bounds(X, t, theta, C, fit_intercept)
        assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all() and np.isfinite(got["hess"]).all()
        worst = {k: float((np.abs(a - b) / np.maximum(B[k], 1e-300)).max())
                 for k, a, b in (("z", got["z"], z), ("r", got["r"], r), ("w", got["w"], w), ("loss", got["loss"], f), ("grad", got["grad"], g),
                                 ("hess", got["hess"], H))}
        print(f"n {n} d {d} {dtype} max|z| {np.abs(z).max():.3g}: error / bound {worst}")
        assert (np.abs(got["z"] - z) <= B["z"]).all()
        assert (np.abs(got["r"] - r) <= B["r"]).all() and (np.abs(got["w"] - w) <= B["w"]).all()
        assert abs(got["loss"] - f) <= B["loss"]
        assert (np.abs(got["grad"] - g) <= B["grad"]).all()
        assert (np.abs(got["hess"] - H) <= B["hess"]).all()
        assert np.array_equal(got["hess"], got["hess"].T) and got["grad"].shape == (d + int(fit_intercept),)


@pytest.mark.parametrize("n,d,sep", FIT_PROBLEMS)
def test_optimality(dev, n, d, sep):
    """max |grad f| recomputed in numpy from coef_ and intercept_ is at most tol plus the gradient's own evaluation bound; the fit takes
    at least one step and does not warn; also without the intercept."""
    X, y = data32(n, d, sep)
    classes, t = O.targets(y)
    Xv = view(X, dev)
    for tol in (1e-4, 1e-10):
        for C, fit_intercept in ((0.1, True), (1.0, True), (10.0, True), (1.0, False)):
            clf = quiet_fit(LM.LogisticRegression(C=C, tol=tol, fit_intercept=fit_intercept, device=dev), Xv, y)
            assert clf.coef_.shape == (1, d) and clf.intercept_.shape == (1,) and clf.n_iter_.shape == (1,) and clf.n_features_in_ == d
            assert np.array_equal(clf.classes_, classes) and clf.n_iter_[0] > 0 and clf.fit_status_ == 0
            assert fit_intercept or clf.intercept_[0] == 0.0
            theta = np.concatenate([clf.coef_[0], clf.intercept_]) if fit_intercept else clf.coef_[0]
            g = O.gradient(X, t, theta, C, fit_intercept)
            B = O.eval_bounds(X, t, theta, C, fit_intercept)["grad"]
            print(f"n {n} d {d} C {C} tol {tol} intercept {fit_intercept}: n_iter {clf.n_iter_[0]}, max |g| {np.abs(g).max():.3g}, bound on g {B.max():.3g}")
            assert (np.abs(g) <= tol + B).all()


@pytest.mark.parametrize("n,d,sep", SKLEARN_PROBLEMS)
def test_against_sklearn(dev, n, d, sep):
    """At tol = 1e-10 on both sides: |theta - theta_sklearn|_2 <= 2 |g(theta) - g(theta_sklearn)|_2 / lambda_min(H(theta_sklearn)),
    both gradients recomputed by the oracle, against scikit-learn's default solver (lbfgs).  Against its newton-cholesky the two points
    are one or two ulps apart (measured: 1.4e-16 on the separable problem, with bitwise equal recomputed gradients, so the bare bound is 0):
    there the gradients' own evaluation bounds join the numerator, see logreg_oracle.distance_bound."""
    X, y = O.make_data(n, d, sep, 1)
    classes, t = O.targets(y)
    Xv = view(X, dev)
    for C in (0.1, 1.0, 10.0):
        for solver in ("lbfgs", "newton-cholesky"):
            sk, ref = O.sklearn_fit(n, d, sep, C, solver, 1e-10)
            clf = quiet_fit(LM.LogisticRegression(C=C, tol=1e-10, solver=solver, device=dev), Xv, y)
            theta = np.concatenate([clf.coef_[0], clf.intercept_])
            dist, bound = float(np.linalg.norm(theta - ref)), O.distance_bound(X, t, theta, ref, C, evaluation_error=solver != "lbfgs")
            print(f"n {n} d {d} C {C} {solver}: n_iter {clf.n_iter_[0]} (scikit-learn {sk.n_iter_[0]}), |d theta| {dist:.3g}, bound {bound:.3g}")
            assert np.array_equal(clf.classes_, sk.classes_)
            assert dist <= bound
            Q, _ = O.make_data(50, d, sep, 2)
            assert (clf.predict(Q) == sk.predict(Q)).mean() >= 0.98 and clf.predict(Q).dtype == sk.predict(Q).dtype


def _batch(dev):
    """16 problems of mixed shape, dtype, C, tol and intercept: (X view, t on the device, C, tol, fit_intercept)."""
    out = []
    shapes = [(63, 3, 3.0), (65, 17, 0.7), (130, 100, 0.5), (333, 167, 0.5), (7, 3, 0.7), (200, 10, 0.7), (600, 17, 0.7), (130, 255, 0.5)]
    for i, (n, d, sep) in enumerate(shapes):
        X, y = data32(n, d, sep)
        _, t = O.targets(y)
        t_d = torch.from_numpy(t).to(dev)
        out.append((view(X, dev, torch.float32 if i % 2 else torch.float64), t_d, (0.1, 1.0, 10.0)[i % 3], 1e-10, True))
        out.append((view(X, dev, torch.float64 if i % 2 else torch.float32), t_d, (10.0, 0.1, 1.0)[i % 3], 1e-4, i % 4 != 3))
    return out


def _run(specs, order, rounds_per_sync=None):
    problems = [LM._Problem(specs[q][0], specs[q][1], specs[q][2], specs[q][3], 100, specs[q][4]) for q in order]
    solved = LM._solve(problems, rounds_per_sync)
    torch.cuda.synchronize()
    return {q: (pr.theta.cpu().numpy().tobytes(), s) for q, pr, s in zip(order, problems, solved)}


def test_batch_independence_bit_for_bit(dev):
    """16 problems together, the same reversed, and the same cut into rounds of 1 each equal the problem solved alone, bit for bit."""
    specs = _batch(dev)
    with torch.cuda.device(dev):
        alone = {}
        for q in range(len(specs)):
            alone.update(_run(specs, [q]))
        assert all(n_iter > 0 and status == 0 for _, (n_iter, status) in alone.values())
        assert len({v[0] for v in alone.values()}) == len(specs)                 # 16 different answers
        assert _run(specs, list(range(len(specs)))) == alone
        assert _run(specs, list(range(len(specs)))[::-1]) == alone
        assert _run(specs, list(range(len(specs))), rounds_per_sync=1) == alone
        assert _run(specs, list(range(len(specs))) + [0, 5, 9], rounds_per_sync=7) == alone       # 19 problems: two launches per kernel


def test_grid_search(dev):
    """The reference's grid on make_data(200, 10, 0.7, 1), tol = 1e-10 on both sides: every score is the single fit's on that fold, the
    scores equal scikit-learn's mean_test_score and the best point agrees -- given that no held-out row lies within 1e-4 of the boundary
    in scikit-learn's own fits, which is asserted for every row."""
    from sklearn.linear_model import LogisticRegression as SkLR
    from sklearn.metrics import f1_score
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    X, y = O.make_data(200, 10, 0.7, 1)
    grid = {"C": [0.1, 1, 10], "penalty": ["l2"]}
    best, scores, fitted = LM.grid_search_cv(X, y, grid, cv=5, device=dev, tol=1e-10, max_iter=1000)
    sk = GridSearchCV(SkLR(max_iter=1000, tol=1e-10), grid, cv=5, scoring="f1").fit(X, y)
    margin, single = np.inf, np.zeros((3, 5))
    for fi, (tr, te) in enumerate(StratifiedKFold(n_splits=5).split(X, y)):
        for ci, C in enumerate(grid["C"]):
            margin = min(margin, np.abs(SkLR(C=C, max_iter=1000, tol=1e-10).fit(X[tr], y[tr]).decision_function(X[te])).min())
            clf = quiet_fit(LM.LogisticRegression(C=C, tol=1e-10, max_iter=1000, device=dev), X[tr], y[tr])
            single[ci, fi] = f1_score(y[te], clf.predict(X[te]), pos_label=1.0)
    print(f"scores {scores}, scikit-learn {list(sk.cv_results_['mean_test_score'])}, best {best}, smallest held-out |decision| {margin:.3g}")
    assert margin >= 1e-4
    assert scores == [float(v) for v in single.mean(axis=1)]
    assert scores == [float(v) for v in sk.cv_results_["mean_test_score"]]
    assert [dict(p) for p in sk.cv_results_["params"]] == [{"C": C, "penalty": "l2"} for C in grid["C"]]
    assert best == sk.best_params_ and scores.index(max(scores)) == sk.best_index_
    alone = quiet_fit(LM.LogisticRegression(C=best["C"], tol=1e-10, max_iter=1000, device=dev), X, y)
    assert np.array_equal(fitted.coef_, alone.coef_) and np.array_equal(fitted.intercept_, alone.intercept_)
    # a list of grids runs one after the other; a missing key takes the default
    best2, scores2, _ = LM.grid_search_cv(X.astype(np.float32), y, [{"C": [1.0]}, {"penalty": ["l2"], "C": [10, 0.1]}], cv=3, device=dev)
    assert len(scores2) == 3 and best2 in ({"C": 1.0}, {"C": 10, "penalty": "l2"}, {"C": 0.1, "penalty": "l2"})


def test_probabilities_queries_and_labels(dev):
    """predict_proba is [1 - p, p] with p = expit(decision) within 4 u and rows summing to 1 within u; a float32 query and its float64
    copy give equal decision values; training rows' decision values are bitwise those of the solver's last evaluation; string labels and
    CUDA input reproduce the numeric fit bitwise."""
    X, y = data32(130, 17, 0.7)
    clf = quiet_fit(LM.LogisticRegression(C=1.0, tol=1e-8, device=dev), X, y)
    Q = np.concatenate([data32(65, 17, 0.7, 2)[0], 32.0 * data32(7, 17, 0.7, 3)[0]])       # the scaled rows (still exact in float32) reach p = 0 and p = 1
    z = clf.decision_function(Q)
    proba = clf.predict_proba(Q)
    assert isinstance(z, np.ndarray) and z.dtype == np.float64 and z.shape == (72,) and proba.shape == (72, 2)
    print(f"max |p - expit(z)| / u = {np.abs(proba[:, 1] - expit(z)).max() / U:.3g}, |z| up to {np.abs(z).max():.3g}")
    assert np.abs(proba[:, 1] - expit(z)).max() <= 4 * U and np.abs(proba[:, 0] - expit(-z)).max() <= 4 * U
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= U
    logp = clf.predict_log_proba(Q)
    assert np.isfinite(logp).all() and np.abs(logp[:, 1] - (-np.logaddexp(0.0, -z))).max() <= 8 * U * (1 + np.abs(z).max())
    assert np.array_equal(clf.predict(Q), clf.classes_[(z > 0).astype(int)])
    assert (np.abs(z - (Q @ clf.coef_[0] + clf.intercept_[0])) <= O.z_bound(Q, np.concatenate([clf.coef_[0], clf.intercept_]))).all()

    z32 = clf.decision_function(Q.astype(np.float32))
    assert np.array_equal(z32, z)
    zt = clf.decision_function(view(Q, dev, torch.float32))
    assert isinstance(zt, torch.Tensor) and zt.is_cuda and zt.dtype == torch.float64 and np.array_equal(zt.cpu().numpy(), z)
    pt = clf.predict_proba(view(Q, dev))
    assert isinstance(pt, torch.Tensor) and pt.is_cuda and np.array_equal(pt.cpu().numpy(), proba)
    assert clf.decision_function(np.zeros((0, 17))).shape == (0,)
    with pytest.raises(ValueError, match="features"):
        clf.decision_function(np.zeros((3, 16)))

    # the decision values of the training rows are those of the solver's last evaluation (an evaluation at the fitted theta)
    theta = np.concatenate([clf.coef_[0], clf.intercept_])
    seen = LM._evaluate(X, np.where(y > 0, 1.0, 0.0), theta, 1.0, True, dev)["z"]
    assert np.array_equal(clf.decision_function(X), seen)

    labels = np.where(y > 0, "pos", "neg")
    for Xin, yin in ((X, labels), (view(X, dev), y), (X.astype(np.float32), y), (view(X, dev, torch.float32), labels)):
        other = quiet_fit(LM.LogisticRegression(C=1.0, tol=1e-8, device=dev), Xin, yin)
        assert np.array_equal(other.coef_, clf.coef_) and np.array_equal(other.intercept_, clf.intercept_) and other.n_iter_[0] == clf.n_iter_[0]
    assert list(other.classes_) == ["neg", "pos"] and set(other.predict(Q[:9])) <= {"neg", "pos"}
    assert np.array_equal(other.predict(Q) == "pos", clf.predict(Q) > 0)


def test_max_iter_and_refusals(dev):
    """max_iter = 2 warns, leaves n_iter_ == 2 and still predicts; non-finite X, more than 255 features and one class are refused."""
    from sklearn.exceptions import ConvergenceWarning
    X, y = data32(63, 3, 3.0)
    with pytest.warns(ConvergenceWarning, match="max_iter"):
        clf = LM.LogisticRegression(C=10.0, tol=1e-10, max_iter=2, device=dev).fit(X, y)
    assert clf.n_iter_[0] == 2 and clf.fit_status_ == 1
    assert (clf.predict(X) == y).mean() > 0.9 and clf.predict_proba(X).shape == (63, 2)
    assert O.newton(X, np.where(y > 0, 1.0, 0.0), 10.0, tol=1e-10, max_iter=2)[1:] == (2, 1)
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[5, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            LM.LogisticRegression(device=dev).fit(Xb, y)
        with pytest.raises(ValueError, match="NaN or infinity"):
            LM.grid_search_cv(Xb, y, {"C": [1.0]}, cv=3, device=dev)
    with pytest.raises(ValueError, match="255"):
        LM.LogisticRegression(device=dev).fit(np.zeros((8, 256)), [0, 1] * 4)
    with pytest.raises(ValueError, match="classes"):
        LM.LogisticRegression(device=dev).fit(torch.zeros(8, 4, device=dev), np.zeros(8))
    with pytest.raises(ValueError, match="rows"):
        LM.LogisticRegression(device=dev).fit(np.zeros((8, 4)), [0, 1, 0])
