"""numpy float64 oracle for linear_model: scikit-learn's binary logistic-regression objective with its scaling,
    f(w, b) = 1/n sum_i log(1 + exp(s_i)) + |w|^2 / (2 C n),   s_i = -z_i (t_i = 1) or z_i (t_i = 0),   z = X w + b,
its gradient and Hessian, evaluated without overflow or cancellation, and a restatement of the damped Newton solver of csrc/logreg.hip
(scikit-learn's NewtonSolver rules).  theta = (w, b) holds d + 1 numbers when the intercept is fitted, d otherwise.
tests/test_logreg_cpu.py pins it to sklearn.linear_model.LogisticRegression; data comes from svc_oracle.make_data.

The objective is strictly convex, so two points are close when their gradients are: for the exact Hessian H between them
|theta_a - theta_b| = |H^-1 (g_a - g_b)|, and `distance_bound` is 2 |g_a - g_b|_2 / lambda_min(H(theta_b)), the factor 2 covering the
Hessian's change between the two points.  Error bounds of an evaluation in float64 (u = 2^-53): `z_bound`, `eval_bounds`."""
import functools

import numpy as np
from scipy.special import expit

from svc_oracle import make_data  # noqa: F401  (re-exported: the tests take their data from here)

U53 = 2.0 ** -53
SIGMA = 2.0 ** -11                 # Armijo factor
MAX_TRIALS = 21
LIP_W = 0.0963                     # max |d/dz expit(z) expit(-z)| = 1 / (6 sqrt 3)


def targets(y):
    """(classes, t in {0, 1}): 1 marks the second of the sorted classes."""
    classes = np.unique(y)
    assert len(classes) == 2
    return classes, np.where(np.asarray(y) == classes[1], 1.0, 0.0)


def split(theta, d, fit_intercept=True):
    theta = np.asarray(theta, dtype=np.float64)
    return theta[:d], (float(theta[d]) if fit_intercept else 0.0)


def rows(X, t, theta, fit_intercept=True):
    """(z, loss terms, r = p - t, w = p (1 - p)) per row."""
    X = np.asarray(X, dtype=np.float64)
    w_, b = split(theta, X.shape[1], fit_intercept)
    z = X @ w_ + b
    s = np.where(t > 0.5, -z, z)
    loss = np.log1p(np.exp(-np.abs(s))) + np.maximum(s, 0.0)
    r = np.where(t > 0.5, -expit(-z), expit(z))
    return z, loss, r, expit(z) * expit(-z)


def evaluate(X, t, theta, C, fit_intercept=True):
    """(f, g [p], H [p, p]) at theta."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    w_, _ = split(theta, d, fit_intercept)
    _, loss, r, w = rows(X, t, theta, fit_intercept)
    pen = 1.0 / (C * n)
    A = np.hstack([X, np.ones((n, 1))]) if fit_intercept else X
    f = loss.sum() / n + 0.5 * pen * (w_ @ w_)
    g = A.T @ r / n
    g[:d] += pen * w_
    H = (A.T * w) @ A / n
    H[np.arange(d), np.arange(d)] += pen
    return float(f), g, H


def gradient(X, t, theta, C, fit_intercept=True):
    return evaluate(X, t, theta, C, fit_intercept)[1]


def newton(X, t, C, tol=1e-4, max_iter=100, fit_intercept=True):
    """(theta, n_iter, status): start at 0; s = -H^-1 g by Cholesky; backtrack alpha = 1, 1/2, ... (at most 21 trials), accepting
    f' <= f + 2^-11 alpha g.s, or |f' - f| <= 16 eps |f| with a smaller 1-norm of the gradient; stop when max |g| <= tol.
    status: 0 converged, 1 max_iter, 2 line search failed, 3 non-positive pivot."""
    X = np.asarray(X, dtype=np.float64)
    p = X.shape[1] + int(fit_intercept)
    theta = np.zeros(p)
    f, g, H = evaluate(X, t, theta, C, fit_intercept)
    n_iter = 0
    while True:
        if np.abs(g).max() <= tol:
            return theta, n_iter, 0
        if n_iter >= max_iter:
            return theta, n_iter, 1
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return theta, n_iter, 3
        s = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        gts, g1, alpha = float(g @ s), np.abs(g).sum(), 1.0
        for _ in range(MAX_TRIALS):
            f2, g2, H2 = evaluate(X, t, theta + alpha * s, C, fit_intercept)
            if f2 - f <= SIGMA * alpha * gts or (abs(f2 - f) <= abs(f) * 16 * np.finfo(np.float64).eps and np.abs(g2).sum() < g1):
                break
            alpha *= 0.5
        else:
            return theta, n_iter, 2
        theta, f, g, H = theta + alpha * s, f2, g2, H2
        n_iter += 1


def distance_bound(X, t, theta_a, theta_b, C, fit_intercept=True, evaluation_error=False):
    """2 |g(theta_a) - g(theta_b)|_2 / lambda_min(H(theta_b)), both gradients recomputed here.  The recomputed gradients carry their own
    rounding error, so two points a few ulps apart can show equal gradients: `evaluation_error` adds both gradients' evaluation bounds
    (eval_bounds) to the numerator, which is what the true gradients' difference is bounded by.  It matters only where the distance itself
    is at rounding level (Newton against Newton); every comparison the bound was stated for is made without it."""
    ga = gradient(X, t, theta_a, C, fit_intercept)
    _, gb, Hb = evaluate(X, t, theta_b, C, fit_intercept)
    num = float(np.linalg.norm(ga - gb))
    if evaluation_error:
        num += float(np.linalg.norm(eval_bounds(X, t, theta_a, C, fit_intercept)["grad"]) + np.linalg.norm(eval_bounds(X, t, theta_b, C, fit_intercept)["grad"]))
    return 2.0 * num / float(np.linalg.eigvalsh(Hb)[0])


def z_bound(X, theta, fit_intercept=True):
    """B_z [n] = 2 (d + 2) u (|x| . |w| + |b|): a float64 dot product of d terms plus the intercept, in any order, here and there."""
    X = np.asarray(X, dtype=np.float64)
    w_, b = split(theta, X.shape[1], fit_intercept)
    return 2.0 * (X.shape[1] + 2) * U53 * (np.abs(X) @ np.abs(w_) + abs(b))


def eval_bounds(X, t, theta, C, fit_intercept=True):
    """Bounds on |got - oracle| for dict(z, loss_rows, r, w, loss, grad, hess) of one evaluation.  The loss, r and w are 1-, 1/4- and
    0.0963-Lipschitz in z and get 8 u relative for exp / log1p; a sum of m terms adds 2 (m + 1) u sum |term|."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    w_, _ = split(theta, d, fit_intercept)
    z, loss, r, w = rows(X, t, theta, fit_intercept)
    bz = z_bound(X, theta, fit_intercept)
    bl, br, bw = bz + 8 * U53 * np.abs(loss), 0.25 * bz + 8 * U53 * np.abs(r), LIP_W * bz + 8 * U53 * np.abs(w)
    A = np.abs(np.hstack([X, np.ones((n, 1))]) if fit_intercept else X)
    pen = 1.0 / (C * n)
    summed = 2.0 * (n + 1) * U53
    b_loss = (bl.sum() + summed * np.abs(loss).sum()) / n + 2.0 * (d + 2) * U53 * 0.5 * pen * (w_ @ w_)
    b_grad = (A.T @ br + summed * (A.T @ np.abs(r))) / n
    b_grad[:d] += 4 * U53 * pen * np.abs(w_)
    b_hess = ((A.T * bw) @ A + (summed + 2 * U53) * ((A.T * np.abs(w)) @ A)) / n
    b_hess[np.arange(d), np.arange(d)] += 4 * U53 * pen
    # one more rounding of each result (the division by n, the added penalty)
    f, g, H = evaluate(X, t, theta, C, fit_intercept)
    return dict(z=bz, loss_rows=bl, r=br, w=bw, loss=b_loss + 4 * U53 * abs(f), grad=b_grad + 4 * U53 * np.abs(g), hess=b_hess + 4 * U53 * np.abs(H))


@functools.lru_cache(maxsize=None)
def sklearn_fit(n, d, sep, C, solver="lbfgs", tol=1e-12, seed=1, fit_intercept=True):
    """scikit-learn's theta (w, b) on make_data(n, d, sep, seed)."""
    from sklearn.linear_model import LogisticRegression
    X, y = make_data(n, d, sep, seed)
    sk = LogisticRegression(C=C, tol=tol, max_iter=10000, solver=solver, fit_intercept=fit_intercept).fit(X, y)
    theta = np.concatenate([sk.coef_[0], sk.intercept_]) if fit_intercept else sk.coef_[0].copy()
    return sk, theta
