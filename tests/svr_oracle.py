"""numpy float64 oracle for svm.SVR: seeded regression data and a restatement of libsvm's epsilon-SVR solver without shrinking.

The dual has 2n variables over the n x n kernel matrix: variable k < n is alpha_k (sign s = +1, linear term epsilon - t_k), variable k + n is
alpha*_k (s = -1, linear term epsilon + t_k), Q[k][l] = s_k s_l K[k mod n][l mod n].  Selection (second order, Fan, Chen and Lin), libsvm's
clipping, tau = 1e-12, the stop rule m(alpha) - M(alpha) < tol and rho are svc_oracle's with s in the place of y; ties go to the later
index of the 2n ordering, so k + n beats k.  The kernels, rho's rule and the later arg-max are svc_oracle's own.

Rounding.  Every step is written so that it rounds as csrc/svr.hip does, and the GPU test asks for equal bits: the gradient update forms
t = (s_i K_i) d_alpha_i + (s_j K_j) d_alpha_j once per base row and adds +t to G[r] and -t to G[r + n] (Q_i[r + n] = -Q_i[r] exactly);
rho's sum over the free variables (`rho_tree`) is added in the kernel's fixed order -- the owner thread of rows r = tid (mod 1024) adds
them in ascending order (r, then r + n), the 64 lanes of a wave by a butterfly, the 16 waves in ascending order -- where svc_oracle.rho_rule
uses numpy's own pairwise sum; the two agree to rounding (tests/test_svr_cpu.py).

sklearn_reference measures, on the CPU, how far scikit-learn's own runs of one problem scatter: the tolerance of every comparison with it."""
import functools

import numpy as np

from svc_oracle import TAU, U53, _later_argmax, gamma_scale, kernel, rho_rule  # noqa: F401  (re-exported for the tests)

THREADS, LANES = 1024, 64


def make_data(n, d, noise, seed):
    """(X [n, d] float64, t [n]): X = randn(n, d), w = randn(d) / sqrt(d), t = X w + sin(2 X[:, 0]) + noise * randn(n), RandomState(seed)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, d)
    w = rs.randn(d) / np.sqrt(d)
    t = X @ w + np.sin(2.0 * X[:, 0]) + noise * rs.randn(n)
    return X, t


def signs(n):
    return np.concatenate([np.ones(n), -np.ones(n)])


def linear_term(t, epsilon):
    return np.concatenate([epsilon - t, epsilon + t])


def gradient(K, t, alpha, epsilon):
    """G = Q alpha + p recomputed from alpha [2n]."""
    n = len(t)
    f = K @ (alpha[:n] - alpha[n:])
    return np.concatenate([f, -f]) + linear_term(t, epsilon)


def violation(K, t, alpha, C, epsilon):
    """(m(alpha) - M(alpha), G) for any feasible alpha [2n], G recomputed from alpha."""
    s, G = signs(len(t)), gradient(K, t, alpha, epsilon)
    up = np.where(s > 0, alpha < C, alpha > 0)
    low = np.where(s > 0, alpha > 0, alpha < C)
    m = (-s * G)[up].max() if up.any() else -np.inf
    M = (-s * G)[low].min() if low.any() else np.inf
    return m - M, G


def rho_tree(s, G, alpha, C):
    """svc_oracle.rho_rule with the sum over the free variables added in csrc/svr.hip's order (module docstring)."""
    n = len(s) // 2
    free = (alpha > 0) & (alpha < C)
    if not free.any():
        return rho_rule(s, G, alpha, C)
    sG = np.where(free, s * G, 0.0)                      # adding +0.0 changes no bit of a sum that starts at +0.0
    rows = -(-n // THREADS)
    pad = np.zeros((2, rows * THREADS))
    pad[0, :n], pad[1, :n] = sG[:n], sG[n:]
    part = np.zeros(THREADS)
    for m in range(rows):
        part = part + pad[0, m * THREADS:(m + 1) * THREADS]
        part = part + pad[1, m * THREADS:(m + 1) * THREADS]
    v = part.reshape(THREADS // LANES, LANES)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    total = v[0, 0]
    for w in range(1, v.shape[0]):
        total = total + v[w, 0]
    return float(total / free.sum())


def smo(K, t, C, epsilon, tol=1e-3, max_iter=-1):
    """(alpha [2n], rho, n_iter, converged) of min 1/2 a^T Q a + p^T a, 0 <= a <= C, s^T a = 0."""
    n = len(t)
    s = signs(n)
    alpha, G, QD = np.zeros(2 * n), linear_term(np.asarray(t, dtype=np.float64), epsilon), np.diag(K).copy()
    QD2 = np.concatenate([QD, QD])
    it = 0
    while max_iter < 0 or it < max_iter:
        up = np.where(s > 0, alpha < C, alpha > 0)
        i = _later_argmax(np.where(up, -s * G, -np.inf))
        if i < 0:
            return alpha, rho_tree(s, G, alpha, C), it, True
        gmax = -s[i] * G[i]
        low = np.where(s > 0, alpha > 0, alpha < C)
        gmax2 = (s * G)[low].max() if low.any() else -np.inf
        gd = gmax + s * G
        Ki = K[i % n]
        quad = QD[i % n] + QD - 2.0 * Ki
        quad = np.where(quad > 0, quad, TAU)
        quad = np.concatenate([quad, quad])
        with np.errstate(invalid="ignore"):
            j = _later_argmax(np.where(low & (gd > 0), gd * gd / quad, -np.inf))
        if gmax + gmax2 < tol or j < 0:
            return alpha, rho_tree(s, G, alpha, C), it, True
        it += 1
        ai, aj = alpha[i], alpha[j]
        q = QD2[i] + QD2[j] - 2.0 * K[i % n, j % n]
        if not q > 0:
            q = TAU
        if s[i] != s[j]:
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > 0:
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
        else:
            delta = (G[i] - G[j]) / q
            sm = ai + aj
            ai, aj = ai - delta, aj + delta
            if sm > C:
                if ai > C:
                    ai, aj = C, sm - C
            elif aj < 0:
                aj, ai = 0.0, sm
            if sm > C:
                if aj > C:
                    aj, ai = C, sm - C
            elif ai < 0:
                ai, aj = 0.0, sm
        dai, daj = ai - alpha[i], aj - alpha[j]
        alpha[i], alpha[j] = ai, aj
        step = (s[i] * Ki) * dai + (s[j] * K[j % n]) * daj
        G[:n] += step
        G[n:] -= step
    return alpha, rho_tree(s, G, alpha, C), it, False


def fit(X, t, C, epsilon, kind, gamma=None, tol=1e-3, max_iter=-1):
    """scikit-learn's fitted attributes from the oracle: dict(support_, dual_coef_, intercept_, n_iter_, alpha, converged)."""
    K = kernel(X, X, kind, gamma)
    alpha, rho, n_iter, ok = smo(K, t, C, epsilon, tol, max_iter)
    return attributes(alpha, rho, n_iter, ok)


def attributes(alpha, rho, n_iter, ok):
    n = len(alpha) // 2
    coef = alpha[:n] - alpha[n:]
    sup = np.flatnonzero(coef != 0.0)
    return dict(support_=sup, dual_coef_=coef[sup][None, :], intercept_=np.array([-rho]), n_iter_=n_iter, alpha=alpha, converged=ok)


def predict(Xq, X, model, kind, gamma=None):
    sup = model["support_"]
    return kernel(Xq, X[sup], kind, gamma) @ model["dual_coef_"][0] + model["intercept_"][0]


@functools.lru_cache(maxsize=None)
def sklearn_reference(n, d, noise, kind, C, epsilon, tol=1e-3, train_seed=1, query_seed=2, n_query=200):
    """scikit-learn on make_data(n, d, noise, train_seed), queried on make_data(n_query, d, noise, query_seed): (the SVR fitted with
    shrinking=False on the rows in their order, its predictions, the tolerance).  Two correct SMO runs agree only to about tol, so the
    tolerance is measured from the reference itself: the rows in their order and reversed, each with shrinking on and off -- four fits --
    and the largest spread of their predictions over the queries; 4 x that spread (another solver is one more sample of the family, not a
    closer one), at least 10 tol."""
    from sklearn.svm import SVR
    X, t = make_data(n, d, noise, train_seed)
    Q, _ = make_data(n_query, d, noise, query_seed)
    fits = [SVR(kernel=kind, C=C, epsilon=epsilon, tol=tol, shrinking=sh).fit(X[::step], t[::step]) for sh in (False, True) for step in (1, -1)]
    preds = np.array([f.predict(Q) for f in fits])
    spread = float((preds.max(axis=0) - preds.min(axis=0)).max())
    return fits[0], preds[0], max(4.0 * spread, 10.0 * tol)
