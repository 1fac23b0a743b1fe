"""numpy float64 oracle for svm: seeded two-class data, direct-difference kernels, and a restatement of libsvm's C-SVC solver without
shrinking -- second-order working-set selection (Fan, Chen and Lin), libsvm's clipping, tau = 1e-12, stop at m(alpha) - M(alpha) < tol,
ties resolved as libsvm's `>=` / `<=` scans resolve them (the later index wins).  tests/test_svc_cpu.py pins it to sklearn.svm.SVC.
sklearn_reference measures, on the CPU, how far scikit-learn's own runs of one problem scatter: the tolerance of every comparison with it."""
import functools

import numpy as np

U53 = 2.0 ** -53
TAU = 1e-12


def make_data(n, d, sep, seed):
    """(X [n, d] float64, y [n] in {-1.0, +1.0}): y uniform from RandomState(seed), X = randn(n, d) + sep * y on the first three features."""
    rs = np.random.RandomState(seed)
    y = np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)
    X = rs.randn(n, d)
    X[:, :min(3, d)] += sep * y[:, None]
    return X, y


def gamma_scale(X):
    return 1.0 / (X.shape[1] * X.var())


def kernel(A, B, kind, gamma=None):
    """K[a, b] float64: "linear" = sum_k A[a, k] B[b, k]; "rbf" = exp(-gamma sum_k (A[a, k] - B[b, k])^2) by direct differences."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        if kind == "linear":
            out[i] = (B * A[i]).sum(axis=1)
        else:
            df = B - A[i]
            out[i] = np.exp(-gamma * (df * df).sum(axis=1))
    return out


def _later_argmax(v):
    """Index of the largest value, the LAST one among equals (a scan with `>=`); -1 when every value is -inf."""
    m = v.max()
    return -1 if m == -np.inf else int(len(v) - 1 - np.argmax(v[::-1]))


def violation(K, y, alpha, C):
    """(m(alpha) - M(alpha), G): the stopping quantity of the solver for any feasible alpha, G = Q alpha - 1 recomputed from alpha."""
    G = y * (K @ (alpha * y)) - 1.0
    up = np.where(y > 0, alpha < C, alpha > 0)
    low = np.where(y > 0, alpha > 0, alpha < C)
    m = (-y * G)[up].max() if up.any() else -np.inf
    M = (-y * G)[low].min() if low.any() else np.inf
    return m - M, G


def rho_rule(y, G, alpha, C):
    """libsvm's calculate_rho: the mean of y G over the free variables, else the midpoint of the bounds."""
    yG = y * G
    free = (alpha > 0) & (alpha < C)
    if free.any():
        return float(yG[free].sum() / free.sum())
    upper, lower = alpha >= C, alpha <= 0
    ub_set = (upper & (y < 0)) | (lower & (y > 0))
    lb_set = (upper & (y > 0)) | (lower & (y < 0))
    ub = yG[ub_set].min() if ub_set.any() else np.inf
    lb = yG[lb_set].max() if lb_set.any() else -np.inf
    return float((ub + lb) / 2)


def smo(K, y, C, tol=1e-3, max_iter=-1):
    """(alpha, rho, n_iter, converged) of min 1/2 a^T Q a - e^T a, 0 <= a <= C, y^T a = 0, Q = y y^T * K.  y in {-1, +1}: libsvm gives +1
    to the first class."""
    n = len(y)
    alpha, G, QD = np.zeros(n), -np.ones(n), np.diag(K).copy()
    it = 0
    while max_iter < 0 or it < max_iter:
        up = np.where(y > 0, alpha < C, alpha > 0)
        i = _later_argmax(np.where(up, -y * G, -np.inf))
        if i < 0:
            return alpha, rho_rule(y, G, alpha, C), it, True
        gmax = -y[i] * G[i]
        low = np.where(y > 0, alpha > 0, alpha < C)
        gmax2 = (y * G)[low].max() if low.any() else -np.inf
        gd = gmax + y * G
        quad = QD[i] + QD - 2.0 * K[i]
        quad = np.where(quad > 0, quad, TAU)
        j = _later_argmax(np.where(low & (gd > 0), gd * gd / quad, -np.inf))      # the smallest -gd^2 / quad, the last among equals
        if gmax + gmax2 < tol or j < 0:
            return alpha, rho_rule(y, G, alpha, C), it, True
        it += 1
        ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            q = QD[i] + QD[j] - 2.0 * K[i, j]
            delta = (-G[i] - G[j]) / (q if q > 0 else TAU)
            diff = ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > 0:                      # C_i - C_j = 0
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
        else:
            q = QD[i] + QD[j] - 2.0 * K[i, j]
            delta = (G[i] - G[j]) / (q if q > 0 else TAU)
            s = ai + aj
            ai, aj = ai - delta, aj + delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
            elif aj < 0:
                aj, ai = 0.0, s
            if s > C:
                if aj > C:
                    aj, ai = C, s - C
            elif ai < 0:
                ai, aj = 0.0, s
        dai, daj = ai - alpha[i], aj - alpha[j]
        alpha[i], alpha[j] = ai, aj
        G += y * (y[i] * K[i] * dai + y[j] * K[j] * daj)
    return alpha, rho_rule(y, G, alpha, C), it, False


def support_order(alpha, y_solver):
    """Support indices as scikit-learn orders them: the first class's (solver y = +1) ascending, then the second's."""
    sv = np.flatnonzero(alpha > 0)
    return np.concatenate([sv[y_solver[sv] > 0], sv[y_solver[sv] < 0]])


def fit(X, labels, C, kind, gamma=None, tol=1e-3, max_iter=-1):
    """scikit-learn's fitted attributes from the oracle: dict(support_, dual_coef_, intercept_, n_iter_, classes_, alpha).  The first of
    the sorted classes is the solver's +1; a positive decision value means classes_[1]."""
    classes = np.unique(labels)
    assert len(classes) == 2
    ys = np.where(labels == classes[0], 1.0, -1.0)
    K = kernel(X, X, kind, gamma)
    alpha, rho, n_iter, ok = smo(K, ys, C, tol, max_iter)
    sup = support_order(alpha, ys)
    return dict(support_=sup, dual_coef_=(-ys * alpha)[sup][None, :], intercept_=np.array([rho]), n_iter_=n_iter, classes_=classes, alpha=alpha,
                converged=ok)


def decision(Xq, X, model, kind, gamma=None):
    sup = model["support_"]
    return kernel(Xq, X[sup], kind, gamma) @ model["dual_coef_"][0] + model["intercept_"][0]


@functools.lru_cache(maxsize=None)
def sklearn_reference(n, d, sep, kind, C, tol=1e-3, train_seed=1, query_seed=2, n_query=200):
    """scikit-learn on make_data(n, d, sep, train_seed), queried on make_data(n_query, d, sep, query_seed): (the SVC fitted with
    shrinking=False on the rows in their order, its decision values, the tolerance).  Two correct SMO runs agree only to about tol, so the
    tolerance is measured from the reference itself: the rows in their order and reversed, each with shrinking on and off -- four fits --
    and the largest spread of their decision values over the queries; 4 x that spread (another solver is one more sample of the family,
    not a closer one), at least 10 tol."""
    from sklearn.svm import SVC
    X, y = make_data(n, d, sep, train_seed)
    Q, _ = make_data(n_query, d, sep, query_seed)
    fits = [SVC(C=C, kernel=kind, tol=tol, shrinking=sh).fit(X[::step], y[::step]) for sh in (False, True) for step in (1, -1)]
    decs = np.array([f.decision_function(Q) for f in fits])
    spread = float((decs.max(axis=0) - decs.min(axis=0)).max())
    return fits[0], decs[0], max(4.0 * spread, 10.0 * tol)
