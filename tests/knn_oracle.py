"""numpy-only float64 oracle for neighbors: seeded point sets, the k nearest neighbours by direct differences under the total order
(squared distance, training index), and the error bound of the centred expansion the GPU search selects with.
tests/test_knn_cpu.py pins it to sklearn.neighbors.NearestNeighbors(algorithm="brute")."""
import numpy as np

U53 = 2.0 ** -53


def make_points(n, d, seed):
    """float64 [n, d], every value exactly representable in float32: anisotropic Gaussian (column scales linspace(3, 0.3, d)) plus a
    per-column offset randn(d) that depends on (d, seed) only, so two sets drawn with different n share it."""
    offset = np.random.RandomState(1000 + seed).randn(d)
    rs = np.random.RandomState(seed * 7919 + n)
    X = rs.randn(n, d) * np.linspace(3.0, 0.3, d) + offset
    return X.astype(np.float32).astype(np.float64)


def sq_dists(Q, T):
    """s*[q, t] = sum_k (Q[q, k] - T[t, k])^2 by direct differences, float64 [m, n]."""
    Q, T = np.asarray(Q, dtype=np.float64), np.asarray(T, dtype=np.float64)
    out = np.empty((Q.shape[0], T.shape[0]))
    for i in range(Q.shape[0]):
        df = T - Q[i]
        out[i] = (df * df).sum(axis=1)
    return out


def knn(Q, T, k, exclude_self=False):
    """(dist [m, k], ind [m, k] int64, s [m, n] with the diagonal at +inf when exclude_self): neighbours by a stable sort on (s*, index)."""
    s = sq_dists(Q, T)
    if exclude_self:
        s[np.arange(s.shape[0]), np.arange(s.shape[0])] = np.inf
    ind = np.argsort(s, axis=1, kind="stable")[:, :k]
    return np.sqrt(np.take_along_axis(s, ind, axis=1)), ind.astype(np.int64), s


def bound(Q, T):
    """B[q, t] = 4 (d + 4) 2^-53 (|q - mu|^2 + |t - mu|^2), mu the training mean: the error bound of s = |q - mu|^2 + |t - mu|^2 -
    2 (q - mu).(t - mu) evaluated in float64 -- the two norms and the d-term inner product each carry the standard d u bound,
    sum |a||b| <= (|a|^2 + |b|^2) / 2, and a factor 2 of slack."""
    Q, T = np.asarray(Q, dtype=np.float64), np.asarray(T, dtype=np.float64)
    mu = T.mean(axis=0)
    qn, tn = ((Q - mu) ** 2).sum(axis=1), ((T - mu) ** 2).sum(axis=1)
    return 4.0 * (Q.shape[1] + 4) * U53 * (qn[:, None] + tn[None, :])


def min_gap_over_bound(Q, T, k, exclude_self=False):
    """Per query: the smallest (gap between consecutive squared distances) / (the larger B of the two rows), over the first k + 1
    neighbours (all of them when fewer exist).  +inf for a query with a single candidate."""
    s = sq_dists(Q, T)
    B = bound(Q, T)
    if exclude_self:
        s[np.arange(s.shape[0]), np.arange(s.shape[0])] = np.inf
    order = np.argsort(s, axis=1, kind="stable")
    avail = s.shape[1] - (1 if exclude_self else 0)
    take = min(k + 1, avail)
    so = np.take_along_axis(s, order[:, :take], axis=1)
    Bo = np.take_along_axis(B, order[:, :take], axis=1)
    if take < 2:
        return np.full(s.shape[0], np.inf)
    return ((so[:, 1:] - so[:, :-1]) / np.maximum(Bo[:, 1:], Bo[:, :-1])).min(axis=1)
