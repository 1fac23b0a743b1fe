"""numpy-only oracle for decomposition.PCA: the seeded low-rank-plus-noise test matrices and the exact (centred SVD) PCA with
scikit-learn 1.7's sign rule.  tests/test_pca_cpu.py pins it to sklearn.decomposition.PCA(svd_solver="full")."""
from types import SimpleNamespace

import numpy as np

# (n, d, r, k) of the fit tests; seed 1
SHAPES = [(37, 203, 12, 8), (150, 19, 19, 10), (61, 4099, 20, 16), (130, 49152, 40, 32), (300, 167, 80, 64)]


def make_matrix(n, d, r, seed, ratio=0.9):
    """float32 [n, d]: U diag(10 ratio^j sqrt(n)) V^T with orthonormal U [n, r], V [d, r], plus 1e-3 randn noise, plus a per-column
    offset 3 randn(d)."""
    rs = np.random.RandomState(seed)
    U = np.linalg.qr(rs.randn(n, r))[0]
    V = np.linalg.qr(rs.randn(d, r))[0]
    s = 10.0 * ratio ** np.arange(r) * np.sqrt(n)
    X = (U * s) @ V.T + 1e-3 * rs.randn(n, d) + 3.0 * rs.randn(d)
    return X.astype(np.float32)


def pca_full(X64, k):
    """Exact PCA of a float64 [n, d] matrix through the SVD of the centred matrix.  Signs: in every component the entry of largest
    magnitude is positive, first index on ties (svd_flip(u_based_decision=False))."""
    X64 = np.asarray(X64, dtype=np.float64)
    n, d = X64.shape
    mean = X64.mean(axis=0)
    _, S, Vt = np.linalg.svd(X64 - mean, full_matrices=False)
    signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    signs[signs == 0] = 1.0
    Vt = Vt * signs[:, None]
    ev = S ** 2 / (n - 1)
    return SimpleNamespace(mean_=mean, components_=Vt[:k].copy(), singular_values_=S[:k].copy(), explained_variance_=ev[:k].copy(),
                           explained_variance_ratio_=ev[:k] / ev.sum(), noise_variance_=float(ev[k:].mean()) if k < min(n, d) else 0.0,
                           n_components_=k, n_samples_=n, n_features_in_=d)


def transform(o, X):
    """(X - mean) C^T in float64."""
    return (np.asarray(X, dtype=np.float64) - o.mean_) @ o.components_.T
