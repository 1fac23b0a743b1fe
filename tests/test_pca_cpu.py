"""CPU: the PCA oracle is pinned to scikit-learn's exact solver; the float64 product's workspace query and decomposition.PCA's
argument handling work without a GPU."""
import ctypes

import numpy as np
import pytest

from bbbp_amd import _lib
from pca_oracle import SHAPES, make_matrix, pca_full, transform


@pytest.mark.parametrize("n,d,r,k", SHAPES)
def test_oracle_equals_sklearn_full(n, d, r, k):
    """This test fixes the sign convention: sklearn 1.7's svd_flip(u_based_decision=False)."""
    from sklearn.decomposition import PCA as SkPCA
    X = make_matrix(n, d, r, 1).astype(np.float64)
    sk = SkPCA(k, svd_solver="full").fit(X)
    o = pca_full(X, k)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()  # noqa: E731
    assert rel(o.components_, sk.components_) <= 1e-12
    assert rel(o.singular_values_, sk.singular_values_) <= 1e-12
    assert rel(o.explained_variance_, sk.explained_variance_) <= 1e-12
    assert rel(o.explained_variance_ratio_, sk.explained_variance_ratio_) <= 1e-12
    assert abs(o.noise_variance_ - sk.noise_variance_) <= 1e-12 * sk.noise_variance_
    assert rel(o.mean_, sk.mean_) <= 1e-12
    assert rel(transform(o, X), sk.transform(X)) <= 1e-12


def _desc(**kw):
    base = dict(layout=0, M=64, N=64, K=64, a_dtype=0, b_dtype=0, c_dtype=1, symmetric=0, split_k=0)
    base.update(kw)
    return _lib.GemmF64cDesc(**base)


def test_gemm_f64c_workspace_bytes_without_gpu():
    L = _lib.lib()
    gram = _desc(M=1058, N=1058, K=49152, symmetric=1)                 # the image Gram matrix: split over K, slabs in the workspace
    ws = L.bbbp_gemm_f64c_workspace_bytes(ctypes.byref(gram))
    assert ws > 0 and ws % (1058 * 1058 * 8) == 0
    forced = _desc(M=130, N=17, K=5, split_k=7)
    assert L.bbbp_gemm_f64c_workspace_bytes(ctypes.byref(forced)) == 7 * 130 * 17 * 8
    assert L.bbbp_gemm_f64c_workspace_bytes(ctypes.byref(_desc(M=130, N=17, K=5, split_k=1))) == 0
    assert L.bbbp_gemm_f64c_workspace_bytes(ctypes.byref(_desc(M=64, N=65, symmetric=1))) == 0
    assert b"symmetric" in L.bbbp_last_error()
    assert L.bbbp_gemm_f64c_workspace_bytes(ctypes.byref(_desc(a_dtype=2))) == 0
    assert b"dtype" in L.bbbp_last_error()
    assert L.bbbp_gemm_f64c_workspace_bytes(ctypes.byref(_desc(layout=2))) == 0
    assert b"layout" in L.bbbp_last_error()
    # the launcher validates before it touches the GPU
    assert L.bbbp_gemm_f64c(None, ctypes.byref(_desc(M=64, N=65, symmetric=1)), None, 0) == 1
    assert L.bbbp_pca_col_mean(None, None, 0, 4, 4, 4, None) == 1
    assert L.bbbp_pca_col_mean(None, ctypes.c_void_p(4096), 3, 4, 4, 4, ctypes.c_void_p(4096)) == 1


def test_pca_argument_handling():
    from bbbp_amd.decomposition import PCA
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PCA(8, device="cpu")
    with pytest.raises(ValueError, match="whiten"):
        PCA(8, whiten=True)
    for bad in (0.95, 8.0, "mle", True):
        with pytest.raises(ValueError, match="n_components"):
            PCA(bad)
    p = PCA(np.int64(8))
    assert p.n_components == 8 and PCA().n_components is None
    with pytest.raises(ValueError):
        PCA.from_arrays(np.zeros(5), np.zeros((2, 4)))
