"""``sklearn.decomposition.PCA`` for the GPU: the stage between ``preprocess`` and the PCA-fusion models / the MLP grid.

The reference reduces its inputs before the fusion network sees them
(``Models/multi_input_data_regression_opt_transformer_cnn_opt.py:30-33``: fingerprints [N,167] -> 64, images [N,49152] -> 128;
``Models/model_opt_maccs.py:104-109``: StandardScaler, then ``PCA(100)`` in front of the ``MLPClassifier`` grid).  ``PCA`` here computes
the exact decomposition ``svd_solver="full"`` computes, deterministically, in float64:

* column means, the covariance (d <= n) or Gram (n < d) matrix, the components of the Gram regime and ``transform`` are launches of
  ``csrc/pca.hip`` (float64 MFMA, centring fused into the operand staging, fixed summation order);
* the dense eigen-solve of the ``min(n, d)^2`` matrix is ``numpy.linalg.eigh`` on the host -- the split ``ensemble.py`` makes for its
  meta-learner: the O(min^2 max) products are GPU work, the O(min^3) solve is LAPACK's.

The reference's ``svd_solver="auto"`` picks the unseeded randomized solver for both of its shapes, an approximation of this result.

Out of scope: ``inverse_transform`` (a third operand layout), whitening, randomized / incremental / sparse solvers, and
``min(n, d) > 8192`` (the host solve).  There is no CPU path.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _dense, _lib

MAX_SOLVE = 8192           # largest min(n, d) handed to the host eigen-solver
_NT, _TN = 0, 1


def _gemm_f64c(layout, M, N, K, A, lda, B, ldb, out, a_shift=None, b_shift=None, row_scale=None, symmetric=False, split_k=0):
    """One ``bbbp_gemm_f64c`` launch on the current stream; ``out`` [M, N] contiguous float32 / float64."""
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    d = _lib.GemmF64cDesc(layout, M, N, K, A.data_ptr(), _dense.DT[A.dtype], lda, B.data_ptr(), _dense.DT[B.dtype], ldb,
                          p(a_shift), p(b_shift), p(row_scale), out.data_ptr(), _dense.DT[out.dtype], N, int(symmetric), int(split_k))
    L = _lib.lib()
    _dense.launch_with_workspace(L.bbbp_gemm_f64c_workspace_bytes, L.bbbp_gemm_f64c, d, out.device, "bbbp_gemm_f64c")
    return out


def gemm_f64c(A, B, *, layout="NT", a_shift=None, b_shift=None, row_scale=None, symmetric=False, out_dtype=torch.float64, split_k=0):
    """``C[M,N] = row_scale[m] * sum_k (A(m,k) - sa)(B(n,k) - sb)`` with float64 accumulation (``bbbp_gemm_f64c``).

    ``layout="NT"``: A [M,K], B [N,K]; ``"TN"``: A [K,M], B [K,N]; CUDA tensors, float32 or float64 each, unit inner stride.  The shifts
    are float64 vectors over k (NT) or over the operand's own row / column index (TN).  ``symmetric`` needs ``B is A``."""
    if layout not in ("NT", "TN"):
        raise ValueError(f"layout must be 'NT' or 'TN', got {layout!r}")
    for name, t in (("A", A), ("B", B)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"gemm_f64c: {name} must be a CUDA (HIP) tensor; there is no CPU fallback")
        if t.dtype not in _dense.DT or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise RuntimeError(f"gemm_f64c: {name} must be a 2-D float32 / float64 tensor with unit inner stride")
    if layout == "NT":
        (M, K), (N, Kb) = A.shape, B.shape
    else:
        (K, M), (Kb, N) = A.shape, B.shape
    if K != Kb:
        raise ValueError(f"gemm_f64c: reduction lengths differ ({K} and {Kb})")
    for name, v, want in (("a_shift", a_shift, K if layout == "NT" else M), ("b_shift", b_shift, K if layout == "NT" else N),
                          ("row_scale", row_scale, M)):
        if v is not None and not (v.is_cuda and v.dtype == torch.float64 and v.is_contiguous() and v.numel() == want):
            raise RuntimeError(f"gemm_f64c: {name} must be a contiguous CUDA float64 vector of length {want}")
    out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    with torch.cuda.device(A.device):
        return _gemm_f64c(_NT if layout == "NT" else _TN, M, N, K, A, _dense.ld(A), B, _dense.ld(B), out, a_shift, b_shift, row_scale, symmetric, split_k)


class PCA:
    """``PCA(n_components=None, *, whiten=False, device="cuda")``: scikit-learn's names, the exact (``svd_solver="full"``) result.

    ``fit`` / ``fit_transform`` / ``transform`` take CUDA tensors or numpy arrays, float32 or float64, [n, d]; non-contiguous input is
    copied.  ``transform`` returns what it was given: a CUDA tensor for a tensor, a numpy array for an array, in the input's dtype
    (float64 accumulation, rounded once).  ``mean_``, ``components_``, ``explained_variance_``, ``explained_variance_ratio_`` and
    ``singular_values_`` are float64 numpy arrays; ``noise_variance_``, ``n_components_``, ``n_samples_``, ``n_features_in_`` scalars.
    Component signs follow scikit-learn 1.7 (``svd_flip(u_based_decision=False)``): the entry of largest magnitude of every component is
    positive, first index on ties.

    Not provided: ``inverse_transform``, whitening, randomized / incremental / sparse solvers, ``min(n, d) > 8192``."""

    def __init__(self, n_components=None, *, whiten=False, device="cuda"):
        if whiten:
            raise ValueError("PCA: whiten=True is not supported")
        if n_components is not None and (isinstance(n_components, bool) or not isinstance(n_components, numbers.Integral)):
            raise ValueError(f"PCA: n_components must be an int or None (floats and 'mle' are not supported), got {n_components!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PCA: device {device!r}: the products run on the GPU (no CPU fallback)")
        self.n_components = None if n_components is None else int(n_components)
        self.whiten = False

    # ---- construction from existing results -------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, mean, components, *, explained_variance=None, explained_variance_ratio=None, singular_values=None,
                    noise_variance=None, n_samples=None, device="cuda"):
        """A fitted PCA from ``mean`` [d] and ``components`` [k, d] (any float arrays): ``transform`` then runs on the GPU."""
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        components = np.ascontiguousarray(components, dtype=np.float64)
        if components.ndim != 2 or mean.shape != (components.shape[1],) or components.shape[0] < 1:
            raise ValueError(f"PCA.from_arrays: mean {mean.shape} and components {components.shape} do not fit together")
        if not (np.isfinite(mean).all() and np.isfinite(components).all()):
            raise ValueError("PCA.from_arrays: non-finite mean or components")
        self = cls(components.shape[0], device=device)
        self.mean_, self.components_ = mean, components
        k = components.shape[0]
        for name, v in (("explained_variance_", explained_variance), ("explained_variance_ratio_", explained_variance_ratio),
                        ("singular_values_", singular_values)):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.float64)
                if v.shape != (k,):
                    raise ValueError(f"PCA.from_arrays: {name} has shape {v.shape}, expected ({k},)")
                setattr(self, name, v)
        if noise_variance is not None:
            self.noise_variance_ = float(noise_variance)
        if n_samples is not None:
            self.n_samples_ = int(n_samples)
        self.n_components_, self.n_features_in_ = k, components.shape[1]
        self._mean_d = torch.from_numpy(mean).to(self.device)
        self._comp_d = torch.from_numpy(components).to(self.device)
        return self

    @classmethod
    def from_sklearn(cls, fitted_pca, device="cuda"):
        """A fitted ``sklearn.decomposition.PCA`` (any solver), to be applied on the GPU."""
        if getattr(fitted_pca, "whiten", False):
            raise ValueError("PCA.from_sklearn: whiten=True is not supported")
        if not hasattr(fitted_pca, "components_"):
            raise ValueError("PCA.from_sklearn: the estimator is not fitted")
        mean = fitted_pca.mean_ if fitted_pca.mean_ is not None else np.zeros(fitted_pca.components_.shape[1])
        return cls.from_arrays(mean, fitted_pca.components_, explained_variance=fitted_pca.explained_variance_,
                               explained_variance_ratio=fitted_pca.explained_variance_ratio_, singular_values=fitted_pca.singular_values_,
                               noise_variance=getattr(fitted_pca, "noise_variance_", None), n_samples=getattr(fitted_pca, "n_samples_", None),
                               device=device)

    # ---- input handling ---------------------------------------------------------------------------------------------
    def _to_device(self, X):
        """(device tensor [n, d] float32 / float64 with unit inner stride and dense rows, was_numpy)"""
        return _dense.to_device_matrix(X, self.device, "PCA", allow_row_stride=False)

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X):
        self._fit(self._to_device(X)[0])
        return self

    def fit_transform(self, X):
        Xd, was_numpy = self._to_device(X)
        self._fit(Xd)
        return self._transform(Xd, was_numpy)

    def _fit(self, X):
        n, d = X.shape
        small = min(n, d)
        if n < 2:
            raise ValueError(f"PCA: at least 2 samples are needed, got {n}")
        k = small if self.n_components is None else self.n_components
        if not 1 <= k <= small:
            raise ValueError(f"PCA: n_components={k} must be between 1 and min(n_samples, n_features)={small}")
        if small > MAX_SOLVE:
            raise ValueError(f"PCA: min(n_samples, n_features)={small} exceeds {MAX_SOLVE}: the {small} x {small} eigen-solve runs on the "
                             "host and is not offered beyond that size")
        L = _lib.lib()
        with torch.cuda.device(self.device):
            mean_d = torch.empty(d, dtype=torch.float64, device=self.device)
            _lib.check(L.bbbp_pca_col_mean(_dense.stream(), X.data_ptr(), _dense.DT[X.dtype], n, d, d, mean_d.data_ptr()),
                       "bbbp_pca_col_mean")
            mean = mean_d.cpu().numpy()
            if not np.isfinite(mean).all():
                raise ValueError("PCA: the input contains NaN or infinity")
            S = torch.empty((small, small), dtype=torch.float64, device=self.device)
            if d <= n:      # covariance regime: Xc^T Xc [d, d]
                _gemm_f64c(_TN, d, d, n, X, d, X, d, S, mean_d, mean_d, symmetric=True)
            else:           # Gram regime: Xc Xc^T [n, n]
                _gemm_f64c(_NT, n, n, d, X, d, X, d, S, mean_d, mean_d, symmetric=True)
            S_host = S.cpu().numpy()
            lam_all, vec = np.linalg.eigh(S_host)
            lam_all, vec = lam_all[::-1], vec[:, ::-1]          # descending
            lam = lam_all[:k]
            sigma = np.sqrt(np.maximum(lam, 0.0))
            if d <= n:
                comp_d = torch.from_numpy(np.ascontiguousarray(vec[:, :k].T)).to(self.device)
            else:
                thresh = max(n, d) * 2.0 ** -52 * lam_all[0]
                if not lam[-1] > thresh:
                    rank = int(np.count_nonzero(lam_all > thresh))
                    raise ValueError(f"PCA: n_components={k} exceeds the numerical rank {rank} of the centred [{n}, {d}] input: with "
                                     "n_samples < n_features a direction of (near-)zero variance cannot be recovered from the Gram matrix")
                U = torch.from_numpy(np.ascontiguousarray(vec[:, :k])).to(self.device)            # [n, k]
                inv_sigma = torch.from_numpy(1.0 / sigma).to(self.device)
                comp_d = torch.empty((k, d), dtype=torch.float64, device=self.device)
                _gemm_f64c(_TN, k, d, n, U, k, X, d, comp_d, None, mean_d, row_scale=inv_sigma)    # diag(1/sigma) U^T Xc
            comp = comp_d.cpu().numpy()
            signs = np.sign(comp[np.arange(k), np.argmax(np.abs(comp), axis=1)])
            signs[signs == 0] = 1.0
            comp = comp * signs[:, None]
            comp_d.mul_(torch.from_numpy(signs).to(self.device)[:, None])
        ev_all = np.maximum(lam_all, 0.0) / (n - 1)
        self.mean_, self._mean_d = mean, mean_d
        self.components_, self._comp_d = comp, comp_d
        self.singular_values_ = sigma
        self.explained_variance_ = lam / (n - 1)
        self.explained_variance_ratio_ = self.explained_variance_ / (np.trace(S_host) / (n - 1))
        self.noise_variance_ = float(ev_all[k:].mean()) if k < small else 0.0
        self.n_components_, self.n_samples_, self.n_features_in_ = k, n, d

    # ---- transform --------------------------------------------------------------------------------------------------
    def transform(self, X):
        return self._transform(*self._to_device(X))

    def _transform(self, X, was_numpy):
        if not hasattr(self, "_comp_d"):
            raise RuntimeError("PCA: not fitted")
        m, d = X.shape
        k = self.n_components_
        if d != self.n_features_in_:
            raise ValueError(f"PCA: the input has {d} features, the fit saw {self.n_features_in_}")
        out = torch.empty((m, k), dtype=X.dtype, device=self.device)
        if m:
            with torch.cuda.device(self.device):
                _gemm_f64c(_NT, m, k, d, X, d, self._comp_d, d, out, self._mean_d, None)         # (X - mean) C^T, one product
        return out.cpu().numpy() if was_numpy else out
