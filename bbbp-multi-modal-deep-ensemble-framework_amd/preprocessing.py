"""``sklearn.preprocessing.StandardScaler`` and ``PolynomialFeatures`` for the GPU: the two steps that feed every other estimator here.

The classification scripts of the reference begin ``StandardScaler().fit_transform(X)`` -> ``PCA`` -> ``SMOTE`` -> learners
(``Models/model_opt_maccs.py:104-113``); the regression feature scripts run ``StandardScaler`` -> ``PCA(30)`` twice ->
``PolynomialFeatures(degree=2, interaction_only=True, include_bias=False)`` on the 60 joined components -> ``IsolationForest``
(``Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest_fixed_1.py:105-134``).  With these two the matrix stays on the
device from the raw table to the fitted stack.  (``preprocess.standardize_features`` is the float32, fused uint8 + image, chunked special
case of one script, without fitted state; it is a different thing and stays as it is.)

Both estimators work in float64 and carry scikit-learn 1.7's names.

* ``StandardScaler``: ``bbbp_scaler_moments`` (``csrc/scaler.hip``) is scikit-learn's ``_incremental_mean_and_var`` followed by
  ``_is_constant_feature`` with every operation rounded on its own, one launch per ``fit`` / ``partial_fit``; ``bbbp_scaler_apply`` is
  ``(x - mean) / scale`` and ``x * scale + mean``, two roundings each.  On C-contiguous float64 input with at least two columns ``mean_``,
  ``var_``, ``scale_``, ``transform`` and ``inverse_transform`` equal scikit-learn 1.7.2 / numpy 2.2 bit for bit
  (``tests/preprocessing_numpy.py`` restates the arithmetic, ``tests/test_preprocessing_cpu.py`` pins the restatement to scikit-learn).
  A column is constant when ``var <= (N eps) var + ((N mean) eps)^2``; there is no ``scale < 10 eps`` rule, which scikit-learn applies
  only where no such mask is passed.
* ``PolynomialFeatures``: the host builds the table of factor indices in ``fit`` ([P, 3] int32, scikit-learn's column order) and
  ``bbbp_poly_expand`` (``csrc/poly.hip``) writes every column as one chain of float64 products, ``(x_k x_j) x_i`` for the column
  ``(i, j, k)``, ``i <= j <= k``: bit for bit scikit-learn's dense result for degrees 1 to 3.

Input, both classes: a CUDA tensor or a numpy array, [n, d].  float64 is taken as is; integers, uint8 and bool are converted to float64
exactly, as ``check_array`` converts them.  A row-major tensor with a padded leading dimension (``stride(1) == 1``, ``stride(0) >= d``) is
read in place at any 8-byte aligned base; every other layout is copied to contiguous rows.  A tensor in gives a CUDA float64 tensor out, an
array in an array out; the result is always a new array.

Known deviations from scikit-learn:

1. Column-major input.  numpy sums a column-major matrix pairwise along its columns; here it is copied to row-major and summed in row
   order, so the last bits of ``mean_`` / ``var_`` may differ.
2. A single column (``d == 1``).  numpy treats it as a contiguous vector and sums it pairwise; here it is summed in row order.  Up to 18
   ulp between the two were measured on the CPU at n <= 7807.

Refused by name: float32 and float16 input (scikit-learn would keep float32; that path is not built -- pass ``X.double()``), NaN or
infinity in ``X`` (scikit-learn's scaler skips NaN; not built), ``sample_weight``, sparse input, ``copy=False`` (in-place operation),
``n`` or ``d`` above ``2**31 - 1``; for ``PolynomialFeatures`` also a ``(min_degree, max_degree)`` tuple, a degree outside 1..3,
``order="F"``, more than ``2**31 - 1`` output columns, and an output that ``torch.empty`` cannot serve.  There is no CPU path.
"""
from __future__ import annotations

import itertools
import numbers

import numpy as np
import torch

from . import _dense, _lib
from ._estimator import Params

INT_MAX = 2 ** 31 - 1
_LAUNCHES = {"moments": 0, "apply": 0, "expand": 0}        # library entry points per kind (tools/bench_preprocessing.py reads the differences)


def _device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: device {str(device)!r}: the kernels run on the GPU (no CPU fallback)")
    return device


def _refuse_float(dtype, who):
    raise TypeError(f"{who}: {dtype} input is not supported (scikit-learn would keep float32; that path is not built): pass X.double() "
                    "for a tensor, X.astype(numpy.float64) for an array")


def _checked(X, who):
    """(tensor [n, d] where it was given, was_numpy) after every check that needs no device."""
    if hasattr(X, "tocsr") or (isinstance(X, torch.Tensor) and X.layout != torch.strided):
        raise TypeError(f"{who}: sparse input is not supported")
    was_numpy = not isinstance(X, torch.Tensor)
    if was_numpy:
        X = np.asarray(X)
        if X.dtype.kind == "f" and X.dtype != np.float64:
            _refuse_float(X.dtype, who)
        if X.dtype.kind not in "fiub":
            raise TypeError(f"{who}: expected a numeric [n, d] input, got dtype {X.dtype}")
        if X.ndim != 2:
            raise ValueError(f"{who}: expected a 2-D [n, d] input, got shape {tuple(X.shape)}")
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))
    else:
        if not X.is_cuda:
            raise RuntimeError(f"{who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU fallback)")
        if X.dtype in (torch.float32, torch.float16, torch.bfloat16):
            _refuse_float(X.dtype, who)
        if X.dtype.is_complex or (X.dtype.is_floating_point and X.dtype != torch.float64):
            raise TypeError(f"{who}: expected a numeric [n, d] input, got dtype {X.dtype}")
        if X.dim() != 2:
            raise ValueError(f"{who}: expected a 2-D [n, d] input, got shape {tuple(X.shape)}")
    n, d = X.shape
    if n < 1 or d < 1:
        raise ValueError(f"{who}: needs at least one row and one feature, got shape {(n, d)}")
    if n > INT_MAX or d > INT_MAX:
        raise ValueError(f"{who}: n = {n} and d = {d} must not exceed 2**31 - 1")
    return X, was_numpy


def _moved(X, device):
    """Device tensor [n, d] float64 with unit inner stride at an 8-byte aligned base: in place where the layout allows, else a copy."""
    n, d = X.shape
    X = X.to(device=device, dtype=torch.float64)
    in_place = (d == 1 or X.stride(1) == 1) and (n == 1 or X.stride(0) >= d) and X.data_ptr() % 8 == 0
    return X if in_place else X.contiguous()


def _to_device(X, device, who):
    X, was_numpy = _checked(X, who)
    return _moved(X, device), was_numpy


def _ptr(t):
    return None if t is None else t.data_ptr()


def _raise_if_flagged(flag_word, who):
    if int(flag_word) != 0:
        raise ValueError(f"{who}: the input contains NaN or infinity")


def _give_back(out, was_numpy):
    return out.cpu().numpy() if was_numpy else out


def _refuse_copy(copy, who):
    if copy is not None and not copy:
        raise ValueError(f"{who}: copy=False (in-place operation) is not supported: the result is always a new array")


class StandardScaler(Params):
    """``StandardScaler(*, with_mean=True, with_std=True, device="cuda")``: ``fit``, ``partial_fit``, ``transform``, ``fit_transform``,
    ``inverse_transform`` with scikit-learn 1.7's arithmetic in float64 (see the module's text for what is exact and what deviates).

    ``mean_``, ``var_`` and ``scale_`` are float64 numpy arrays, ``n_samples_seen_`` and ``n_features_in_`` ints.  With ``with_std=False``
    ``var_`` and ``scale_`` are ``None``; with both flags off ``mean_`` is ``None`` as well (the input is still checked and counted).
    ``from_sklearn`` / ``from_arrays`` adopt a scaler fitted elsewhere, so that it transforms on the GPU.

    Refused by name: float32 / float16 input (pass ``X.double()``), NaN or infinity, ``sample_weight``, sparse input, ``copy=False``."""

    _params = ("with_mean", "with_std", "device")
    _who = "StandardScaler"

    def __init__(self, *, with_mean=True, with_std=True, device="cuda"):
        for name, v in (("with_mean", with_mean), ("with_std", with_std)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"StandardScaler: {name} must be a bool, got {v!r}")
        self.device = _device(device, self._who)
        self.with_mean, self.with_std = bool(with_mean), bool(with_std)

    # ---- construction from existing results -------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, mean, scale, *, var=None, n_samples_seen=None, with_mean=None, with_std=None, n_features=None, device="cuda"):
        """A fitted scaler from ``mean`` [d] and ``scale`` [d] (any float arrays): ``transform`` and ``inverse_transform`` then run on the
        GPU.  ``with_mean`` / ``with_std`` default to whether the array is given.  ``var`` and ``n_samples_seen`` let ``partial_fit``
        continue the series; ``n_features`` is needed only when no array is given."""
        arrays = {}
        for name, v in (("mean", mean), ("scale", scale), ("var", var)):
            if v is not None:
                v = np.array(v, dtype=np.float64, ndmin=1)
                if v.ndim != 1 or v.size < 1 or not np.isfinite(v).all():
                    raise ValueError(f"StandardScaler.from_arrays: {name} must be a finite vector, got shape {v.shape}")
                arrays[name] = v
        sizes = {v.size for v in arrays.values()} | ({int(n_features)} if n_features is not None else set())
        if len(sizes) != 1:
            raise ValueError(f"StandardScaler.from_arrays: mean, scale, var and n_features must agree on one length, got {sorted(sizes)}")
        if "scale" in arrays and (arrays["scale"] == 0).any():
            raise ValueError("StandardScaler.from_arrays: a scale of 0 (scikit-learn stores 1.0 for a constant column)")
        self = cls(with_mean=mean is not None if with_mean is None else with_mean, with_std=scale is not None if with_std is None else with_std,
                   device=device)
        if self.with_mean and "mean" not in arrays or self.with_std and "scale" not in arrays:
            raise ValueError("StandardScaler.from_arrays: with_mean needs mean, with_std needs scale")
        self.mean_, self.scale_, self.var_ = arrays.get("mean"), arrays.get("scale"), arrays.get("var")
        self.n_features_in_ = sizes.pop()
        if n_samples_seen is not None:
            self.n_samples_seen_ = int(n_samples_seen)
        self._upload()
        return self

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """A fitted ``sklearn.preprocessing.StandardScaler``, to be applied on the GPU."""
        if not hasattr(fitted, "n_samples_seen_"):
            raise ValueError("StandardScaler.from_sklearn: the estimator is not fitted")
        if np.ndim(fitted.n_samples_seen_) != 0:
            raise ValueError("StandardScaler.from_sklearn: fitted on data with NaN (a sample count per column): not supported")
        return cls.from_arrays(fitted.mean_, fitted.scale_, var=fitted.var_, n_samples_seen=fitted.n_samples_seen_, with_mean=bool(fitted.with_mean),
                               with_std=bool(fitted.with_std), n_features=fitted.n_features_in_, device=device)

    def _upload(self):
        up = lambda v: None if v is None else torch.from_numpy(v).to(self.device)  # noqa: E731
        self._mean_d, self._var_d, self._scale_d = up(self.mean_), up(self.var_), up(self.scale_)

    # ---- fit ----------------------------------------------------------------------------------------------------------
    def _reset(self):
        for name in ("mean_", "var_", "scale_", "n_samples_seen_", "n_features_in_", "_mean_d", "_var_d", "_scale_d"):
            if hasattr(self, name):
                delattr(self, name)

    def fit(self, X, y=None, sample_weight=None):
        self._reset()
        return self.partial_fit(X, y, sample_weight)

    def partial_fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("StandardScaler: sample_weight is not supported")
        self._partial_fit(_to_device(X, self.device, self._who)[0])
        return self

    def _partial_fit(self, X):
        n, d = X.shape
        last_n = int(getattr(self, "n_samples_seen_", 0))
        if hasattr(self, "n_features_in_") and d != self.n_features_in_:
            raise ValueError(f"StandardScaler: the input has {d} features, the earlier batches had {self.n_features_in_}")
        if hasattr(self, "n_features_in_") and not last_n:
            raise RuntimeError("StandardScaler: adopted without n_samples_seen: partial_fit cannot continue the series (fit starts anew)")
        last_mean, last_var = (getattr(self, "_mean_d", None), getattr(self, "_var_d", None)) if last_n else (None, None)
        if last_n and (self.with_mean or self.with_std) and (last_mean is None or (self.with_std and last_var is None)):
            raise RuntimeError("StandardScaler: adopted without mean or var: partial_fit cannot continue the series (fit starts anew)")
        last_n_kernel = last_n if last_mean is not None else 0            # both flags off: only the count continues
        with torch.cuda.device(self.device):
            res = torch.empty(3 * d + 1, dtype=torch.float64, device=self.device)            # mean | var | scale | flag word
            mean_d, var_d, scale_d, flag = res[:d], res[d:2 * d], res[2 * d:3 * d], res[3 * d:]
            _LAUNCHES["moments"] += 1
            _lib.check(_lib.lib().bbbp_scaler_moments(_dense.stream(), X.data_ptr(), _dense.ld(X), n, d, _ptr(last_mean), _ptr(last_var), last_n_kernel,
                                                      mean_d.data_ptr(), var_d.data_ptr(), scale_d.data_ptr(), flag.data_ptr()), "bbbp_scaler_moments")
            host = res.cpu().numpy()                         # one read: the three vectors and the flag
        _raise_if_flagged(host[3 * d:].view(np.int32)[0], self._who)
        self.n_samples_seen_, self.n_features_in_ = last_n + n, d
        if not (self.with_mean or self.with_std):
            self.mean_ = self.var_ = self.scale_ = None
            self._mean_d = self._var_d = self._scale_d = None
            return
        self.mean_, self._mean_d = host[:d].copy(), mean_d
        if self.with_std:
            self.var_, self.scale_ = host[d:2 * d].copy(), host[2 * d:3 * d].copy()
            self._var_d, self._scale_d = var_d, scale_d
        else:
            self.var_ = self.scale_ = self._var_d = self._scale_d = None

    # ---- transform ----------------------------------------------------------------------------------------------------
    def _apply(self, X, was_numpy, inverse, check):
        if not hasattr(self, "n_features_in_"):
            raise RuntimeError("StandardScaler: not fitted")
        n, d = X.shape
        if d != self.n_features_in_:
            raise ValueError(f"StandardScaler: the input has {d} features, the fit saw {self.n_features_in_}")
        mean = self._mean_d if self.with_mean else None
        scale = self._scale_d if self.with_std else None
        with torch.cuda.device(self.device):
            out = torch.empty((n, d), dtype=torch.float64, device=self.device)
            flag = torch.empty(1, dtype=torch.int32, device=self.device) if check else None
            _LAUNCHES["apply"] += 1
            _lib.check(_lib.lib().bbbp_scaler_apply(_dense.stream(), X.data_ptr(), _dense.ld(X), n, d, _ptr(mean), _ptr(scale), int(inverse),
                                                    out.data_ptr(), d, _ptr(flag)), "bbbp_scaler_apply")
            if check:
                _raise_if_flagged(flag.cpu()[0], self._who)
        return _give_back(out, was_numpy)

    def fit_transform(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("StandardScaler: sample_weight is not supported")
        Xd, was_numpy = _to_device(X, self.device, self._who)
        self._reset()
        self._partial_fit(Xd)
        return self._apply(Xd, was_numpy, False, check=False)            # the fit has checked these rows

    def transform(self, X, copy=None):
        _refuse_copy(copy, self._who)
        return self._apply(*_to_device(X, self.device, self._who), False, check=True)

    def inverse_transform(self, X, copy=None):
        _refuse_copy(copy, self._who)
        return self._apply(*_to_device(X, self.device, self._who), True, check=True)


def _combinations(d, degree, interaction_only, include_bias):
    """scikit-learn's ``_combinations``: the index tuples of the output columns, lazily."""
    comb = itertools.combinations if interaction_only else itertools.combinations_with_replacement
    return itertools.chain.from_iterable(comb(range(d), k) for k in range(0 if include_bias else 1, degree + 1))


def _n_output_features(d, degree, interaction_only, include_bias):
    """The number of output columns, in exact integers."""
    from math import comb
    if interaction_only:
        total = sum(comb(d, k) for k in range(1, min(degree, d) + 1))
    else:
        total = comb(d + degree, degree) - 1
    return total + int(include_bias)


class PolynomialFeatures(Params):
    """``PolynomialFeatures(degree=2, *, interaction_only=False, include_bias=True, device="cuda")``: ``fit``, ``transform``,
    ``fit_transform``; ``n_features_in_``, ``n_output_features_`` and ``powers_`` (int64 numpy array) as scikit-learn sets them, the columns
    in its order.  A column is one chain of float64 products, rounded one by one: ``x_k x_j`` for ``(j, k)``, ``(x_k x_j) x_i`` for
    ``(i, j, k)``, 1.0 for the bias; bit for bit scikit-learn 1.7's dense result.

    Refused by name: a ``(min_degree, max_degree)`` tuple, a degree outside 1..3, ``order="F"``, sparse input, float32 / float16 input (pass
    ``X.double()``), NaN or infinity, more than ``2**31 - 1`` output columns, an output matrix that ``torch.empty`` cannot serve."""

    _params = ("degree", "interaction_only", "include_bias", "order", "device")
    _who = "PolynomialFeatures"

    def __init__(self, degree=2, *, interaction_only=False, include_bias=True, order="C", device="cuda"):
        if isinstance(degree, (tuple, list)):
            raise ValueError(f"PolynomialFeatures: a (min_degree, max_degree) tuple is not supported, got degree={degree!r}")
        if isinstance(degree, bool) or not isinstance(degree, numbers.Integral) or not 1 <= degree <= 3:
            raise ValueError(f"PolynomialFeatures: degree must be an int in 1..3, got {degree!r}")
        if order != "C":
            raise ValueError(f"PolynomialFeatures: order={order!r} is not supported (the output is row-major, order='C')")
        for name, v in (("interaction_only", interaction_only), ("include_bias", include_bias)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"PolynomialFeatures: {name} must be a bool, got {v!r}")
        self.device = _device(device, self._who)
        self.degree, self.interaction_only, self.include_bias, self.order = int(degree), bool(interaction_only), bool(include_bias), "C"

    def _fit_shape(self, d):
        """The table of factor indices for ``d`` inputs; the refusals come before anything touches the device."""
        P = _n_output_features(d, self.degree, self.interaction_only, self.include_bias)
        if P > INT_MAX:
            raise ValueError(f"PolynomialFeatures: {d} features at degree {self.degree} give {P} output columns, more than 2**31 - 1")
        if P < 1:
            raise ValueError(f"PolynomialFeatures: {d} features at degree {self.degree} give no output column")
        table = np.full((P, 3), -1, dtype=np.int32)
        for p, c in enumerate(_combinations(d, self.degree, self.interaction_only, self.include_bias)):
            table[p, :len(c)] = c[::-1]                         # (k, j, i): the kernel multiplies in this order
        self._table, self._table_d = table, torch.from_numpy(table).to(self.device)
        self.n_features_in_, self.n_output_features_ = d, P

    @property
    def powers_(self):
        if not hasattr(self, "_table"):
            raise AttributeError("PolynomialFeatures: not fitted")
        out = np.zeros((self.n_output_features_, self.n_features_in_), dtype=np.int64)
        for col in range(3):
            rows = np.flatnonzero(self._table[:, col] >= 0)
            np.add.at(out, (rows, self._table[rows, col]), 1)
        return out

    def fit(self, X, y=None):
        self._fit_shape(_checked(X, self._who)[0].shape[1])
        return self

    def _transform(self, X, was_numpy):
        if not hasattr(self, "_table_d"):
            raise RuntimeError("PolynomialFeatures: not fitted")
        n, d = X.shape
        P = self.n_output_features_
        if d != self.n_features_in_:
            raise ValueError(f"PolynomialFeatures: the input has {d} features, the fit saw {self.n_features_in_}")
        with torch.cuda.device(self.device):
            try:
                out = torch.empty((n, P), dtype=torch.float64, device=self.device)
            except RuntimeError as e:                           # torch.OutOfMemoryError is one
                raise RuntimeError(f"PolynomialFeatures: the [{n}, {P}] float64 output ({n * P * 8} bytes) cannot be allocated: {e}") from e
            flag = torch.empty(1, dtype=torch.int32, device=self.device)
            _LAUNCHES["expand"] += 1
            _lib.check(_lib.lib().bbbp_poly_expand(_dense.stream(), X.data_ptr(), _dense.ld(X), n, d, self._table_d.data_ptr(), P, out.data_ptr(), P,
                                                   flag.data_ptr()), "bbbp_poly_expand")
            _raise_if_flagged(flag.cpu()[0], self._who)
        return _give_back(out, was_numpy)

    def transform(self, X):
        return self._transform(*_to_device(X, self.device, self._who))

    def fit_transform(self, X, y=None):
        Xh, was_numpy = _checked(X, self._who)
        self._fit_shape(Xh.shape[1])
        return self._transform(_moved(Xh, self.device), was_numpy)
