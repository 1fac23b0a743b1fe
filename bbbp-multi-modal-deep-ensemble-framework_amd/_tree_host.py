"""What the host sides of the tree learners share (``random_forest``, ``gradient_boosting``, ``trees.ForestGPU``): input validation, the
training matrix on the device, scikit-learn's ``tree_`` objects as flat arrays, the grid's points and the small uploads.  Private: the
learners' modules are the API.  Every function takes ``who``, the name its messages begin with.

Flat trees are a dict of host arrays: ``left`` / ``right`` (int32, absolute child indices, -1 at a leaf), ``feature`` (int32, 0 at a leaf),
``threshold`` and ``value`` (float64), ``n_node_samples`` (int32) and ``root`` (int32, ``root[t]`` the first node of tree t, one entry past
the last tree)."""
from __future__ import annotations

import numbers
from itertools import product

import numpy as np
import torch


def is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


class Matrix:
    """One training matrix on the device: float32 by columns, and every column's rows sorted stably by value (``torch.sort``: done once
    per matrix, outside the hot path)."""

    def __init__(self, X32, device):
        X32 = X32 if isinstance(X32, torch.Tensor) else torch.from_numpy(X32)
        self.XT = X32.to(device).t().contiguous()
        self.order0 = torch.sort(self.XT, dim=1, stable=True).indices.to(torch.int32).contiguous()
        self.d, self.n = self.XT.shape


def training_matrix32(X, who, max_rows, max_features, limit_prefix):
    """X as float32 [n, d], numpy (host) or a CUDA tensor, checked for shape and finiteness; a numpy input never touches the GPU here.
    ``limit_prefix`` names the kernels' limits in the messages (``BBBP_RF_FIT_MAX`` gives ``BBBP_RF_FIT_MAX_N`` and ``..._D``)."""
    on_device = isinstance(X, torch.Tensor)
    if on_device and not X.is_cuda:
        raise RuntimeError(f"{who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU fallback)")
    if not on_device:
        X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"{who}: expected a 2-D [n, d] input, got shape {tuple(X.shape)}")
    n, d = X.shape
    if n < 2 or d < 1:
        raise ValueError(f"{who}: need at least two rows and one feature, got shape {(n, d)}")
    if n > max_rows:
        raise ValueError(f"{who}: n = {n} rows, at most {max_rows} are supported ({limit_prefix}_N)")
    if d > max_features:
        raise ValueError(f"{who}: d = {d} features, at most {max_features} are supported ({limit_prefix}_D)")
    if on_device:
        X32 = X.to(torch.float32)
        finite = bool(torch.isfinite(X32).all())
    else:
        with np.errstate(over="ignore"):
            X32 = np.ascontiguousarray(X, dtype=np.float32)
        finite = bool(np.isfinite(X32).all())
    if not finite:
        raise ValueError(f"{who}: X contains NaN, infinity or a value too large for float32")
    return X32


def targets_1d(y, n_rows, who, many_columns_message):
    """Regression targets as finite float64 [n_rows] on the host, unrounded; [n, 1] is taken as [n]."""
    y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
    if y.ndim == 2 and y.shape[1] == 1:
        y = y[:, 0]
    if y.ndim != 1:
        raise NotImplementedError(f"{who}: {many_columns_message}, got y of shape {y.shape}")
    try:
        y = np.ascontiguousarray(y, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: y must be numeric, got dtype {y.dtype}") from None
    if len(y) != n_rows:
        raise ValueError(f"{who}: X has {n_rows} rows, y has {len(y)}")
    if not np.isfinite(y).all():
        raise ValueError(f"{who}: y contains NaN or infinity")
    return y


def refuse_non_defaults(who, other, defaults, ignored=()):
    """scikit-learn's further constructor parameters: ``ignored`` ones pass with any value, the others only with their default."""
    for name, value in other.items():
        if name in ignored:
            continue
        if name not in defaults:
            raise ValueError(f"{who}: unknown parameter {name}")
        if value is not defaults[name] and not (isinstance(value, (numbers.Real, str)) and value == defaults[name]):
            raise NotImplementedError(f"{who}: {name}={value!r} is not supported (only {defaults[name]!r})")


def check_trees(trees, n_features, who, keys):
    """Host-side validation of flat trees handed to a walking kernel: every index it follows stays inside its arrays.  ``keys``: the arrays
    that must be as long as ``left``."""
    left, right, feature, root = trees["left"], trees["right"], trees["feature"], trees["root"]
    n_nodes = len(left)
    if not all(len(trees[k]) == n_nodes for k in keys) or root[-1] != n_nodes or root[0] != 0:
        raise ValueError(f"{who}: tree arrays of unequal length")
    if np.any(np.diff(root) < 1):
        raise ValueError(f"{who}: an empty tree")
    split = left >= 0
    if np.any(left[split] >= n_nodes) or np.any(right[split] < 0) or np.any(right[split] >= n_nodes) or np.any(feature < 0) or np.any(feature >= n_features):
        raise ValueError(f"{who}: a child or feature index outside its array")


def query_matrix(model, X, device, who):
    """The queries of a fitted model as float32 [m, d] on ``device``, and whether they came as numpy."""
    if not hasattr(model, "_dev"):
        raise RuntimeError(f"{who}: not fitted")
    was_numpy = not isinstance(X, torch.Tensor)
    if was_numpy:
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"{who}: expected a 2-D [m, d] input, got shape {X.shape}")
        with np.errstate(over="ignore"):
            X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    elif not X.is_cuda:
        raise RuntimeError(f"{who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU fallback)")
    if X.dim() != 2 or X.shape[1] != model.n_features_in_:
        raise ValueError(f"{who}: the queries must be [m, {model.n_features_in_}], got shape {tuple(X.shape)}")
    return X.to(device, torch.float32).contiguous(), was_numpy


def rebase_children(left, right, offsets):
    """Child indices counted from their own tree's first node as absolute int32 indices (``offsets``: that node, per node or one number);
    -1 stays -1."""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    return np.where(left >= 0, left + offsets, -1).astype(np.int32), np.where(right >= 0, right + offsets, -1).astype(np.int32)


def sklearn_trees(estimators, value_columns=None, who=""):
    """The ``tree_`` objects of fitted single-output scikit-learn trees as flat trees without ``value``, and the values: one float64 array per
    entry of ``value_columns`` (columns of ``tree_.value[:, 0, :]``: a classifier's classes), or with None the one value a node holds (more
    than one per node is an error)."""
    left, right, feature, threshold, nns, root = [], [], [], [], [], [0]
    values = [[] for _ in (value_columns or (0,))]
    for est in estimators:
        t, off = est.tree_, root[-1]
        l, r = rebase_children(t.children_left, t.children_right, off)
        left.append(l); right.append(r)
        feature.append(np.where(t.feature >= 0, t.feature, 0)); threshold.append(t.threshold); nns.append(t.n_node_samples)
        if value_columns is None:
            values[0].append(t.value.reshape(t.node_count))
        else:
            for v, col in zip(values, value_columns):
                v.append(t.value[:, 0, col])
        root.append(off + t.node_count)
    if root[-1] >= 2 ** 31:
        raise ValueError(f"{who}forest too large for 32-bit node indices")
    cat = np.concatenate
    trees = dict(left=cat(left), right=cat(right), feature=cat(feature).astype(np.int32), threshold=cat(threshold).astype(np.float64),
                 n_node_samples=cat(nns).astype(np.int32), root=np.asarray(root, dtype=np.int32))
    return trees, tuple(cat(v).astype(np.float64) for v in values)


def grid_points(param_grid, keys, defaults, check, who):
    """The grid's points in scikit-learn's order (sorted keys, ``itertools.product``; a list of grids one after the other) and each point's
    full parameter tuple in ``keys``' order, every one passed through ``check(*params, who=who)``."""
    points = []
    for sub in ([param_grid] if isinstance(param_grid, dict) else list(param_grid)):
        unknown = set(sub) - set(keys)
        if unknown:
            raise ValueError(f"{who}: unsupported grid keys {sorted(unknown)}")
        names = sorted(sub)
        points += [dict(zip(names, vals)) for vals in product(*(sub[k] for k in names))]
    if not points:
        raise ValueError(f"{who}: the grid is empty")
    full = [tuple({**defaults, **pt}[k] for k in keys) for pt in points]
    for params in full:
        check(*params, who=who)
    return points, full


def upload(arr, device):
    """A ctypes array of descriptors as bytes on the device; the caller keeps the tensor alive until the kernels that read it are done."""
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def to_device(trees, keys, f64_keys, device):
    """{key: tensor on ``device``} of ``trees[key]``: float64 for ``f64_keys``, int32 for the rest."""
    return {k: torch.from_numpy(np.ascontiguousarray(trees[k], dtype=np.float64 if k in f64_keys else np.int32)).to(device) for k in keys}
