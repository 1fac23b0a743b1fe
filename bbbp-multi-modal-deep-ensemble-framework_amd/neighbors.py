"""``sklearn.neighbors`` for the GPU: brute-force k-nearest-neighbour search in float64, and the classifier on top of it.

The classification stack of the reference (``Models/model_opt_maccs.py``) runs StandardScaler, ``PCA(100)``, SMOTE and eight learners under
``GridSearchCV(cv=5, scoring='f1')``; ``KNeighborsClassifier()`` is searched over ``n_neighbors in {3, 5, 7} x weights in {uniform,
distance}`` (lines 126, 143-144).  Its search primitive -- the k nearest training rows of every query, Euclidean, in float64 -- is one
fused launch sequence of ``csrc/knn.hip``: the distance block of 64 queries x 64 training rows is formed on the float64 matrix pipe from
rows centred at the training mean and consumed by the selection in the same kernel, so the [m, n] distance matrix never exists in memory.
The kept neighbours get their distances recomputed by direct differences: a duplicate of a query is at distance exactly 0.

* ``NearestNeighbors``: ``fit`` / ``kneighbors`` (``X=None`` queries the training rows without themselves -- the query a SMOTE starts with);
* ``KNeighborsClassifier``: ``fit`` / ``predict`` / ``predict_proba`` / ``kneighbors``, ``weights`` ``"uniform"`` or ``"distance"``;
* ``grid_search_cv``: the reference's grid with one search per fold; every grid point is a vote over a prefix of that fold's lists.

Neighbours are ordered by (distance, training index): among equidistant rows the lower index comes first.

SMOTE, TomekLinks and SMOTETomek are built on this search in ``imbalance``.  Out of scope: tree / ball-tree indices,
approximate search, metrics other than Euclidean, ``radius_neighbors``, regression, ``n_neighbors > 32``, more than 32 classes, more than
one GPU.  There is no CPU path.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _estimator, _dense, _lib

MAX_NEIGHBORS = 32
MAX_CLASSES = 32
_WEIGHTS = {"uniform": 0, "distance": 1}


def _check_k(k, what="n_neighbors"):
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise ValueError(f"{what} must be an int, got {k!r}")
    if not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"{what}={k} must be between 1 and {MAX_NEIGHBORS}")
    return int(k)


def _vote(dist, ind, kk, labels, n_classes, weights):
    """``bbbp_knn_vote`` over the first ``kk`` columns of ``dist`` / ``ind`` [m, k]: (proba [m, n_classes] float64, pred [m] int32)."""
    m, k = dist.shape
    proba = torch.empty((m, n_classes), dtype=torch.float64, device=dist.device)
    pred = torch.empty(m, dtype=torch.int32, device=dist.device)
    if m:
        with torch.cuda.device(dist.device):
            _lib.check(_lib.lib().bbbp_knn_vote(_dense.stream(), dist.data_ptr(), ind.data_ptr(), m, k, kk, labels.data_ptr(), labels.numel(), n_classes,
                                                _WEIGHTS[weights], proba.data_ptr(), pred.data_ptr()), "bbbp_knn_vote")
    return proba, pred


class NearestNeighbors:
    """``NearestNeighbors(n_neighbors=5, *, device="cuda")``: scikit-learn's names, ``algorithm="brute"``, Euclidean metric.

    ``fit`` takes a CUDA tensor or a numpy array, float32 or float64, [n, d], and keeps it on the device (non-contiguous input is copied);
    ``mean_`` is the float64 column mean the search centres on.  ``kneighbors`` returns ``(dist [m, k] float64, ind [m, k] int64)``: numpy
    arrays for numpy input or ``None``, CUDA tensors for a CUDA tensor."""

    def __init__(self, n_neighbors=5, *, device="cuda", **unsupported):
        if unsupported:
            raise ValueError(f"NearestNeighbors: unsupported parameters {sorted(unsupported)} (brute-force Euclidean search only)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"NearestNeighbors: device {device!r}: the search runs on the GPU (no CPU fallback)")
        self.n_neighbors = _check_k(n_neighbors)

    # ---- input handling ---------------------------------------------------------------------------------------------
    def _to_device(self, X):
        """(device tensor [n, d] float32 / float64 with unit inner stride, a row / column slice of a larger matrix in place; was_numpy)"""
        return _dense.to_device_matrix(X, self.device, "neighbors", allow_row_stride=True)

    def _norms(self, X, what):
        """Centred squared row norms of X (float64, device); ValueError when X holds NaN or infinity (one host read of the flag)."""
        n, d = X.shape
        norms = torch.empty(n, dtype=torch.float64, device=self.device)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().bbbp_knn_row_norms(_dense.stream(), X.data_ptr(), _dense.DT[X.dtype], n, d, _dense.ld(X), self._mean_d.data_ptr(), norms.data_ptr(),
                                                 flag.data_ptr()), "bbbp_knn_row_norms")
        if int(flag.item()):
            raise ValueError(f"neighbors: {what} contains NaN or infinity (or values whose squares overflow float64)")
        return norms

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y=None):
        X, _ = self._to_device(X)
        n, d = X.shape
        if n < 1 or d < 1:
            raise ValueError(f"neighbors: fit needs at least one row and one feature, got shape {(n, d)}")
        for name in ("_X", "_norms_d", "_mean_d"):
            self.__dict__.pop(name, None)
        with torch.cuda.device(self.device):
            self._mean_d = torch.empty(d, dtype=torch.float64, device=self.device)
            _lib.check(_lib.lib().bbbp_pca_col_mean(_dense.stream(), X.data_ptr(), _dense.DT[X.dtype], n, d, _dense.ld(X), self._mean_d.data_ptr()), "bbbp_pca_col_mean")
            try:
                self._norms_d = self._norms(X, "the training set")
            except ValueError:
                del self._mean_d
                raise
        self._X = X
        self.mean_ = self._mean_d.cpu().numpy()
        self.n_samples_fit_, self.n_features_in_ = n, d
        return self

    # ---- search -----------------------------------------------------------------------------------------------------
    def _search(self, Xq, k, *, slices=0):
        """(dist, ind) device tensors for device queries ``Xq`` (``None``: the training rows, each without itself)."""
        if not hasattr(self, "_X"):
            raise RuntimeError("neighbors: not fitted")
        n, d = self._X.shape
        k = self.n_neighbors if k is None else _check_k(k)
        exclude = Xq is None
        avail = n - 1 if exclude else n
        if k > avail:
            raise ValueError(f"neighbors: n_neighbors={k} exceeds the {avail} training rows a query can be given"
                             + (" (X=None leaves a row's own copy out)" if exclude else ""))
        if not exclude and Xq.shape[1] != d:
            raise ValueError(f"neighbors: the queries have {Xq.shape[1]} features, the fit saw {d}")
        with torch.cuda.device(self.device):
            Q = self._X if exclude else Xq
            m = Q.shape[0]
            dist = torch.empty((m, k), dtype=torch.float64, device=self.device)
            ind = torch.empty((m, k), dtype=torch.int64, device=self.device)
            if m == 0:
                return dist, ind
            qn = self._norms_d if exclude else self._norms(Q, "the query set")
            desc = _lib.KnnDesc(m, n, d, k, Q.data_ptr(), _dense.DT[Q.dtype], _dense.ld(Q), self._X.data_ptr(), _dense.DT[self._X.dtype],
                                _dense.ld(self._X), self._mean_d.data_ptr(), qn.data_ptr(), self._norms_d.data_ptr(), dist.data_ptr(),
                                ind.data_ptr(), int(exclude), int(slices))
            L = _lib.lib()
            _dense.launch_with_workspace(L.bbbp_knn_workspace_bytes, L.bbbp_knn_f64, desc, self.device, "bbbp_knn_f64")
        return dist, ind

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True, *, slices=0):
        """The ``n_neighbors`` nearest training rows of every row of ``X`` (``None``: of every training row, itself left out).
        ``slices`` > 0 forces the number of training slices (a test hook: the result does not depend on it)."""
        if not hasattr(self, "_X"):
            raise RuntimeError("neighbors: not fitted")
        if X is None:
            Xq, was_numpy = None, True
        else:
            Xq, was_numpy = self._to_device(X)
        dist, ind = self._search(Xq, n_neighbors, slices=slices)
        if was_numpy:
            dist, ind = dist.cpu().numpy(), ind.cpu().numpy()
        return (dist, ind) if return_distance else ind


class KNeighborsClassifier(_estimator.Params, NearestNeighbors):
    """``KNeighborsClassifier(n_neighbors=5, *, weights="uniform", device="cuda")``.

    ``fit(X, y)`` maps the labels (any sortable values, at most 32 distinct) to ids as ``numpy.unique`` does (``classes_``).
    ``predict_proba`` adds the neighbours' weights per class in neighbour order (1, or 1 / distance with scikit-learn's rule for zero
    distances) and normalises; ``predict`` is the class of largest weight, the first in ``classes_`` on ties."""

    def __init__(self, n_neighbors=5, *, weights="uniform", device="cuda", **unsupported):
        if unsupported:
            raise ValueError(f"KNeighborsClassifier: unsupported parameters {sorted(unsupported)} (brute-force Euclidean search only)")
        if weights not in _WEIGHTS:
            raise ValueError(f"KNeighborsClassifier: weights must be 'uniform' or 'distance', got {weights!r}")
        super().__init__(n_neighbors, device=device)
        self.weights = weights

    _params = ("n_neighbors", "weights", "device")

    def fit(self, X, y):
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError(f"KNeighborsClassifier: y must be 1-D, got shape {y.shape}")
        classes, ids = np.unique(y, return_inverse=True)
        if len(classes) > MAX_CLASSES:
            raise ValueError(f"KNeighborsClassifier: {len(classes)} classes, at most {MAX_CLASSES} are supported")
        super().fit(X)
        if len(y) != self.n_samples_fit_:
            del self._X
            raise ValueError(f"KNeighborsClassifier: X has {self.n_samples_fit_} rows, y has {len(y)}")
        self.classes_ = classes
        self._labels_d = torch.from_numpy(ids.astype(np.int32)).to(self.device)
        return self

    def _proba(self, X):
        if not hasattr(self, "_X"):
            raise RuntimeError("neighbors: not fitted")
        Xq, was_numpy = self._to_device(X)
        dist, ind = self._search(Xq, self.n_neighbors)
        proba, pred = _vote(dist, ind, self.n_neighbors, self._labels_d, len(self.classes_), self.weights)
        return proba, pred, was_numpy

    def predict_proba(self, X):
        proba, _, was_numpy = self._proba(X)
        return proba.cpu().numpy() if was_numpy else proba

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype (labels need not be numbers, so they stay on the host)."""
        _, pred, _ = self._proba(X)
        return self.classes_[pred.cpu().numpy()]


def grid_search_cv(X, y, param_grid: dict, cv: int = 5, device="cuda"):
    """The reference's ``GridSearchCV(KNeighborsClassifier(), param_grid, cv=5, scoring='f1')`` (model_opt_maccs.py:126, 143-144).

    Same conventions as ``mlp.grid_search_cv``: sorted keys, ``itertools.product`` order, scikit-learn's ``StratifiedKFold(cv)``,
    ``f1_score``, the first maximum wins.  Per fold there is one search with ``max(n_neighbors)``; every grid point is a vote over a
    prefix of that list.  Returns (best_params, mean F1 per point, the classifier refitted on all rows with best_params)."""
    from itertools import product
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    unknown = set(param_grid) - {"n_neighbors", "weights"}
    if unknown:
        raise ValueError(f"neighbors.grid_search_cv: unsupported grid keys {sorted(unknown)}")
    grid = {"n_neighbors": list(param_grid.get("n_neighbors", [5])), "weights": list(param_grid.get("weights", ["uniform"]))}
    for w in grid["weights"]:
        if w not in _WEIGHTS:
            raise ValueError(f"neighbors.grid_search_cv: weights must be 'uniform' or 'distance', got {w!r}")
    kmax = max(_check_k(k) for k in grid["n_neighbors"])
    keys = sorted(param_grid)
    points = [dict(zip(keys, vals)) for vals in product(*(param_grid[k] for k in keys))]
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    y = np.asarray(y)
    folds = list(StratifiedKFold(n_splits=cv).split(X, y))
    f1 = np.zeros((len(points), len(folds)))
    for fi, (tr, te) in enumerate(folds):
        clf = KNeighborsClassifier(kmax, device=device).fit(X[tr], y[tr])
        dist, ind = clf._search(clf._to_device(X[te])[0], kmax)
        votes = {}
        for pi, pt in enumerate(points):
            key = (int(pt.get("n_neighbors", 5)), pt.get("weights", "uniform"))
            if key not in votes:
                votes[key] = clf.classes_[_vote(dist, ind, key[0], clf._labels_d, len(clf.classes_), key[1])[1].cpu().numpy()]
            f1[pi, fi] = f1_score(y[te], votes[key])
    scores = [float(v) for v in f1.mean(axis=1)]
    best = int(np.argmax(scores))
    fitted = KNeighborsClassifier(int(points[best].get("n_neighbors", 5)), weights=points[best].get("weights", "uniform"), device=device).fit(X, y)
    return points[best], scores, fitted
