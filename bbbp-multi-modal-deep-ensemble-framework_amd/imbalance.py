"""``imblearn``'s ``SMOTE``, ``TomekLinks`` and ``SMOTETomek`` for the GPU: the resampling step of the classification stack.

Every classification script of the reference runs StandardScaler, ``PCA(100)``, ``SMOTE(random_state=42).fit_resample(X_reduced, y)`` and
then its learners (``Models/model_opt_maccs.py``, ``model_opt.py``, ``model_opt_rdkit.py``, ``model_opt_all-2.py``); the latest,
``Models/model_opt_20250130.py``, runs ``SMOTETomek(random_state=42)`` at that point.  Here the matrix stays on the device between the
PCA and the learners:

* ``SMOTE``: per resampled class, in ascending class order, the class rows' ``k_neighbors`` nearest rows of the same class come from
  ``neighbors.NearestNeighbors`` (``csrc/knn.hip``, order (distance, index)); the draws are imbalanced-learn's two calls on a
  ``numpy.random.RandomState``, made on the host -- ``randint(0, n_c * k, n_new)`` picks (base row, neighbour slot), ``uniform(size=n_new)``
  the steps -- and ``bbbp_smote_synth`` (``csrc/smote.hip``) writes ``base + step * (neighbour - base)`` straight into the tail of the
  result, rounded as numpy rounds that expression, so a numpy restatement (``tests/smote_numpy.py``) reproduces the result bit for bit.
  The original rows come first, unchanged and in order, then each class's synthetic rows.
* ``TomekLinks``: rows i and j of different classes that are each other's nearest row form a link; the members whose class the strategy
  names are removed (``bbbp_tomek_links`` writes the keep mask), the kept rows are returned in order, ``sample_indices_`` names them.
* ``SMOTETomek``: ``SMOTE``, then ``TomekLinks(sampling_strategy="all")`` on its output, without the matrix leaving the device.

``X`` is a CUDA tensor or a numpy array, float32 or float64, [n, d]; ``X_res`` comes back as what was given and in its dtype, ``y_res``
is always a numpy array of the labels' dtype (labels of any sortable dtype, strings included, are encoded on the host as ``numpy.unique``
does).  NaN or infinity in ``X`` raises the search's ``ValueError``.

Two deviations from imbalanced-learn:

1. Self-exclusion.  imbalanced-learn asks for ``k + 1`` neighbours and drops column 0, assuming it is the row itself.  Here a row is left
   out by index and ties go to the lower index.  The two differ only when a class holds duplicate rows.
2. Parity with imbalanced-learn is unpinned.  The package was not available where this was written and tested; the algorithm is written
   from imbalanced-learn's published source, and the draws are in its order, so with the same ``random_state`` and tie-free neighbour lists
   the output is expected to be equal -- nobody has checked that.  ``tests/test_smote_cpu.py`` holds the comparison for whoever has the
   package; it is skipped without it.

Not built: ``BorderlineSMOTE``, ``ADASYN``, ``SMOTENC``, ``RandomOverSampler``, sparse input, ``k_neighbors`` given as an estimator, a
callable ``sampling_strategy``, ``k_neighbors > 32``, more than one GPU.  There is no CPU path.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _dense, _lib
from .neighbors import NearestNeighbors, _check_k

_LAUNCHES = {"fit": 0, "search": 0, "synth": 0, "tomek": 0}       # library entry points per kind (tools/bench_smote.py reads the differences)
_SMOTE_STRATEGIES = ("auto", "not majority", "minority", "not minority", "all")
_TOMEK_STRATEGIES = ("auto", "not minority", "not majority", "majority", "all")


def check_random_state(seed):
    """scikit-learn's rule: ``None`` is numpy's global stream, an int seeds a fresh ``RandomState``, an instance is used as it is."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral) and not isinstance(seed, bool):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"imbalance: random_state must be None, an int or a numpy RandomState, got {seed!r}")


def _device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: device {str(device)!r}: resampling runs on the GPU (no CPU fallback)")
    return device


def _encode(X, y, who):
    """(y as an array, classes, ids int64 [n], counts per class) after the checks that need no device."""
    if not isinstance(X, torch.Tensor):
        X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"{who}: expected a 2-D [n, d] input, got shape {tuple(X.shape)}")
    y = np.asarray(y)
    if y.ndim != 1 or len(y) != X.shape[0]:
        raise ValueError(f"{who}: y must be 1-D with one label per row of X, got shapes {tuple(X.shape)} and {y.shape}")
    if len(y) == 0 or X.shape[1] == 0:
        raise ValueError(f"{who}: needs at least one row and one feature, got shape {tuple(X.shape)}")
    classes, ids = np.unique(y, return_inverse=True)
    return y, classes, ids.astype(np.int64).ravel(), np.bincount(ids.ravel(), minlength=len(classes))


def _class_index(classes, key, who):
    hit = np.flatnonzero(classes == key)
    if len(hit) != 1:
        raise ValueError(f"{who}: sampling_strategy names the class {key!r}, which y does not hold")
    return int(hit[0])


def _smote_targets(strategy, classes, counts):
    """{class id: n_new} for the over-sampler, as imbalanced-learn resolves ``sampling_strategy`` (the first class wins a tie for the
    majority or the minority); iterated in ascending class order."""
    n_max, maj, mino = int(counts.max()), int(np.argmax(counts)), int(np.argmin(counts))
    if isinstance(strategy, str):
        if strategy not in _SMOTE_STRATEGIES:
            raise ValueError(f"SMOTE: sampling_strategy must be one of {_SMOTE_STRATEGIES}, a float or a dict, got {strategy!r}")
        chosen = {"auto": [c for c in range(len(classes)) if c != maj], "not majority": [c for c in range(len(classes)) if c != maj],
                  "minority": [mino], "not minority": [c for c in range(len(classes)) if c != mino], "all": list(range(len(classes)))}[strategy]
        return {c: n_max - int(counts[c]) for c in chosen}
    if isinstance(strategy, dict):
        out = {}
        for key, target in strategy.items():
            c = _class_index(classes, key, "SMOTE")
            if isinstance(target, bool) or not isinstance(target, numbers.Integral) or target < 0:
                raise ValueError(f"SMOTE: the target count of class {key!r} must be a non-negative int, got {target!r}")
            if target < counts[c]:
                raise ValueError(f"SMOTE: class {key!r} has {int(counts[c])} rows, a target of {target} would remove some (over-sampling only adds)")
            out[c] = int(target) - int(counts[c])
        return dict(sorted(out.items()))
    if isinstance(strategy, numbers.Real) and not isinstance(strategy, bool):
        if len(classes) != 2:
            raise ValueError(f"SMOTE: a float sampling_strategy is the ratio minority / majority of two classes, y holds {len(classes)}")
        if not 0 < strategy <= 1:
            raise ValueError(f"SMOTE: a float sampling_strategy must lie in (0, 1], got {strategy!r}")
        other = 1 - maj
        n_new = int(strategy * n_max - int(counts[other]))
        if n_new < 0:
            raise ValueError(f"SMOTE: the ratio {strategy!r} would remove rows of the minority class ({int(counts[other])} of them against {n_max})")
        return {other: n_new}
    raise ValueError(f"SMOTE: sampling_strategy must be one of {_SMOTE_STRATEGIES}, a float or a dict, got {strategy!r}")


def _tomek_remove(strategy, classes, counts):
    """uint8 [n_classes]: 1 for the classes whose link members are removed."""
    maj, mino = int(np.argmax(counts)), int(np.argmin(counts))
    remove = np.zeros(len(classes), dtype=np.uint8)
    if isinstance(strategy, str):
        if strategy not in _TOMEK_STRATEGIES:
            raise ValueError(f"TomekLinks: sampling_strategy must be one of {_TOMEK_STRATEGIES} or a list of classes, got {strategy!r}")
        remove[:] = 1
        if strategy in ("auto", "not minority"):
            remove[mino] = 0
        elif strategy == "not majority":
            remove[maj] = 0
        elif strategy == "majority":
            remove[:] = 0
            remove[maj] = 1
        return remove
    if isinstance(strategy, (list, tuple, np.ndarray)):
        for key in strategy:
            remove[_class_index(classes, key, "TomekLinks")] = 1
        return remove
    raise ValueError(f"TomekLinks: sampling_strategy must be one of {_TOMEK_STRATEGIES} or a list of classes, got {strategy!r}")


def _fitted(X, device):
    _LAUNCHES["fit"] += 1
    return NearestNeighbors(1, device=device).fit(X)


def _neighbours(nbrs, k):
    _LAUNCHES["search"] += 1
    return nbrs._search(None, k)[1]


def _synthesize(Xc, nn, idx, steps, out):
    """``bbbp_smote_synth``: ``out`` [n_new, d] (a view with unit inner stride, of ``Xc``'s dtype) from the class matrix ``Xc`` [n_c, d], its
    neighbour lists ``nn`` [n_c, k] int64 and the device arrays ``idx`` int64 / ``steps`` float64 [n_new]."""
    (n_c, d), (n_new, k) = Xc.shape, (idx.numel(), nn.shape[1])
    assert out.shape == (n_new, d) and out.dtype == Xc.dtype and nn.is_contiguous() and idx.dtype == nn.dtype == torch.int64
    assert steps.dtype == torch.float64 and steps.numel() == n_new and (d == 1 or (Xc.stride(1) == 1 and out.stride(1) == 1))
    _LAUNCHES["synth"] += 1
    with torch.cuda.device(Xc.device):
        _lib.check(_lib.lib().bbbp_smote_synth(_dense.stream(), Xc.data_ptr(), _dense.DT[Xc.dtype], _dense.ld(Xc), n_c, nn.data_ptr(), idx.data_ptr(),
                                               steps.data_ptr(), k, n_new, d, out.data_ptr(), _dense.ld(out)), "bbbp_smote_synth")


def _keep_mask(nn1, ids_d, remove_d):
    """``bbbp_tomek_links``: the uint8 keep mask [n] from ``nn1`` int64 [n], the encoded labels int32 [n] and the per-class remove flags."""
    n = ids_d.numel()
    keep = torch.empty(n, dtype=torch.uint8, device=ids_d.device)
    _LAUNCHES["tomek"] += 1
    with torch.cuda.device(ids_d.device):
        _lib.check(_lib.lib().bbbp_tomek_links(_dense.stream(), nn1.data_ptr(), ids_d.data_ptr(), remove_d.data_ptr(), remove_d.numel(), n, keep.data_ptr()),
                   "bbbp_tomek_links")
    return keep


def _smote_device(X, ids, targets, k, random_state, device, check_all=True):
    """``X`` [n, d] on the device, ``ids`` int64 [n] on the host, ``targets`` {class id: n_new > 0}: (X_res on the device, ids_res).
    ``check_all``: put the whole matrix through the search's NaN / infinity check, not only the resampled classes (SMOTETomek's second
    stage does that anyway)."""
    n, d = X.shape
    total = sum(targets.values())
    if check_all:
        _fitted(X, device)
    out = torch.empty((n + total, d), dtype=X.dtype, device=device)
    out[:n].copy_(X)
    at = n
    for c, n_new in targets.items():
        rows = np.flatnonzero(ids == c)
        n_c = len(rows)
        rs = check_random_state(random_state)
        idx = rs.randint(0, n_c * k, size=n_new)
        steps = rs.uniform(size=n_new)
        Xc = X.index_select(0, torch.from_numpy(rows).to(device))
        nn = _neighbours(_fitted(Xc, device), k)
        _synthesize(Xc, nn, torch.from_numpy(idx.astype(np.int64)).to(device), torch.from_numpy(steps).to(device), out[at:at + n_new])
        at += n_new
    return out, np.concatenate([ids] + [np.full(n_new, c, dtype=np.int64) for c, n_new in targets.items()])


def _tomek_device(X, ids, remove, device):
    """Indices (int64, device, ascending) of the rows of ``X`` that stay."""
    if X.shape[0] < 2:
        return torch.arange(X.shape[0], device=device)
    nn1 = _neighbours(_fitted(X, device), 1)
    keep = _keep_mask(nn1, torch.from_numpy(ids.astype(np.int32)).to(device), torch.from_numpy(remove).to(device))
    return torch.nonzero(keep).flatten()


def _give_back(X_res, was_numpy):
    return X_res.cpu().numpy() if was_numpy else X_res


def _copy_of(X):
    return X.clone() if isinstance(X, torch.Tensor) else np.array(X)


class SMOTE:
    """``SMOTE(sampling_strategy="auto", random_state=None, k_neighbors=5, device="cuda")``: imbalanced-learn's names and
    ``fit_resample(X, y) -> (X_res, y_res)``.

    ``sampling_strategy``: ``"auto"`` / ``"not majority"``, ``"minority"``, ``"not minority"``, ``"all"`` (the named classes are filled up
    to the largest class), a float for two classes (the ratio minority / majority afterwards: ``int(ratio * n_maj - n_min)`` new rows) or a
    dict ``{class: target count}``.  An int ``random_state`` seeds a fresh ``RandomState`` per class, an instance continues.  A resampled
    class needs more than ``k_neighbors`` rows.  A balanced input returns copies and launches nothing."""

    def __init__(self, sampling_strategy="auto", random_state=None, k_neighbors=5, device="cuda"):
        self.device = _device(device, "SMOTE")
        self.k_neighbors = _check_k(k_neighbors, "k_neighbors")
        if isinstance(sampling_strategy, str) and sampling_strategy not in _SMOTE_STRATEGIES:
            raise ValueError(f"SMOTE: sampling_strategy must be one of {_SMOTE_STRATEGIES}, a float or a dict, got {sampling_strategy!r}")
        if random_state is not None:
            check_random_state(random_state)
        self.sampling_strategy, self.random_state = sampling_strategy, random_state

    def _plan(self, X, y):
        y, classes, ids, counts = _encode(X, y, "SMOTE")
        targets = {c: m for c, m in _smote_targets(self.sampling_strategy, classes, counts).items() if m > 0}
        for c in targets:
            if counts[c] <= self.k_neighbors:
                raise ValueError(f"SMOTE: class {classes[c]!r} has {int(counts[c])} rows, k_neighbors={self.k_neighbors} needs more than that many")
        return y, classes, ids, targets

    def _resample_device(self, X, ids, targets, check_all=True):
        return _smote_device(X, ids, targets, self.k_neighbors, self.random_state, self.device, check_all)

    def fit_resample(self, X, y):
        y, classes, ids, targets = self._plan(X, y)
        if not targets:
            if isinstance(X, torch.Tensor) and not X.is_cuda:
                raise RuntimeError(f"SMOTE: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU fallback)")
            return _copy_of(X), y.copy()
        Xd, was_numpy = _dense.to_device_matrix(X, self.device, "SMOTE", allow_row_stride=True)
        X_res, ids_res = self._resample_device(Xd, ids, targets)
        return _give_back(X_res, was_numpy), classes[ids_res]


class TomekLinks:
    """``TomekLinks(sampling_strategy="auto", device="cuda")``: removes the members of Tomek links -- pairs of rows of different classes
    that are each other's nearest row -- whose class the strategy names: ``"auto"`` / ``"not minority"`` every class but the smallest,
    ``"not majority"``, ``"majority"``, ``"all"``, or a list of classes.  The kept rows are returned in order; ``sample_indices_`` (numpy
    int64) names them."""

    def __init__(self, sampling_strategy="auto", device="cuda"):
        self.device = _device(device, "TomekLinks")
        if not (sampling_strategy in _TOMEK_STRATEGIES if isinstance(sampling_strategy, str) else isinstance(sampling_strategy, (list, tuple, np.ndarray))):
            raise ValueError(f"TomekLinks: sampling_strategy must be one of {_TOMEK_STRATEGIES} or a list of classes, got {sampling_strategy!r}")
        self.sampling_strategy = sampling_strategy

    def _clean_device(self, X, ids, classes):
        """(X_res, ids_res) for a device matrix and encoded labels; sets ``sample_indices_``."""
        remove = _tomek_remove(self.sampling_strategy, classes, np.bincount(ids, minlength=len(classes)))
        kept = _tomek_device(X, ids, remove, self.device)
        self.sample_indices_ = kept.cpu().numpy().astype(np.int64)
        return X.index_select(0, kept), ids[self.sample_indices_]

    def fit_resample(self, X, y):
        y, classes, ids, counts = _encode(X, y, "TomekLinks")
        _tomek_remove(self.sampling_strategy, classes, counts)
        Xd, was_numpy = _dense.to_device_matrix(X, self.device, "TomekLinks", allow_row_stride=True)
        X_res, _ = self._clean_device(Xd, ids, classes)
        return _give_back(X_res, was_numpy), y[self.sample_indices_]


class SMOTETomek:
    """``SMOTETomek(sampling_strategy="auto", random_state=None, smote=None, tomek=None, device="cuda")``: ``SMOTE`` (built from
    ``sampling_strategy`` and ``random_state`` unless an instance is given), then ``TomekLinks(sampling_strategy="all")`` (or the given
    instance) on its output; the matrix stays on the device in between."""

    def __init__(self, sampling_strategy="auto", random_state=None, smote=None, tomek=None, device="cuda"):
        self.device = _device(device, "SMOTETomek")
        if smote is not None and not isinstance(smote, SMOTE):
            raise ValueError(f"SMOTETomek: smote must be an imbalance.SMOTE, got {type(smote).__name__}")
        if tomek is not None and not isinstance(tomek, TomekLinks):
            raise ValueError(f"SMOTETomek: tomek must be an imbalance.TomekLinks, got {type(tomek).__name__}")
        for part in (smote, tomek):
            if part is not None and part.device != self.device:
                raise ValueError(f"SMOTETomek: {type(part).__name__} is set up for {part.device}, this estimator for {self.device}")
        self.smote_ = smote if smote is not None else SMOTE(sampling_strategy, random_state, device=device)
        self.tomek_ = tomek if tomek is not None else TomekLinks("all", device=device)
        self.sampling_strategy, self.random_state, self.smote, self.tomek = sampling_strategy, random_state, smote, tomek

    def fit_resample(self, X, y):
        y, classes, ids, targets = self.smote_._plan(X, y)
        _tomek_remove(self.tomek_.sampling_strategy, classes, np.bincount(ids, minlength=len(classes)))       # its errors before any launch; the set itself follows the resampled counts
        Xd, was_numpy = _dense.to_device_matrix(X, self.device, "SMOTETomek", allow_row_stride=True)
        if targets:
            Xd, ids = self.smote_._resample_device(Xd, ids, targets, check_all=False)
        X_res, ids_res = self.tomek_._clean_device(Xd, ids, classes)
        return _give_back(X_res, was_numpy), classes[ids_res]
