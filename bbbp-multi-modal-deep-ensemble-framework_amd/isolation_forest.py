"""``sklearn.ensemble.IsolationForest`` for the GPU: random trees on small sub-samples, all grown in one launch, and scikit-learn's anomaly
score of any number of rows.

Every preprocessing script of the reference that feeds the regression models ends with
``IsolationForest(contamination=0.05, random_state=42).fit_predict(features)`` on the 30 + 30 PCA columns
(``Descriptors/multi_input_data_preprocess_maccs_opt_IsolationForest*.py``, ``create_descriptors_PCA_regression_{1,2,3}.py``): the step
between ``decomposition.PCA`` and the training loop.  The entry points of ``csrc/iforest.hip`` carry it:

* ``bbbp_iforest_fit`` grows every tree in one launch, one work-group per tree, the tree's rows and node tables in LDS, no host read per
  level.  A fit reads only its sub-samples, so there is no limit on the rows of ``X``; a tree takes at most 1 024 rows
  (``BBBP_IFOREST_MAX_SAMPLES``; scikit-learn's default is 256).
* ``bbbp_iforest_path_sum`` walks query rows through the trees and sums the leaves' path terms in tree order in float64.

The rule is scikit-learn 1.7's ``ExtraTreeRegressor(max_features=1, splitter="random")`` as ``IsolationForest`` uses it: a node is a leaf
with fewer than two rows, at depth ``ceil(log2(max(max_samples_, 2)))`` or when every feature is constant on its rows; otherwise its feature
is uniform among the features that are not constant there and its threshold uniform in [min, max) of that feature.  scikit-learn's further
stop on the impurity of its random ``y`` has no counterpart here: a tree has no target.  scikit-learn's per-tree random stream cannot be
matched; as in ``random_forest`` every random choice is one counter-based hash (``bbbp_rf_hash``) of the seed, the tree's number and the
node's path, under a key tag of its own (``include/bbbp_hip.h`` states the keys).  ``random_state`` is therefore part of the model and must
be an int when ``fit`` is called, and a forest of fewer trees is a prefix of a larger one.  ``tests/iforest_numpy.py`` reproduces a fit bit
for bit; trees are certified (``tests/iforest_replay.py``) and compared with scikit-learn's in distribution, not tree by tree.

The score is scikit-learn's bit for bit.  On the host, in numpy: a node's path term ``(depth + c(n_node_samples)) - 1.0``, depth counted
from 1 at the root and ``c`` the average path length of ``_average_path_length``; the kernel returns every row's sum over the trees; the
host finishes with ``-(2.0 ** -(sum / (T * c(max_samples_))))``, also for CUDA inputs (m doubles cross the bus: a device ``pow`` would not
give numpy's bits).  ``from_sklearn`` adopts a fitted scikit-learn model and scores like it.

Out of scope, each refused by name: ``max_features != 1.0``, ``bootstrap=True``, ``sample_weight``, sparse input, NaN or infinity in ``X``
(scikit-learn lets NaN through), ``warm_start``, ``max_samples_`` above 1 024, more than 1 024 features, more than one GPU.  There is no
CPU path.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from . import _dense, _lib, _tree_host
from ._tree_host import is_int as _is_int

MAX_SAMPLES, MAX_FEATURES, MAX_ROWS = 1024, 1024, 2147483392          # BBBP_IFOREST_MAX_SAMPLES, BBBP_IFOREST_MAX_D, BBBP_IFOREST_MAX_N
MAX_TREES = 65535                                  # one work-group per tree, one launch
_SKLEARN_DEFAULTS = dict(warm_start=False, n_jobs=None, verbose=0)
_TREE_KEYS = ("left", "right", "feature", "threshold", "value", "n_node_samples", "root")
_GROWN = {"launches": 0}                           # fit launches of this process (tests and the bench tool count them)


def average_path_length(n_samples_leaf):
    """scikit-learn's ``_average_path_length``: the mean depth of an unsuccessful search in a binary tree of that many rows, float64."""
    n = np.asarray(n_samples_leaf)
    shape = n.shape
    n = n.reshape((1, -1))
    out = np.zeros(n.shape)
    mask_1, mask_2 = n <= 1, n == 2
    rest = ~np.logical_or(mask_1, mask_2)
    out[mask_1] = 0.0
    out[mask_2] = 1.0
    out[rest] = 2.0 * (np.log(n[rest] - 1.0) + np.euler_gamma) - 2.0 * (n[rest] - 1.0) / n[rest]
    return out.reshape(shape)


def node_depths(trees):
    """Every node's depth counted from 1 at its tree's root (``tree_.compute_node_depths()``), int64, for flat trees in any numbering."""
    left, right = trees["left"], trees["right"]
    depth = np.zeros(len(left), dtype=np.int64)
    level, at = np.asarray(trees["root"][:-1], dtype=np.int64), 1
    while len(level):
        depth[level] = at
        inner = level[left[level] >= 0]
        level = np.concatenate([left[inner], right[inner]]).astype(np.int64)
        at += 1
    return depth


def path_terms(trees):
    """What a walk that ends in each node adds to a row's sum: ``(depth + c(n_node_samples)) - 1.0`` as scikit-learn adds it."""
    return (node_depths(trees) + average_path_length(trees["n_node_samples"].astype(np.int64))) - 1.0


def scores_of_path_sums(sums, n_trees, max_samples):
    """scikit-learn's ``score_samples`` from the rows' path sums: ``-(2 ** -(sum / (T c(max_samples))))``; 1 where the denominator is 0."""
    depths = np.asarray(sums, dtype=np.float64)
    denominator = n_trees * average_path_length(np.asarray([max_samples]))
    scores = 2 ** (-np.divide(depths, denominator, out=np.ones_like(depths), where=denominator != 0))
    return -scores


def resolve_max_samples(max_samples, n, who="IsolationForest"):
    """scikit-learn's ``max_samples_`` (``ensemble/_iforest.py:331-349``): "auto" is ``min(256, n)``, an int is clamped to n with a warning,
    a float is ``int(max_samples * n)``."""
    if isinstance(max_samples, str):
        if max_samples != "auto":
            raise ValueError(f"{who}: max_samples must be 'auto', an int or a float, got {max_samples!r}")
        return min(256, n)
    if _is_int(max_samples):
        if max_samples < 1:
            raise ValueError(f"{who}: max_samples must be >= 1, got {max_samples!r}")
        if max_samples > n:
            warnings.warn(f"max_samples ({max_samples}) is greater than the total number of samples ({n}). max_samples will be set to n_samples for "
                          "estimation.", UserWarning, stacklevel=3)
            return int(n)
        return int(max_samples)
    if isinstance(max_samples, numbers.Real) and not isinstance(max_samples, bool):
        if not 0.0 < max_samples <= 1.0:
            raise ValueError(f"{who}: a fractional max_samples must lie in (0, 1], got {max_samples!r}")
        resolved = int(max_samples * n)
        if resolved < 1:
            raise ValueError(f"{who}: max_samples = {max_samples!r} of {n} rows leaves no row")
        return resolved
    raise ValueError(f"{who}: max_samples must be 'auto', an int or a float, got {max_samples!r}")


def depth_limit(max_samples_):
    """``ceil(log2(max(max_samples_, 2)))`` in integers."""
    return max(1, (int(max_samples_) - 1).bit_length())


def _is_sparse(X):
    return hasattr(X, "tocsr") or (isinstance(X, torch.Tensor) and X.layout != torch.strided)


class IsolationForest:
    """``IsolationForest(*, n_estimators=100, max_samples="auto", contamination="auto", max_features=1.0, bootstrap=False, random_state=None,
    device="cuda")``: scikit-learn 1.7's names.

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (d <= 1 024, any n; cast to float32, as scikit-learn's trees do) and sets
    ``max_samples_``, ``n_features_in_``, ``offset_`` (-0.5, or with a ``contamination`` the percentile of the training scores, one more
    scoring launch), ``estimators_samples_`` (int32 [T, max_samples_]: each tree's rows, ascending) and ``trees_``: ``left``, ``right``,
    ``feature``, float64 ``threshold``, ``n_node_samples`` and ``root`` in ``_tree_host``'s flat convention, nodes numbered level by level,
    and ``value``, the path term of a walk that ends in the node.  ``random_state`` must be an int by then: the seed is part of the model.
    A node is a leaf with fewer than two rows, at the depth limit or when every feature is constant on its rows; scikit-learn's stop on the
    impurity of its random target does not exist here.

    ``score_samples`` and ``decision_function`` return float64 [m], numpy for numpy queries and a CUDA tensor for a CUDA tensor, equal to
    scikit-learn's arithmetic on the same trees bit for bit; ``predict`` and ``fit_predict`` return numpy int64 flags, -1 where
    ``decision_function < 0``.  ``get_params`` / ``set_params`` make ``sklearn.base.clone`` work."""

    _who = "IsolationForest"
    _params = ("n_estimators", "max_samples", "contamination", "max_features", "bootstrap", "random_state", "device")

    def __init__(self, *, n_estimators=100, max_samples="auto", contamination="auto", max_features=1.0, bootstrap=False, random_state=None,
                 device="cuda", **other):
        who = self._who
        _tree_host.refuse_non_defaults(who, other, _SKLEARN_DEFAULTS, ignored=("n_jobs", "verbose"))
        if not _is_int(n_estimators) or n_estimators < 1:
            raise ValueError(f"{who}: n_estimators must be an int >= 1, got {n_estimators!r}")
        if n_estimators > MAX_TREES:
            raise ValueError(f"{who}: n_estimators = {n_estimators}, at most {MAX_TREES} trees grow in the one launch")
        if not (isinstance(max_features, numbers.Real) and not isinstance(max_features, bool) and float(max_features) == 1.0 and not _is_int(max_features)):
            raise NotImplementedError(f"{who}: max_features={max_features!r} is not supported (only 1.0: every tree sees every feature)")
        if bootstrap is not False:
            raise NotImplementedError(f"{who}: bootstrap={bootstrap!r} is not supported (only False: a tree's rows are distinct)")
        if not (isinstance(contamination, str) and contamination == "auto"):
            if not isinstance(contamination, numbers.Real) or isinstance(contamination, bool) or not 0.0 < contamination <= 0.5:
                raise ValueError(f"{who}: contamination must be 'auto' or a float in (0, 0.5], got {contamination!r}")
        resolve_max_samples(max_samples, MAX_ROWS, who)          # the type and the range; the value waits for n
        if random_state is not None and not _is_int(random_state):
            raise ValueError(f"{who}: random_state must be an int (the seed is part of the model), got {random_state!r}")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU fallback)")
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.n_estimators, self.max_samples, self.contamination, self.max_features = n_estimators, max_samples, contamination, max_features
        self.bootstrap, self.random_state, self.device = bootstrap, random_state, device

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._params}

    def set_params(self, **params):
        unknown = set(params) - set(self._params)
        if unknown:
            raise ValueError(f"{self._who}: unknown parameters {sorted(unknown)}")
        type(self)(**{**self.get_params(), **params})          # the constructor's checks
        for name, value in params.items():
            setattr(self, name, value)
        return self

    # ---- fit --------------------------------------------------------------------------------------------------------
    def _checked(self, X, sample_weight):
        """(float32 X, max_samples_), validated: no GPU call yet for a numpy input."""
        who = self._who
        if sample_weight is not None:
            raise NotImplementedError(f"{who}: sample_weight is not supported")
        if _is_sparse(X):
            raise NotImplementedError(f"{who}: sparse input is not supported (X must be a dense numpy array or CUDA tensor)")
        if self.random_state is None:
            raise ValueError(f"{who}: random_state must be an int (the seed is part of the model), got None")
        shape = tuple(X.shape) if isinstance(X, torch.Tensor) else np.shape(X)
        if len(shape) == 2 and shape[0] >= 1:                  # the limit comes first: nothing has touched the GPU yet
            S = resolve_max_samples(self.max_samples, shape[0], who)
            if S > MAX_SAMPLES:
                raise ValueError(f"{who}: max_samples = {S} rows per tree, at most {MAX_SAMPLES} are supported (BBBP_IFOREST_MAX_SAMPLES)")
        X32 = _tree_host.training_matrix32(X, who, MAX_ROWS, MAX_FEATURES, "BBBP_IFOREST_MAX")
        return X32, S

    def fit(self, X, y=None, sample_weight=None):
        X32, S = self._checked(X, sample_weight)
        dev = torch.device(self.device)
        with torch.cuda.device(dev):
            Xd = (X32 if isinstance(X32, torch.Tensor) else torch.from_numpy(X32)).to(dev).contiguous()
            trees, samples = _grow(Xd, S, int(self.n_estimators), int(self.random_state))
            self.max_samples_, self._max_samples, self.estimators_samples_ = S, S, samples
            self._set_model(trees, Xd.shape[1])
            if isinstance(self.contamination, str):
                self.offset_ = -0.5
            else:
                self.offset_ = np.percentile(self._scores(Xd), 100.0 * self.contamination)
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, y, sample_weight).predict(X)

    def _set_model(self, trees, n_features):
        trees = {**trees, "value": path_terms(trees)}
        trees = {k: trees[k] for k in _TREE_KEYS}
        _tree_host.check_trees(trees, n_features, "isolation_forest", ("right", "feature", "threshold", "value", "n_node_samples"))
        self.trees_, self.n_features_in_, self.n_estimators_ = trees, int(n_features), len(trees["root"]) - 1
        self._dev = _tree_host.to_device(trees, ("left", "right", "feature", "threshold", "value", "root"), ("threshold", "value"), torch.device(self.device))

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """Adopt a fitted scikit-learn ``IsolationForest`` (``estimators_``, ``_max_samples``, ``offset_``) for scoring only:
        ``score_samples``, ``decision_function`` and ``predict`` equal scikit-learn's bit for bit."""
        who = f"{cls.__name__}.from_sklearn"
        if not all(hasattr(fitted, a) for a in ("estimators_", "_max_samples", "offset_")):
            raise ValueError(f"{who}: a fitted scikit-learn IsolationForest is expected")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: scoring runs on the GPU (no CPU fallback)")
        d = int(fitted.n_features_in_)
        if any(len(f) != d or np.any(np.asarray(f) != np.arange(d)) for f in getattr(fitted, "estimators_features_", ())):
            raise NotImplementedError(f"{who}: max_features={getattr(fitted, 'max_features', None)!r} is not supported (only 1.0: every tree sees every feature)")
        trees, _ = _tree_host.sklearn_trees(list(fitted.estimators_), None, who + ": ")
        self = cls.__new__(cls)
        # the fitting parameters are kept as scikit-learn holds them: an adopted model scores, it is not refitted
        self.n_estimators, self.max_samples, self.contamination = len(fitted.estimators_), fitted.max_samples, fitted.contamination
        self.max_features, self.bootstrap, self.random_state, self.device = 1.0, False, None, device
        self.max_samples_, self._max_samples, self.offset_ = int(fitted.max_samples_), int(fitted._max_samples), fitted.offset_
        self.estimators_samples_ = None
        self._set_model(trees, d)
        return self

    # ---- scoring ----------------------------------------------------------------------------------------------------
    def _path_sums(self, Xq):
        """float64 [m] on the device: every row's sum of path terms over the trees, one launch."""
        m = Xq.shape[0]
        out = torch.empty(m, dtype=torch.float64, device=Xq.device)
        if m == 0:
            return out
        t = self._dev
        with torch.cuda.device(Xq.device):
            _lib.check(_lib.lib().bbbp_iforest_path_sum(_dense.stream(), Xq.data_ptr(), Xq.stride(0), m, Xq.shape[1], t["left"].data_ptr(),
                                                        t["right"].data_ptr(), t["feature"].data_ptr(), t["threshold"].data_ptr(), t["value"].data_ptr(),
                                                        t["root"].data_ptr(), self.n_estimators_, out.data_ptr()), "bbbp_iforest_path_sum")
        return out

    def _scores(self, Xq):
        """numpy float64 [m]: the last step runs on the host, in numpy, whatever the input was."""
        return scores_of_path_sums(self._path_sums(Xq).cpu().numpy(), self.n_estimators_, self._max_samples)

    def _queries(self, X):
        if _is_sparse(X):
            raise NotImplementedError(f"{self._who}: sparse input is not supported (X must be a dense numpy array or CUDA tensor)")
        Xq, was_numpy = _tree_host.query_matrix(self, X, torch.device(self.device), "isolation_forest")
        if not bool(torch.isfinite(Xq).all()):
            raise ValueError(f"{self._who}: X contains NaN, infinity or a value too large for float32")
        return Xq, was_numpy

    def score_samples(self, X):
        """[m] float64: the opposite of the anomaly score of the original paper, the lower the more abnormal."""
        Xq, was_numpy = self._queries(X)
        s = self._scores(Xq)
        return s if was_numpy else torch.from_numpy(s).to(Xq.device)

    def decision_function(self, X):
        """``score_samples(X) - offset_``: negative for outliers."""
        Xq, was_numpy = self._queries(X)
        s = self._scores(Xq) - self.offset_
        return s if was_numpy else torch.from_numpy(s).to(Xq.device)

    def predict(self, X):
        """numpy int64 [m]: -1 where ``decision_function < 0`` (an outlier), else 1."""
        Xq, _ = self._queries(X)
        flags = np.ones(Xq.shape[0], dtype=int)
        flags[self._scores(Xq) - self.offset_ < 0] = -1
        return flags


def _grow(Xd, S, n_trees, seed):
    """``bbbp_iforest_fit`` over X [n, d] float32 on the device: every tree in one launch.  Returns the flat host trees (without ``value``)
    and the trees' rows, int32 [T, S]."""
    L = _lib.lib()
    dev = Xd.device
    n, d = Xd.shape
    cap = L.bbbp_iforest_tree_capacity(S)
    if not cap:
        raise ValueError("isolation_forest: " + L.bbbp_last_error().decode("utf-8", "replace"))
    i32 = lambda: torch.empty((n_trees, cap), dtype=torch.int32, device=dev)  # noqa: E731
    left, right, feature, nns = i32(), i32(), i32(), i32()
    threshold = torch.empty((n_trees, cap), dtype=torch.float64, device=dev)
    samples = torch.empty((n_trees, S), dtype=torch.int32, device=dev)
    n_nodes = torch.empty(n_trees, dtype=torch.int32, device=dev)
    _lib.check(L.bbbp_iforest_fit(_dense.stream(), Xd.data_ptr(), Xd.stride(0), n, d, S, n_trees, seed & ((1 << 64) - 1), left.data_ptr(),
                                  right.data_ptr(), feature.data_ptr(), nns.data_ptr(), threshold.data_ptr(), samples.data_ptr(),
                                  n_nodes.data_ptr()), "bbbp_iforest_fit")
    _GROWN["launches"] += 1
    counts_d = n_nodes.to(torch.int64)
    counts = counts_d.cpu().numpy()
    if (counts < 1).any():
        raise RuntimeError(f"isolation_forest: the fit kernel reported an index outside its array in tree {int(np.argmax(counts < 1))} "
                           "(a defect of csrc/iforest.hip, not of the data); no model is returned")
    keep = torch.arange(cap, device=dev)[None, :] < counts_d[:, None]
    l, r, f, m, thr = (a[keep].cpu().numpy() for a in (left, right, feature, nns, threshold))      # only the slots in use cross the bus
    root = np.concatenate([[0], np.cumsum(counts)])
    l, r = _tree_host.rebase_children(l, r, np.repeat(root[:-1], counts))
    return dict(left=l, right=r, feature=f, threshold=thr, n_node_samples=m, root=root.astype(np.int32)), samples.cpu().numpy()
