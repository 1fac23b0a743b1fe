"""``sklearn.ensemble.RandomForestClassifier`` and ``sklearn.tree.DecisionTreeClassifier`` for the GPU: two classes, Gini, exact-split
trees of any depth fitted level by level, many trees in one batch.

The classification stack of the reference (``Models/model_opt_maccs.py:124-200``) searches ``RandomForestClassifier`` over
``n_estimators in {50, 100, 200, 300}``, ``max_depth in {None, 10, 20, 30}``, ``min_samples_split in {2, 5, 10}`` and ``min_samples_leaf in
{1, 2, 4}`` under ``GridSearchCV(cv=5, scoring='f1')`` -- 720 forests, about 117 000 trees on about 5 100 rows of 100 features -- and a
``DecisionTreeClassifier``, the one-tree case without bootstrap and with all features.  The entry points of ``csrc/rf.hip`` carry both:

* a training matrix is cast to float32 (scikit-learn's trees compare float32 features), transposed and every column's rows are sorted
  stably once (``_tree_host.Matrix``); all trees over that matrix share both;
* ``bbbp_rf_fit`` grows any number of trees side by side, one level per round of six launches; the host reads one word per eight levels;
* ``bbbp_rf_predict_proba`` walks query rows through the trees in tree order with scikit-learn's forest arithmetic, optionally stopping
  at limits ``(n_trees, max_depth, min_samples_split)``.

The rules are scikit-learn 1.7's (``ensemble/_forest.py``, ``tree/_splitter.pyx``, ``_criterion.pyx``).  A tree's bootstrap is a vector of
integer row weights; ``n_node_samples`` and the ``min_samples_*`` rules count distinct rows, class totals use the weights.  With two
classes the Gini proxy orders candidates like ``(W_R L_1 - W_L R_1)^2 / (W_L W_R)``: exact integers and one float64 division, so a fit has
no summation order and ``tests/rf_numpy.py`` reproduces it bit for bit.  scikit-learn's per-tree random stream cannot be matched: here
every random choice is one counter-based hash (``bbbp_rf_hash``) of the seed, the tree's number and the node's path, which makes
``random_state`` part of the model and has a structural consequence: a subtree depends on its rows, ``min_samples_leaf``, ``max_features``
and its path alone, so a tree under a larger ``min_samples_split`` or a smaller ``max_depth`` is the pruning of the unlimited tree, and a
forest of fewer trees is a prefix.  ``grid_search_cv`` grows one forest per fold and distinct ``(min_samples_leaf, max_features)`` and scores
every other grid point with the predict kernel's limits.  Among equal scores the lowest feature wins, then the lowest position; trees are
certified (``tests/rf_replay.py``), not compared with scikit-learn's.

A tree's probabilities are scikit-learn 1.7's: the leaf's stored class shares ``value`` (already divided by the node's weight when the
tree was built; ``tree_.predict`` returns them as they are), summed over trees in tree order in float64 and divided by the number of trees.

Out of scope for the classifiers (each is refused by name): more than two classes, ``criterion != "gini"``, ``sample_weight``,
``class_weight``, ``max_samples``, ``max_leaf_nodes``, ``ccp_alpha``, ``min_impurity_decrease != 0``, fractional ``min_samples_*``,
``oob_score``, more than 8 192 rows or 1 024 features, more than one GPU.  There is no CPU path.

``RandomForestRegressor`` and ``DecisionTreeRegressor`` are the logBB stack's forest
(``Models/multi_input_data_regression_opt_transformer_cnn_opt.py:163-165``: ``RandomForestRegressor(n_estimators=300, max_depth=15,
random_state=42)`` on the 64 + 128 PCA features, five folds; ``..._20250113.py:394-403`` refits it six times inside ``StackingRegressor``)
under the squared-error criterion.  They grow through the same rounds (``bbbp_rf_fit_regression``): the targets are rounded once to a
dyadic grid 49 bits below the binade of ``max |y|`` so that a node's sums are exact 64-bit integers, a candidate's score is scikit-learn's
proxy ``S_L^2 / W_L + S_R^2 / W_R`` on those sums in seven float64 roundings, and ``tests/rfr_numpy.py`` reproduces a fit bit for bit.
``fit_regressors`` grows the forests of many ``(X, y)`` problems, the folds and the stacker's refits, in one batch;
``bbbp_rf_predict_mean`` predicts.  The regressors' docstring lists what they refuse.

The training matrix (``Matrix``), the input checks, the flattening of scikit-learn's trees and the small uploads are shared with
``gradient_boosting`` and live in ``_tree_host.py``; the kernels' shared device code is ``csrc/tree_fit.h``.  ``isolation_forest`` draws
from the same hash under a key tag of its own.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _estimator, _dense, _lib, _tree_host
from ._tree_host import Matrix as _Matrix, is_int as _is_int          # shared with gradient_boosting: they live in _tree_host.py
from .linear_model import _binary_targets

MAX_ROWS, MAX_FEATURES = 8192, 1024                # BBBP_RF_FIT_MAX_N, BBBP_RF_FIT_MAX_D
UNLIMITED = 1 << 30                                # max_depth=None for the kernels: depth is limited by the rows alone
MEMORY_BUDGET = 8 << 30                            # bytes of work areas and node slots one batch of trees may take
GRID_KEYS = ("n_estimators", "max_depth", "min_samples_split", "min_samples_leaf", "max_features")
_SKLEARN_DEFAULTS = dict(criterion="gini", class_weight=None, max_samples=None, max_leaf_nodes=None, ccp_alpha=0.0, min_impurity_decrease=0.0,
                         oob_score=False, min_weight_fraction_leaf=0.0, warm_start=False, n_jobs=None, verbose=0, monotonic_cst=None, splitter="best")
_TREE_KEYS = ("left", "right", "feature", "threshold", "value", "n_node_samples", "root")


def _resolve_max_features(max_features, d, who):
    """scikit-learn's ``max_features_`` for "sqrt", "log2", None or an int."""
    if max_features is None:
        return d
    if isinstance(max_features, str):
        if max_features == "sqrt":
            return max(1, int(np.sqrt(d)))
        if max_features == "log2":
            return max(1, int(np.log2(d)))
        raise ValueError(f"{who}: max_features must be 'sqrt', 'log2', None or an int, got {max_features!r}")
    if not 1 <= max_features <= d:
        raise ValueError(f"{who}: max_features = {max_features} outside 1..{d}")
    return int(max_features)


def _check_params(n_estimators, max_depth, min_samples_split, min_samples_leaf, max_features, who="RandomForestClassifier"):
    if not _is_int(n_estimators) or n_estimators < 1:
        raise ValueError(f"{who}: n_estimators must be an int >= 1, got {n_estimators!r}")
    if max_depth is not None and (not _is_int(max_depth) or max_depth < 1):
        raise ValueError(f"{who}: max_depth must be None or an int >= 1, got {max_depth!r}")
    if not _is_int(min_samples_split):
        raise NotImplementedError(f"{who}: min_samples_split must be an int >= 2 (fractions are not supported), got {min_samples_split!r}")
    if min_samples_split < 2:
        raise ValueError(f"{who}: min_samples_split must be an int >= 2, got {min_samples_split!r}")
    if not _is_int(min_samples_leaf):
        raise NotImplementedError(f"{who}: min_samples_leaf must be an int >= 1 (fractions are not supported), got {min_samples_leaf!r}")
    if min_samples_leaf < 1:
        raise ValueError(f"{who}: min_samples_leaf must be an int >= 1, got {min_samples_leaf!r}")
    if isinstance(max_features, str) or max_features is None:
        _resolve_max_features(max_features, 1, who)
    elif not _is_int(max_features):
        raise NotImplementedError(f"{who}: max_features must be 'sqrt', 'log2', None or an int (fractions are not supported), got {max_features!r}")
    elif max_features < 1:
        raise ValueError(f"{who}: max_features must be >= 1, got {max_features!r}")


def _training_matrix32(X, who):
    return _tree_host.training_matrix32(X, who, MAX_ROWS, MAX_FEATURES, "BBBP_RF_FIT_MAX")


class _Spec:
    """One forest to grow: ``n_trees`` trees (numbers 0 .. n_trees - 1) over one matrix under one set of parameters.  ``t_d`` holds the class
    indicator 0.0 / 1.0, or with ``regression`` the integer targets ``q`` of ``_quantise``, as float64 on the device."""

    def __init__(self, mat, t_d, n_trees, max_depth, min_samples_split, min_samples_leaf, max_features, bootstrap, seed, regression=False):
        self.mat, self.t, self.T, self.regression = mat, t_d, int(n_trees), bool(regression)
        self.max_depth = UNLIMITED if max_depth is None else int(max_depth)
        self.mss, self.msl, self.mf, self.bootstrap = int(min_samples_split), int(min_samples_leaf), int(max_features), bool(bootstrap)
        self.seed = int(seed) & ((1 << 64) - 1)
        L = _lib.lib()
        self.work_bytes = (L.bbbp_rf_fit_regression_work_bytes if self.regression else L.bbbp_rf_fit_work_bytes)(mat.n, mat.d, self.mf)
        self.cap = L.bbbp_rf_fit_tree_capacity(mat.n)
        if not self.work_bytes or not self.cap:
            raise ValueError("random_forest: " + L.bbbp_last_error().decode("utf-8", "replace"))
        self.trees = None                          # the flat host arrays, set by _grow


_GROWN = {"trees": 0}                              # trees grown by this process (tests count them)


def _grow(specs, budget=None):
    """``bbbp_rf_fit`` (``bbbp_rf_fit_regression`` for regression specs; one call grows one kind) over every tree of every spec, in batches
    whose work areas and node slots fit ``budget`` bytes.  Sets ``spec.trees``: the flat host arrays in ``ForestGPU.flatten_sklearn``'s
    convention plus ``n_node_samples`` and the private ``value0`` (the class-0 share; a regression node's weight)."""
    budget = MEMORY_BUDGET if budget is None else int(budget)
    regression = specs[0].regression
    if any(s.regression != regression for s in specs):
        raise ValueError("random_forest: classification and regression forests cannot grow in one batch")
    fit_name = "bbbp_rf_fit_regression" if regression else "bbbp_rf_fit"
    dev = specs[0].mat.XT.device
    L = _lib.lib()
    todo = [(si, t) for si, s in enumerate(specs) for t in range(s.T)]
    per_tree = max(s.work_bytes + s.cap * 40 for s in specs)
    batch = int(max(1, min(65535, budget // per_tree)))
    parts = {si: [] for si in range(len(specs))}
    for lo in range(0, len(todo), batch):
        chunk = todo[lo:lo + batch]
        B = len(chunk)
        cap = max(specs[si].cap for si, _ in chunk)
        wb = max(specs[si].work_bytes for si, _ in chunk)
        work = torch.empty(B * wb, dtype=torch.uint8, device=dev)
        i32 = lambda: torch.empty((B, cap), dtype=torch.int32, device=dev)  # noqa: E731
        f64 = lambda: torch.empty((B, cap), dtype=torch.float64, device=dev)  # noqa: E731
        left, right, feature, nns, threshold, value, value0 = i32(), i32(), i32(), i32(), f64(), f64(), f64()
        n_nodes = torch.empty(B, dtype=torch.int32, device=dev)
        alive = torch.empty(1, dtype=torch.int32, device=dev)
        descs = []
        for b, (si, t) in enumerate(chunk):
            s = specs[si]
            descs.append(_lib.RfTree(s.mat.XT.data_ptr(), s.mat.order0.data_ptr(), s.t.data_ptr(), s.mat.n, s.mat.d, s.max_depth, s.mss, s.msl, s.mf,
                                     int(s.bootstrap), t, s.seed, work.data_ptr() + b * wb, left.data_ptr() + 4 * b * cap, right.data_ptr() + 4 * b * cap,
                                     feature.data_ptr() + 4 * b * cap, nns.data_ptr() + 4 * b * cap, threshold.data_ptr() + 8 * b * cap,
                                     value.data_ptr() + 8 * b * cap, value0.data_ptr() + 8 * b * cap, n_nodes.data_ptr() + 4 * b))
        arr = (_lib.RfTree * B)(*descs)
        on_device = _tree_host.upload(arr, dev)
        _lib.check(getattr(L, fit_name)(_dense.stream(), arr, on_device.data_ptr(), B, alive.data_ptr()), fit_name)
        _GROWN["trees"] += B
        counts_d = n_nodes.to(torch.int64)
        counts = counts_d.cpu().numpy()
        if (counts < 1).any():
            bad = chunk[int(np.argmax(counts < 1))]
            raise RuntimeError(f"random_forest: the fit kernels reported an index outside its array in tree {bad[1]} (a defect of csrc/rf.hip, "
                               "not of the data); no model is returned")
        keep = torch.arange(cap, device=dev)[None, :] < counts_d[:, None]
        host = [a[keep].cpu().numpy() for a in (left, right, feature, nns, threshold, value, value0)]      # only the slots in use cross the bus
        ends = np.cumsum(counts)
        for b, (si, t) in enumerate(chunk):
            parts[si].append([a[ends[b] - counts[b]:ends[b]] for a in host])
        del work, on_device
    for si, s in enumerate(specs):
        counts = np.array([len(p[0]) for p in parts[si]], dtype=np.int64)
        root = np.concatenate([[0], np.cumsum(counts)])
        cat = lambda i: np.concatenate([p[i] for p in parts[si]])  # noqa: E731
        left, right = _tree_host.rebase_children(cat(0), cat(1), np.repeat(root[:-1], counts))
        s.trees = dict(left=left, right=right, feature=cat(2), threshold=cat(4), value=cat(5), n_node_samples=cat(3), root=root.astype(np.int32),
                       value0=cat(6))


def _prune(trees, n_trees, max_depth, min_samples_split):
    """The first ``n_trees`` trees as they grow under ``max_depth`` and ``min_samples_split``: a node at that depth or with fewer rows becomes a
    leaf, what hangs below it goes, and the nodes are numbered level by level again."""
    depth_limit = UNLIMITED if max_depth is None else int(max_depth)
    left, right, root = trees["left"], trees["right"], trees["root"]
    out = {k: [] for k in trees if k != "root"}
    new_root = [0]
    for t in range(n_trees):
        level, depth, olds, lefts, rights = np.array([int(root[t])]), 0, [], [], []
        at = new_root[-1]
        while len(level):
            split = (left[level] >= 0) & (trees["n_node_samples"][level] >= min_samples_split) & (depth < depth_limit)
            first = at + len(level) + 2 * np.cumsum(split) - 2 * split           # the left child's new number
            olds.append(level)
            lefts.append(np.where(split, first, -1))
            rights.append(np.where(split, first + 1, -1))
            at += len(level)
            level = np.stack([left[level[split]], right[level[split]]], axis=1).ravel()
            depth += 1
        old, nl = np.concatenate(olds), np.concatenate(lefts)
        leaf = nl < 0
        out["left"].append(nl.astype(np.int32))
        out["right"].append(np.concatenate(rights).astype(np.int32))
        out["feature"].append(np.where(leaf, 0, trees["feature"][old]).astype(np.int32))
        out["threshold"].append(np.where(leaf, -2.0, trees["threshold"][old]))
        for k in out:
            if k not in ("left", "right", "feature", "threshold"):
                out[k].append(trees[k][old])
        new_root.append(at)
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["root"] = np.asarray(new_root, dtype=np.int32)
    return res


def _limited(spec, limits, who):
    """A grown forest's trees, or with ``limits = (n_estimators, max_depth, min_samples_split)`` their view under those limits, pruned and
    renumbered: what a single fit with those parameters gives."""
    if limits is None:
        return spec.trees
    T, depth, mss = limits
    if T > spec.T or mss < spec.mss or (UNLIMITED if depth is None else depth) > spec.max_depth:
        raise ValueError(f"{who}: limits {limits} ask for more than the forest was grown with")
    return _prune(spec.trees, int(T), depth, int(mss))


def _check_trees(trees, n_features):
    _tree_host.check_trees(trees, n_features, "random_forest", ("right", "feature", "threshold", "value", "n_node_samples"))


def _flat_sklearn(fitted, value_columns, who):
    """A fitted scikit-learn forest's or single tree's trees as flat trees without ``value``, the values asked for, and the number of trees."""
    ests = list(fitted.estimators_) if hasattr(fitted, "estimators_") else [fitted]
    return _tree_host.sklearn_trees(ests, value_columns, who + ": ") + (len(ests),)


class RandomForestClassifier(_estimator.Params):
    """``RandomForestClassifier(n_estimators=100, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features="sqrt",
    bootstrap=True, random_state=0, device="cuda")``: scikit-learn's names for two classes and the Gini criterion.

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (n <= 8 192, d <= 1 024; cast to float32, as scikit-learn's trees do) and labels with
    two distinct values.  It sets ``classes_``, ``n_features_in_``, ``n_estimators_`` and ``trees_``: ``left``, ``right``, ``feature``, float64
    ``threshold``, ``value`` (the weighted share of ``classes_[1]`` in every node, inner nodes included), ``n_node_samples`` (distinct rows)
    and ``root`` in ``ForestGPU.flatten_sklearn``'s convention, nodes numbered level by level.  ``random_state`` must be an int: without the
    tie-breaking that scikit-learn's generator provides, the seed is part of the model.  ``predict_proba`` returns float64 [m, 2] (numpy for
    numpy input, a CUDA tensor for a CUDA tensor); ``predict`` takes the larger probability, ties to ``classes_[0]``."""

    _who = "RandomForestClassifier"

    def __init__(self, n_estimators=100, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features="sqrt", bootstrap=True,
                 random_state=0, device="cuda", **other):
        who = self._who
        _tree_host.refuse_non_defaults(who, other, _SKLEARN_DEFAULTS)
        _check_params(n_estimators, max_depth, min_samples_split, min_samples_leaf, max_features, who)
        if not _is_int(random_state):
            raise ValueError(f"{who}: random_state must be an int (the seed is part of the model), got {random_state!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU fallback)")
        self.n_estimators, self.max_depth = int(n_estimators), None if max_depth is None else int(max_depth)
        self.min_samples_split, self.min_samples_leaf, self.max_features = int(min_samples_split), int(min_samples_leaf), max_features
        self.bootstrap, self.random_state = bool(bootstrap), int(random_state)

    _params = ("n_estimators", "max_depth", "min_samples_split", "min_samples_leaf", "max_features", "bootstrap", "random_state", "device")

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError(f"{self._who}: sample_weight is not supported")
        _fit_classifiers([self], [(X, y)])
        return self

    def _adopt(self, classes, spec, limits=None):
        """Fitted attributes from a grown forest.  ``limits = (n_estimators, max_depth, min_samples_split)`` materialises the view of the
        forest under those limits, pruned and renumbered: the model a single fit with those parameters gives."""
        trees = _limited(spec, limits, self._who)
        self._set_model(classes, {k: trees[k] for k in _TREE_KEYS}, trees["value0"], trees["value"], spec.mat.d)

    def _set_model(self, classes, trees, p0, p1, n_features):
        _check_trees(trees, n_features)
        self.classes_, self.trees_, self.n_features_in_ = classes, trees, int(n_features)
        self.n_estimators_ = len(trees["root"]) - 1
        self._dev = _tree_host.to_device({**trees, "p0": p0, "p1": p1}, ("left", "right", "feature", "threshold", "n_node_samples", "root", "p0", "p1"),
                                         ("threshold", "p0", "p1"), self.device)

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """Adopt a fitted scikit-learn ``RandomForestClassifier``, ``ExtraTreesClassifier`` or ``DecisionTreeClassifier`` (two classes, one
        output) for prediction only: ``predict_proba`` equals scikit-learn's (fitted with ``n_jobs=None``) bit for bit."""
        who = f"{cls.__name__}.from_sklearn"
        if getattr(fitted, "n_outputs_", 1) != 1 or np.ndim(getattr(fitted, "n_classes_", 0)) != 0 or int(fitted.n_classes_) != 2:
            raise ValueError(f"{who}: exactly two classes and one output are supported")
        trees, (p0, p1), n_trees = _flat_sklearn(fitted, (0, 1), who)
        self = cls.__new__(cls)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: prediction runs on the GPU (no CPU fallback)")
        # the fitting parameters are kept only where this class would accept them: an adopted model predicts, it is not refitted
        self.n_estimators = n_trees
        for name in ("max_depth", "min_samples_split", "min_samples_leaf", "max_features"):
            v = getattr(fitted, name, None)
            setattr(self, name, v if (_is_int(v) or (name == "max_features" and isinstance(v, str))) else None)
        self.bootstrap, self.random_state = bool(getattr(fitted, "bootstrap", False)), None
        self._set_model(np.asarray(fitted.classes_), {**trees, "value": p1}, p0, p1, int(fitted.n_features_in_))
        return self

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _queries(self, X):
        return _tree_host.query_matrix(self, X, self.device, "random_forest")

    def _proba(self, Xq, limits=None):
        """float64 [m, 2] on the device; ``limits = (n_estimators, max_depth, min_samples_split)`` stops every walk as a fit under them would."""
        m = Xq.shape[0]
        out = torch.empty((m, 2), dtype=torch.float64, device=self.device)
        if m == 0:
            return out
        T, depth, mss = (self.n_estimators_, None, 0) if limits is None else limits
        if not 1 <= T <= self.n_estimators_:
            raise ValueError(f"random_forest: {T} trees asked of a forest of {self.n_estimators_}")
        t = self._dev
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bbbp_rf_predict_proba(_dense.stream(), Xq.data_ptr(), Xq.shape[1], m, Xq.shape[1], t["left"].data_ptr(),
                                                        t["right"].data_ptr(), t["feature"].data_ptr(), t["threshold"].data_ptr(), t["p0"].data_ptr(),
                                                        t["p1"].data_ptr(), t["n_node_samples"].data_ptr(), t["root"].data_ptr(), int(T),
                                                        UNLIMITED if depth is None else int(depth), int(mss), out.data_ptr()), "bbbp_rf_predict_proba")
        return out

    def predict_proba(self, X):
        """[m, 2]: the trees' class shares at the leaves, summed in tree order and divided by the number of trees."""
        Xq, was_numpy = self._queries(X)
        out = self._proba(Xq)
        return out.cpu().numpy() if was_numpy else out

    def predict_log_proba(self, X):
        """log of ``predict_proba`` (scikit-learn's: -inf where a probability is 0)."""
        Xq, was_numpy = self._queries(X)
        out = self._proba(Xq)
        if not was_numpy:
            return torch.log(out)
        with np.errstate(divide="ignore"):
            return np.log(out.cpu().numpy())

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype: the larger probability, ties to ``classes_[0]`` (scikit-learn's argmax)."""
        Xq, _ = self._queries(X)
        p = self._proba(Xq)
        return self.classes_[(p[:, 1] > p[:, 0]).cpu().numpy().astype(np.intp)]


class DecisionTreeClassifier(RandomForestClassifier):
    """``DecisionTreeClassifier(*, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, bootstrap=False,
    random_state=0, device="cuda")``: the same fit with one tree, every row once and all features at every node."""

    _who = "DecisionTreeClassifier"
    _params = RandomForestClassifier._params[1:]

    def __init__(self, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, bootstrap=False, random_state=0, device="cuda",
                 **other):
        super().__init__(1, max_depth=max_depth, min_samples_split=min_samples_split, min_samples_leaf=min_samples_leaf, max_features=max_features,
                         bootstrap=bootstrap, random_state=random_state, device=device, **other)


def _fit_classifiers(classifiers, problems):
    """Grow the forests of ``classifiers[i]`` over ``problems[i] = (X, y)`` in one ``_grow`` call and fit every classifier from its own: what
    ``fit`` does, for one or many (``ensemble`` fits a learner on all rows and on every fold's training rows this way).  Each classifier
    equals its single ``fit`` bit for bit."""
    checked = []
    for clf, (X, y) in zip(classifiers, problems):
        who = clf._who
        classes, t = _binary_targets(y, None, who)
        X32 = _training_matrix32(X, who)
        if X32.shape[0] != len(t):
            raise ValueError(f"{who}: X has {X32.shape[0]} rows, y has {len(t)}")
        checked.append((classes, t, X32, _resolve_max_features(clf.max_features, X32.shape[1], who)))
    with torch.cuda.device(classifiers[0].device):
        specs = [_Spec(_Matrix(X32, clf.device), torch.from_numpy(t).to(clf.device), clf.n_estimators, clf.max_depth, clf.min_samples_split,
                       clf.min_samples_leaf, mf, clf.bootstrap, clf.random_state) for clf, (_, t, X32, mf) in zip(classifiers, checked)]
        _grow(specs)
        for clf, spec, (classes, _, _, _) in zip(classifiers, specs, checked):
            clf._adopt(classes, spec)


def grid_points(param_grid, who="random_forest.grid_search_cv"):
    """The grid's points in scikit-learn's order (sorted keys, ``itertools.product``; a list of grids one after the other) and each point's
    full parameter tuple in ``GRID_KEYS``' order, checked."""
    defaults = dict(n_estimators=100, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features="sqrt")
    return _tree_host.grid_points(param_grid, GRID_KEYS, defaults, _check_params, who)


def _cv_forests(X32, t_all, folds, full, dev, random_state=0):
    """One forest per (fold, distinct (min_samples_leaf, max_features)), grown with the largest ``n_estimators``, the smallest
    ``min_samples_split`` and the largest ``max_depth`` asked of it, all in one call of ``_grow``.  Returns ({(fold, (min_samples_leaf,
    max_features)): spec}, the folds' test rows on the device)."""
    widest = {}
    for T, depth, mss, msl, mf in full:
        depth = UNLIMITED if depth is None else depth
        old = widest.get((msl, mf), (0, 0, 1 << 30))
        widest[(msl, mf)] = (max(old[0], T), max(old[1], depth), min(old[2], mss))
    specs, queries = {}, []
    for fi, (tr, te) in enumerate(folds):
        mat = _Matrix(X32[tr], dev)
        t_d = torch.from_numpy(t_all[tr]).to(dev)
        queries.append(torch.from_numpy(X32[te]).to(dev))
        for (msl, mf), (T, depth, mss) in widest.items():
            specs[(fi, (msl, mf))] = _Spec(mat, t_d, T, None if depth >= UNLIMITED else depth, mss, msl,
                                           _resolve_max_features(mf, mat.d, "random_forest.grid_search_cv"), True, random_state)
    _grow(list(specs.values()))
    return specs, queries


def grid_search_cv(X, y, param_grid, cv: int = 5, device="cuda", random_state=0):
    """The reference's ``GridSearchCV(RandomForestClassifier(), param_grid, cv=5, scoring='f1')`` (model_opt_maccs.py:124-200) over
    ``n_estimators``, ``max_depth`` (None allowed), ``min_samples_split``, ``min_samples_leaf`` and ``max_features``.

    Same conventions as ``gradient_boosting.grid_search_cv``: sorted keys, ``itertools.product`` order, scikit-learn's
    ``StratifiedKFold(cv)``, ``f1_score`` of ``classes_[1]``, the first maximum wins.  Every fold grows one forest per distinct
    (min_samples_leaf, max_features); every grid point is that forest seen through the predict kernel's limits and equals a single ``fit``
    on that fold bit for bit; the refit on all rows follows.  Returns (best_params, mean F1 per point, the refitted classifier)."""
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    who = "random_forest.grid_search_cv"
    points, full = grid_points(param_grid, who)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU fallback)")
    X = np.asarray(X)
    y = np.asarray(y)
    classes, t_all = _binary_targets(y, X.shape[0] if X.ndim == 2 else None, who)
    X32 = _training_matrix32(X, who)
    pos = classes[1]
    folds = list(StratifiedKFold(n_splits=cv).split(X32, y))
    f1 = np.zeros((len(points), len(folds)))
    with torch.cuda.device(dev):
        specs, queries = _cv_forests(X32, t_all, folds, full, dev, random_state)
        for (fi, group), spec in specs.items():
            big = RandomForestClassifier(spec.T, min_samples_leaf=group[0], max_features=group[1], random_state=random_state, device=dev)
            big._adopt(classes, spec)
            seen = {}
            for pi, params in enumerate(full):
                if params[3:] != group:
                    continue
                if params[:3] not in seen:
                    p = big._proba(queries[fi], params[:3])
                    seen[params[:3]] = classes[(p[:, 1] > p[:, 0]).cpu().numpy().astype(np.intp)]
                f1[pi, fi] = f1_score(y[folds[fi][1]], seen[params[:3]], pos_label=pos)
        del specs, queries
    scores = [float(v) for v in f1.mean(axis=1)]
    best = int(np.argmax(scores))
    T, depth, mss, msl, mf = full[best]
    fitted = RandomForestClassifier(T, max_depth=depth, min_samples_split=mss, min_samples_leaf=msl, max_features=mf, random_state=random_state,
                                    device=dev).fit(X32, y)
    return points[best], scores, fitted


# ---- regression: RandomForestRegressor and DecisionTreeRegressor under the squared-error criterion ---------------------------------------
TARGET_BITS = 49                                   # |q| <= 2^49: with weights summing to n <= 2^13 every sum of w q stays within 2^62
_REGRESSOR_DEFAULTS = dict(criterion="squared_error", max_samples=None, max_leaf_nodes=None, ccp_alpha=0.0, min_impurity_decrease=0.0, oob_score=False,
                           min_weight_fraction_leaf=0.0, warm_start=False, n_jobs=None, verbose=0, monotonic_cst=None, splitter="best")


def _quantise(y, n_rows, who):
    """The targets on their dyadic grid: (q, s) with ``q = rint(y 2^s)`` (integers held in float64, ``|q| <= 2^TARGET_BITS``) and
    ``s = TARGET_BITS - e``, ``(_, e) = frexp(max |y|)``; ``s = 0`` when all of y is 0."""
    y = _tree_host.targets_1d(y, n_rows, who, "multi-output targets are not supported")
    top = float(np.abs(y).max())
    s = 0 if top == 0.0 else TARGET_BITS - int(np.frexp(top)[1])
    return np.rint(np.ldexp(y, s)), s


class RandomForestRegressor:
    """``RandomForestRegressor(n_estimators=100, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=1.0, bootstrap=True,
    random_state=0, device="cuda")``: scikit-learn's names for one output and the squared-error criterion -- the reference's
    ``RandomForestRegressor(n_estimators=300, max_depth=15, random_state=42)`` (Models/multi_input_data_regression_opt_transformer_cnn_opt.py:163-165).

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (n <= 8 192, d <= 1 024; cast to float32) and finite float64 targets [n].  The targets
    are rounded once to a dyadic grid, ``y_hat = rint(y 2^s) 2^-s`` with ``2^-s = y_quantum_`` (49 bits below the binade of ``max |y|``: within
    ``2^-50 2^e`` of y, 7e-15 for ``|y| < 8``), and the model is by definition scikit-learn's tree on ``(X, y_hat)``: every node's sums are
    exact integers, a candidate's score is ``S_L S_L / W_L + S_R S_R / W_R`` in seven float64 roundings, so a fit has no summation order,
    ``tests/rfr_numpy.py`` reproduces it bit for bit, and a tree is the same alone, in any batch and run to run.  A node is pure when all its
    targets are one grid point (scikit-learn: ``impurity <= 2.2e-16``; the rules differ only for nodes whose spread is below about 1e-8).
    The bootstrap, the per-node feature draw, the valid positions, the thresholds, the tie rule and the numbering are the classifier's, and so
    are the pruning and prefix properties.  ``max_features`` takes 1.0 or None (all features), "sqrt", "log2" or an int.

    Sets ``n_features_in_``, ``n_estimators_``, ``y_quantum_``, ``trees_`` (``value`` the node mean of ``y_hat``, ``n_node_samples`` distinct
    rows) and ``weighted_n_node_samples_``.  ``predict`` is scikit-learn's: leaf values summed in tree order in float64, divided by the number
    of trees; float64 numpy for numpy queries, a CUDA tensor for a CUDA tensor.  ``get_params`` / ``set_params`` make ``sklearn.base.clone``
    work, so ``ensemble.StackingRegressor`` takes this class as a base learner.

    Out of scope, each refused with a message: more than 1 024 features (the reference's raw [N, 49 319] hstack needs a work layout without
    a per-tree copy of every column's order), ``criterion != "squared_error"``, ``sample_weight``, ``oob_score``, ``max_samples``,
    multi-output targets, ``feature_importances_``.  There is no regressor grid search (the reference has none) and no CPU path."""

    _who = "RandomForestRegressor"
    _params = ("n_estimators", "max_depth", "min_samples_split", "min_samples_leaf", "max_features", "bootstrap", "random_state", "device")

    def __init__(self, n_estimators=100, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=1.0, bootstrap=True,
                 random_state=0, device="cuda", **other):
        who = self._who
        _tree_host.refuse_non_defaults(who, other, _REGRESSOR_DEFAULTS)
        _check_params(n_estimators, max_depth, min_samples_split, min_samples_leaf, self._all_features(max_features), who)
        if not _is_int(random_state):
            raise ValueError(f"{who}: random_state must be an int (the seed is part of the model), got {random_state!r}")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU fallback)")
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.n_estimators, self.max_depth, self.min_samples_split, self.min_samples_leaf = n_estimators, max_depth, min_samples_split, min_samples_leaf
        self.max_features, self.bootstrap, self.random_state, self.device = max_features, bootstrap, random_state, device

    @staticmethod
    def _all_features(max_features):
        """scikit-learn's regressor default ``max_features=1.0`` means every feature, like None."""
        return None if isinstance(max_features, float) and max_features == 1.0 else max_features

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

    def __getattr__(self, name):
        if name in ("feature_importances_", "oob_score_", "oob_prediction_"):
            raise AttributeError(f"{self._who}: {name} is not supported")
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError(f"{self._who}: sample_weight is not supported")
        _fit_regressors([self], [(X, y)])
        return self

    def _checked(self, X, y):
        """(float32 X, the integer targets, the grid's exponent, max_features as a count), validated: no GPU call yet."""
        who = self._who
        X32 = _training_matrix32(X, who)
        q, s = _quantise(y, X32.shape[0], who)
        return X32, q, s, _resolve_max_features(self._all_features(self.max_features), X32.shape[1], who)

    def _spec(self, X32, q, mf):
        """The forest this regressor asks for, not yet grown."""
        dev = torch.device(self.device)
        return _Spec(_Matrix(X32, dev), torch.from_numpy(q).to(dev), self.n_estimators, self.max_depth, self.min_samples_split, self.min_samples_leaf,
                     mf, self.bootstrap, self.random_state, regression=True)

    def _adopt(self, spec, s, limits=None):
        """Fitted attributes from a grown forest whose values are in units of ``2^-s``; ``limits`` as ``RandomForestClassifier._adopt``."""
        trees = _limited(spec, limits, self._who)
        model = {k: trees[k] for k in _TREE_KEYS}
        model["value"] = np.ldexp(trees["value"], -s)          # an exact power of two
        self._set_model(model, spec.mat.d)
        self.y_quantum_, self.weighted_n_node_samples_ = float(np.ldexp(1.0, -s)), trees["value0"]

    def _set_model(self, trees, n_features):
        _check_trees(trees, n_features)
        self.trees_, self.n_features_in_, self.n_estimators_ = trees, int(n_features), len(trees["root"]) - 1
        self._dev = _tree_host.to_device(trees, _TREE_KEYS, ("threshold", "value"), torch.device(self.device))

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """Adopt a fitted scikit-learn ``RandomForestRegressor``, ``ExtraTreesRegressor`` or ``DecisionTreeRegressor`` (one output) for
        prediction only: ``predict`` equals scikit-learn's (fitted with ``n_jobs=None``) bit for bit."""
        who = f"{cls.__name__}.from_sklearn"
        if hasattr(fitted, "classes_") or getattr(fitted, "n_outputs_", 1) != 1:
            raise ValueError(f"{who}: a fitted regressor with one output is expected")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: prediction runs on the GPU (no CPU fallback)")
        trees, (value,), n_trees = _flat_sklearn(fitted, (0,), who)
        self = cls.__new__(cls)
        # the fitting parameters are kept only where this class would accept them: an adopted model predicts, it is not refitted
        self.n_estimators, self.device = n_trees, device
        for name in ("max_depth", "min_samples_split", "min_samples_leaf", "max_features"):
            v = getattr(fitted, name, None)
            setattr(self, name, v if (_is_int(v) or (name == "max_features" and (isinstance(v, str) or v == 1.0))) else None)
        self.bootstrap, self.random_state = bool(getattr(fitted, "bootstrap", False)), None
        self._set_model({**trees, "value": value}, int(fitted.n_features_in_))
        return self

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _queries(self, X):
        return _tree_host.query_matrix(self, X, torch.device(self.device), "random_forest")

    def _mean(self, Xq, limits=None):
        """float64 [m] on the device; ``limits = (n_estimators, max_depth, min_samples_split)`` stops every walk as a fit under them would."""
        m = Xq.shape[0]
        out = torch.empty(m, dtype=torch.float64, device=Xq.device)
        if m == 0:
            return out
        T, depth, mss = (self.n_estimators_, None, 0) if limits is None else limits
        if not 1 <= T <= self.n_estimators_:
            raise ValueError(f"random_forest: {T} trees asked of a forest of {self.n_estimators_}")
        t = self._dev
        with torch.cuda.device(Xq.device):
            _lib.check(_lib.lib().bbbp_rf_predict_mean(_dense.stream(), Xq.data_ptr(), Xq.shape[1], m, Xq.shape[1], t["left"].data_ptr(),
                                                       t["right"].data_ptr(), t["feature"].data_ptr(), t["threshold"].data_ptr(), t["value"].data_ptr(),
                                                       t["n_node_samples"].data_ptr(), t["root"].data_ptr(), int(T),
                                                       UNLIMITED if depth is None else int(depth), int(mss), out.data_ptr()), "bbbp_rf_predict_mean")
        return out

    def predict(self, X):
        """[m] float64: the trees' leaf means summed in tree order and divided by the number of trees."""
        Xq, was_numpy = self._queries(X)
        out = self._mean(Xq)
        return out.cpu().numpy() if was_numpy else out


class DecisionTreeRegressor(RandomForestRegressor):
    """``DecisionTreeRegressor(*, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, bootstrap=False, random_state=0,
    device="cuda")``: the same fit with one tree, every row once and all features at every node."""

    _who = "DecisionTreeRegressor"
    _params = RandomForestRegressor._params[1:]

    def __init__(self, *, max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features=None, bootstrap=False, random_state=0, device="cuda",
                 **other):
        super().__init__(1, max_depth=max_depth, min_samples_split=min_samples_split, min_samples_leaf=min_samples_leaf, max_features=max_features,
                         bootstrap=bootstrap, random_state=random_state, device=device, **other)


def _fit_regressors(regressors, problems):
    """Grow the forests of ``regressors[i]`` over ``problems[i] = (X, y)`` in one ``_grow`` call and fit every regressor from its own."""
    checked = [reg._checked(X, y) for reg, (X, y) in zip(regressors, problems)]
    with torch.cuda.device(torch.device(regressors[0].device)):
        specs = [reg._spec(X32, q, mf) for reg, (X32, q, _, mf) in zip(regressors, checked)]
        _grow(specs)
        for reg, spec, (_, _, s, _) in zip(regressors, specs, checked):
            reg._adopt(spec, s)


def fit_regressors(problems, **params):
    """``[RandomForestRegressor(**params).fit(X, y) for X, y in problems]`` with every tree of every problem grown in one batch: the
    reference's five folds of 300 trees and the stacker's six refits are one call.  Each regressor equals its single ``fit`` bit for bit."""
    problems = list(problems)
    if not problems:
        raise ValueError("random_forest.fit_regressors: no problems")
    regressors = [RandomForestRegressor(**params) for _ in problems]
    if len({str(torch.device(r.device)) for r in regressors}) != 1:
        raise ValueError("random_forest.fit_regressors: one device")
    _fit_regressors(regressors, problems)
    return regressors
