"""``sklearn.ensemble.GradientBoostingClassifier`` for the GPU: two classes, log-loss, exact-split regression trees fitted level by level.

The classification stack of the reference (``Models/model_opt_maccs.py:124-200``) searches ``GradientBoostingClassifier`` over
``n_estimators in {50, 100, 200}``, ``learning_rate in {0.01, 0.05, 0.1}``, ``max_depth in {3, 5, 7}`` and ``min_samples_split in
{2, 5, 10}`` under ``GridSearchCV(cv=5, scoring='f1')`` -- 405 fits on about 6 400 rows of 100 features -- and uses the same learner as
the ``StackingClassifier``'s final estimator.  The entry points of ``csrc/gbt.hip`` carry it:

* a training matrix is cast to float32 (scikit-learn's trees compare float32 features), transposed and every column's rows are sorted
  stably once; all chains over that matrix share both;
* ``bbbp_gbt_fit`` fits any number of chains side by side, one tree level per round of six launches, with no host read before the end;
* ``bbbp_gbt_staged_decision`` walks query rows through the trees in stage order and writes the raw score at every requested stage count
  in one pass, with scikit-learn's ``predict_stages`` arithmetic: a model adopted by ``from_sklearn`` predicts bit for bit what
  scikit-learn predicts.

The algorithm is scikit-learn 1.7's (``ensemble/_gb.py``, ``tree/_splitter.pyx``, ``_criterion.pyx``): raw scores start at the prior's
logit, a stage fits one tree to ``g = y - expit(raw)`` with the ``friedman_mse`` split score ``(n_r S_l - n_l S_r)^2 / (n_l n_r)``, a leaf's
value is ``mean(g) / mean(p (1 - p))`` and ``raw += learning_rate * value[leaf]``.  Residuals take few distinct values, so many splits
tie; scikit-learn breaks ties by a random feature order (its trees differ between any two ``random_state`` values), here the lowest
feature index wins among equal computed scores, then the lowest position.  Trees are therefore not scikit-learn's trees; they are
certified instead (``tests/gbt_replay.py``).  Results are bit-identical for a problem alone, in any batch, in any order and run to run.

Out of scope (each is refused by name): more than two classes, other losses and criteria, ``subsample < 1``, ``max_features``,
``sample_weight``, ``init`` estimators, ``n_iter_no_change``, ``max_leaf_nodes``, ``ccp_alpha``, ``min_impurity_decrease != 0``,
``max_depth > 7``, more than 8 192 rows or 1 024 features, more than one GPU.  There is no CPU path.

``GradientBoostingRegressor`` is the logBB stack's boosted learner (``Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:118-125``:
``GradientBoostingRegressor(n_estimators=200, learning_rate=0.1, max_depth=5, random_state=42)`` per fold) under the squared error.  It
grows through the same rounds with the loss swapped at compile time (``bbbp_gbr_fit``): ``g = y - raw`` from ``init_ = mean(y)``, a node's
value is ``sum g / m`` in leaves and split nodes alike, ``train_score_`` is the mean of ``(y - raw)^2``.  It shares the matrix, the chain,
the query path and the staged kernel with the classifier; ``fit_regressors`` fits the five folds and the refit in one batch.  Its trees
are certified by ``tests/gbr_replay.py``; on continuous features, where exact ties arise only between candidates that part the rows the
same way, its training-row predictions also agree with scikit-learn's to a few ulp.  The regressor's docstring lists what it refuses.

The training matrix (``Matrix``), the input checks, the flattening of scikit-learn's trees and the small uploads are shared with
``random_forest`` and live in ``_tree_host.py``; the kernels' shared device code is ``csrc/tree_fit.h``.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _estimator, _dense, _lib, _tree_host
from ._tree_host import Matrix as _Matrix, is_int as _is_int          # shared with random_forest: they live in _tree_host.py
from .linear_model import _binary_targets

MAX_ROWS, MAX_FEATURES, MAX_DEPTH, MAX_TREES = 8192, 1024, 7, 10000        # BBBP_GBT_FIT_MAX_*
GRID_KEYS = ("n_estimators", "learning_rate", "max_depth", "min_samples_split", "min_samples_leaf")
EPS32 = float(np.finfo(np.float32).eps)
_SKLEARN_DEFAULTS = dict(loss="log_loss", criterion="friedman_mse", subsample=1.0, max_features=None, init=None, n_iter_no_change=None,
                         max_leaf_nodes=None, ccp_alpha=0.0, min_impurity_decrease=0.0, min_weight_fraction_leaf=0.0, warm_start=False)


def _check_params(n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf, who="GradientBoostingClassifier"):
    if not _is_int(n_estimators) or not 1 <= n_estimators <= MAX_TREES:
        raise ValueError(f"{who}: n_estimators must be an int in 1..{MAX_TREES}, got {n_estimators!r}")
    if isinstance(learning_rate, bool) or not isinstance(learning_rate, numbers.Real) or not (0.0 < float(learning_rate) < float("inf")):
        raise ValueError(f"{who}: learning_rate must be a positive finite number, got {learning_rate!r}")
    if max_depth is None or not _is_int(max_depth):
        raise NotImplementedError(f"{who}: max_depth must be an int in 1..{MAX_DEPTH}, got {max_depth!r}")
    if max_depth < 1:
        raise ValueError(f"{who}: max_depth must be an int in 1..{MAX_DEPTH}, got {max_depth!r}")
    if max_depth > MAX_DEPTH:
        raise NotImplementedError(f"{who}: max_depth {max_depth} exceeds the {MAX_DEPTH} levels the kernels keep per tree")
    if not _is_int(min_samples_split):
        raise NotImplementedError(f"{who}: min_samples_split must be an int >= 2 (fractions are not supported), got {min_samples_split!r}")
    if min_samples_split < 2:
        raise ValueError(f"{who}: min_samples_split must be an int >= 2, got {min_samples_split!r}")
    if not _is_int(min_samples_leaf):
        raise NotImplementedError(f"{who}: min_samples_leaf must be an int >= 1 (fractions are not supported), got {min_samples_leaf!r}")
    if min_samples_leaf < 1:
        raise ValueError(f"{who}: min_samples_leaf must be an int >= 1, got {min_samples_leaf!r}")


def _training_matrix32(X, who):
    return _tree_host.training_matrix32(X, who, MAX_ROWS, MAX_FEATURES, "BBBP_GBT_FIT_MAX")


def _prior_logit(t):
    """scikit-learn's initial raw score for ``init=None``: the logit of the positive class's share, clipped to [eps32, 1 - eps32]."""
    from scipy.special import logit
    return float(logit(np.clip(np.float64(np.mean(t)), EPS32, 1.0 - EPS32)))


class _Chain:
    """One model to fit: its outputs, its work area and the descriptor ``bbbp_gbt_fit`` and ``bbbp_gbr_fit`` take (``t_d``: the 0.0 / 1.0
    labels or the regression targets, float64 on the device).  Nothing needs initialising."""

    def __init__(self, mat, t_d, init, n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf):
        L, dev = _lib.lib(), mat.XT.device
        nbytes = L.bbbp_gbt_fit_work_bytes(mat.n, mat.d)
        self.cap = L.bbbp_gbt_fit_tree_capacity(max_depth)
        if not nbytes or not self.cap:
            raise ValueError("gradient_boosting: " + L.bbbp_last_error().decode("utf-8", "replace"))
        T = int(n_estimators)
        self.mat, self.t, self.T, self.init, self.learning_rate = mat, t_d, T, float(init), float(learning_rate)
        self.params = (T, float(learning_rate), int(max_depth), int(min_samples_split), int(min_samples_leaf))
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
        f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)  # noqa: E731
        self.left, self.right, self.feature, self.nns = i32(T * self.cap), i32(T * self.cap), i32(T * self.cap), i32(T * self.cap)
        self.threshold, self.value = f64(T * self.cap), f64(T * self.cap)
        self.tree_nodes, self.train_score, self.raw = i32(T), f64(T), f64(mat.n)
        self.desc = _lib.GbtChain(mat.XT.data_ptr(), mat.order0.data_ptr(), t_d.data_ptr(), mat.n, mat.d, T, int(max_depth), int(min_samples_split),
                                  int(min_samples_leaf), float(learning_rate), float(init), self.work.data_ptr(), self.left.data_ptr(),
                                  self.right.data_ptr(), self.feature.data_ptr(), self.nns.data_ptr(), self.threshold.data_ptr(), self.value.data_ptr(),
                                  self.tree_nodes.data_ptr(), self.train_score.data_ptr(), self.raw.data_ptr())

    def trees(self):
        """The fitted trees as flat host arrays in ``ForestGPU.flatten_sklearn``'s convention (absolute child indices, -1 at a leaf), plus
        ``n_node_samples``; the one host read of a fit."""
        counts = self.tree_nodes.cpu().numpy().astype(np.int64)
        if (counts < 1).any():
            raise RuntimeError(f"gradient_boosting: the fit kernels reported an index outside its array in tree {int(np.argmax(counts < 1))} "
                               "(a defect of csrc/gbt.hip, not of the data); no model is returned")
        root = np.concatenate([[0], np.cumsum(counts)])
        keep = (np.arange(self.cap)[None, :] < counts[:, None]).ravel()
        pick = lambda a: a.cpu().numpy()[keep]  # noqa: E731
        left, right = _tree_host.rebase_children(pick(self.left), pick(self.right), np.repeat(root[:-1], counts))
        return dict(left=left, right=right, feature=pick(self.feature), threshold=pick(self.threshold), value=pick(self.value),
                    n_node_samples=pick(self.nns), root=root.astype(np.int32))


def _fit_chains(chains, entry="bbbp_gbt_fit"):
    """``entry`` (``bbbp_gbt_fit``: the log-loss, ``bbbp_gbr_fit``: the squared error) over all chains in one batch: the descriptors go to
    the device once, nothing is read back here."""
    dev = chains[0].work.device
    arr = (_lib.GbtChain * len(chains))(*[c.desc for c in chains])
    on_device = _tree_host.upload(arr, dev)
    _lib.check(getattr(_lib.lib(), entry)(_dense.stream(), arr, on_device.data_ptr(), len(chains)), entry)
    return on_device                                   # kept alive by the caller until the results are read


def _sklearn_trees(fitted):
    """A fitted scikit-learn booster's trees (one column of ``estimators_``) as the flat host arrays of ``trees_``, and its feature count."""
    trees, (value,) = _tree_host.sklearn_trees(fitted.estimators_[:, 0])
    return {**trees, "value": value}, int(fitted.n_features_in_)


class _BoostedTrees:
    """What the classifier and the regressor share once a model is there: its trees on the device, the query path and the staged raw
    scores of ``bbbp_gbt_staged_decision``.  ``self.device`` is anything ``torch.device`` takes."""

    def _set_trees(self, trees, init, learning_rate, n_features):
        _tree_host.check_trees(trees, n_features, "gradient_boosting", ("right", "feature", "threshold", "value"))
        self.trees_, self.init_, self.n_features_in_ = trees, float(init), int(n_features)
        self.n_estimators_ = len(trees["root"]) - 1
        self._lr = float(learning_rate)
        self._dev = _tree_host.to_device(trees, ("left", "right", "feature", "threshold", "value", "root"), ("threshold", "value"), torch.device(self.device))

    def _queries(self, X):
        return _tree_host.query_matrix(self, X, torch.device(self.device), "gradient_boosting")

    def _staged(self, Xq, stages):
        """Raw scores [len(stages), m] after ``stages`` trees each (ascending, within 1..n_estimators_)."""
        m, dev = Xq.shape[0], torch.device(self.device)
        out = torch.empty((len(stages), m), dtype=torch.float64, device=dev)
        if m == 0:
            return out
        stages_d = torch.tensor(list(stages), dtype=torch.int32, device=dev)
        t = self._dev
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bbbp_gbt_staged_decision(_dense.stream(), Xq.data_ptr(), Xq.shape[1], m, Xq.shape[1], t["left"].data_ptr(),
                                                           t["right"].data_ptr(), t["feature"].data_ptr(), t["threshold"].data_ptr(), t["value"].data_ptr(),
                                                           t["root"].data_ptr(), self.n_estimators_, self.init_, self._lr, stages_d.data_ptr(), len(stages),
                                                           out.data_ptr()), "bbbp_gbt_staged_decision")
        return out


class GradientBoostingClassifier(_estimator.Params, _BoostedTrees):
    """``GradientBoostingClassifier(n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, *,
    device="cuda")``: scikit-learn's names for two classes and the log-loss.

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (n <= 8 192, d <= 1 024; cast to float32, as scikit-learn's trees do) and labels
    with two distinct values; ``classes_[1]`` is the positive class.  It sets ``classes_``, ``n_estimators_``, ``n_features_in_``,
    ``init_`` (the prior's logit), ``train_score_`` (scikit-learn's: twice the mean of ``log(1 + exp(raw)) - y raw`` after each stage) and ``trees_``: ``left``, ``right``, ``feature``,
    float64 ``threshold``, ``value``, ``n_node_samples`` and ``root`` in ``ForestGPU.flatten_sklearn``'s convention, nodes numbered level
    by level.  ``decision_function`` returns float64 [m] (numpy for numpy input, a CUDA tensor for a CUDA tensor), positive meaning
    ``classes_[1]``; ``staged_decision_function`` yields it after every stage; ``predict_proba`` is ``[1 - p, p]`` with ``p =
    expit(decision)``; ``predict`` is ``classes_[decision >= 0]``, scikit-learn's rule."""

    def __init__(self, n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, *, device="cuda", random_state=None,
                 verbose=0, **other):
        _tree_host.refuse_non_defaults("GradientBoostingClassifier", other, _SKLEARN_DEFAULTS)
        _check_params(n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"GradientBoostingClassifier: device {device!r}: trees are fitted on the GPU (no CPU fallback)")
        self.n_estimators, self.learning_rate, self.max_depth = int(n_estimators), float(learning_rate), int(max_depth)
        self.min_samples_split, self.min_samples_leaf = int(min_samples_split), int(min_samples_leaf)
        self.random_state = random_state                 # accepted and unused: ties are broken by the fixed rule, not by a random order

    _params = ("n_estimators", "learning_rate", "max_depth", "min_samples_split", "min_samples_leaf", "random_state", "device")

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        who = "GradientBoostingClassifier"
        if sample_weight is not None:
            raise ValueError(f"{who}: sample_weight is not supported")
        _fit_classifiers([self], [(X, y)])
        return self

    def _adopt(self, classes, chain, n_estimators=None):
        """Fitted attributes from a fitted chain; ``n_estimators`` below the chain's keeps its first trees (a shorter model is the prefix of a
        longer one)."""
        trees = chain.trees()
        T = chain.T if n_estimators is None else int(n_estimators)
        if T < chain.T:
            end = int(trees["root"][T])
            trees = {k: (v[:T + 1] if k == "root" else v[:end]) for k, v in trees.items()}
        self._set_model(classes, trees, chain.init, chain.learning_rate, chain.mat.d)
        self.train_score_ = chain.train_score.cpu().numpy()[:T].copy()
        self._train_raw = chain.raw.cpu().numpy() if T == chain.T else None       # the training rows' raw scores after the last stage (tests)

    def _set_model(self, classes, trees, init, learning_rate, n_features):
        self._set_trees(trees, init, learning_rate, n_features)
        self.classes_ = classes

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """Adopt a fitted scikit-learn ``GradientBoostingClassifier`` (two classes, ``init=None``) for prediction only:
        ``decision_function`` and every stage of ``staged_decision_function`` equal scikit-learn's bit for bit."""
        from scipy.special import logit
        from sklearn.dummy import DummyClassifier
        if getattr(fitted, "n_classes_", None) != 2 or fitted.estimators_.shape[1] != 1:
            raise ValueError("GradientBoostingClassifier.from_sklearn: exactly two classes are supported")
        if not isinstance(fitted.init_, DummyClassifier) or fitted.init_.strategy != "prior":
            raise NotImplementedError("GradientBoostingClassifier.from_sklearn: init estimators are not supported (only init=None, the prior)")
        self = cls(1, float(fitted.learning_rate), device=device)
        trees, d = _sklearn_trees(fitted)
        init = float(logit(np.clip(np.float64(fitted.init_.class_prior_[1]), EPS32, 1.0 - EPS32)))
        self.n_estimators = len(trees["root"]) - 1
        # the fitting parameters are kept only where this class would accept them (scikit-learn allows None and fractions): an adopted
        # model predicts, it is not refitted
        for name in ("max_depth", "min_samples_split", "min_samples_leaf"):
            setattr(self, name, getattr(fitted, name) if _is_int(getattr(fitted, name)) else None)
        self._set_model(np.asarray(fitted.classes_), trees, init, float(fitted.learning_rate), d)
        self.train_score_ = np.asarray(fitted.train_score_, dtype=np.float64).copy()
        self._train_raw = None
        return self

    # ---- decision ---------------------------------------------------------------------------------------------------
    def decision_function(self, X):
        """The raw score of every row after all stages; positive means ``classes_[1]``."""
        Xq, was_numpy = self._queries(X)
        out = self._staged(Xq, [self.n_estimators_])[0]
        return out.cpu().numpy() if was_numpy else out

    def staged_decision_function(self, X):
        """Yields the raw scores [m] after 1, 2, ... trees (computed in one pass over the trees)."""
        Xq, was_numpy = self._queries(X)
        out = self._staged(Xq, range(1, self.n_estimators_ + 1))
        out = out.cpu().numpy() if was_numpy else out
        for s in range(self.n_estimators_):
            yield out[s]

    def predict_proba(self, X):
        """[m, 2]: ``[1 - p, p]`` with ``p = expit(decision_function(X))``."""
        Xq, was_numpy = self._queries(X)
        p = torch.special.expit(self._staged(Xq, [self.n_estimators_])[0])
        out = torch.stack([1.0 - p, p], dim=1)
        return out.cpu().numpy() if was_numpy else out

    def predict_log_proba(self, X):
        """log of ``predict_proba``, each column from ``logsigmoid`` of the decision value."""
        Xq, was_numpy = self._queries(X)
        z = self._staged(Xq, [self.n_estimators_])[0]
        out = torch.stack([torch.nn.functional.logsigmoid(-z), torch.nn.functional.logsigmoid(z)], dim=1)
        return out.cpu().numpy() if was_numpy else out

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype: ``classes_[1]`` where the decision value is >= 0 (scikit-learn's rule)."""
        Xq, _ = self._queries(X)
        return self.classes_[(self._staged(Xq, [self.n_estimators_])[0] >= 0).cpu().numpy().astype(np.intp)]


def _fit_classifiers(classifiers, problems):
    """Fit the chains of ``classifiers[i]`` over ``problems[i] = (X, y)`` in one ``bbbp_gbt_fit`` batch and every classifier from its own: what
    ``fit`` does, for one or many (``ensemble`` fits a learner on all rows and on every fold's training rows this way).  Each classifier
    equals its single ``fit`` bit for bit."""
    who = "GradientBoostingClassifier"
    checked = []
    for X, y in problems:
        classes, t = _binary_targets(y, None, who)
        X32 = _training_matrix32(X, who)
        if X32.shape[0] != len(t):
            raise ValueError(f"{who}: X has {X32.shape[0]} rows, y has {len(t)}")
        checked.append((classes, t, X32))
    with torch.cuda.device(classifiers[0].device):
        chains = [_Chain(_Matrix(X32, clf.device), torch.from_numpy(t).to(clf.device), _prior_logit(t), clf.n_estimators, clf.learning_rate, clf.max_depth,
                         clf.min_samples_split, clf.min_samples_leaf) for clf, (_, t, X32) in zip(classifiers, checked)]
        keep = _fit_chains(chains)
        for clf, chain, (classes, _, _) in zip(classifiers, chains, checked):
            clf._adopt(classes, chain)
        del keep


def grid_points(param_grid, who="gradient_boosting.grid_search_cv"):
    """The grid's points in scikit-learn's order (sorted keys, ``itertools.product``; a list of grids one after the other) and each point's
    full parameter tuple (n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf), checked."""
    defaults = dict(n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1)
    return _tree_host.grid_points(param_grid, GRID_KEYS, defaults, _check_params, who)


def _cv_chains(X32, t_all, folds, full, dev):
    """One chain per (fold, distinct (learning_rate, max_depth, min_samples_split, min_samples_leaf)) to the largest ``n_estimators`` asked
    of it, all fitted in one batch.  Returns ({(fold, rest): chain}, the folds' test rows on the device, what must outlive the read)."""
    longest = {}
    for params in full:
        longest[params[1:]] = max(longest.get(params[1:], 0), params[0])
    chains, queries = {}, []
    for fi, (tr, te) in enumerate(folds):
        mat = _Matrix(X32[tr], dev)
        t_d = torch.from_numpy(t_all[tr]).to(dev)
        init = _prior_logit(t_all[tr])
        queries.append(torch.from_numpy(X32[te]).to(dev))
        for rest, T in longest.items():
            chains[(fi, rest)] = _Chain(mat, t_d, init, T, *rest)
    return chains, queries, _fit_chains(list(chains.values()))


def grid_search_cv(X, y, param_grid, cv: int = 5, device="cuda"):
    """The reference's ``GridSearchCV(GradientBoostingClassifier(), param_grid, cv=5, scoring='f1')`` (model_opt_maccs.py:124-200) over
    ``n_estimators``, ``learning_rate``, ``max_depth``, ``min_samples_split`` and ``min_samples_leaf``.

    Same conventions as ``svm.grid_search_cv`` and ``linear_model.grid_search_cv``: sorted keys, ``itertools.product`` order,
    scikit-learn's ``StratifiedKFold(cv)``, ``f1_score`` of ``classes_[1]``, the first maximum wins.  Without subsampling a shorter model is
    the prefix of a longer one, so every fold fits one chain per distinct (learning_rate, max_depth, min_samples_split,
    min_samples_leaf) to the largest ``n_estimators`` asked of it and the shorter models are scored from staged decisions.  All chains of
    all folds are fitted in one batch; every grid point equals a single ``fit`` on that fold bit for bit; the refit follows.
    Returns (best_params, mean F1 per point, the classifier refitted on all rows with best_params)."""
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    who = "gradient_boosting.grid_search_cv"
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
        chains, queries, keep = _cv_chains(X32, t_all, folds, full, dev)
        for (fi, rest), chain in chains.items():
            clf = GradientBoostingClassifier(chain.T, *rest, device=dev)
            clf._adopt(classes, chain)
            wanted = sorted({p[0] for p in full if p[1:] == rest})
            staged = (clf._staged(queries[fi], wanted) >= 0).cpu().numpy()
            preds = {T: classes[staged[j].astype(np.intp)] for j, T in enumerate(wanted)}
            for pi, params in enumerate(full):
                if params[1:] == rest:
                    f1[pi, fi] = f1_score(y[folds[fi][1]], preds[params[0]], pos_label=pos)
        del keep, chains, queries
    scores = [float(v) for v in f1.mean(axis=1)]
    best = int(np.argmax(scores))
    fitted = GradientBoostingClassifier(*full[best], device=dev).fit(X32, y)
    return points[best], scores, fitted


# ---- regression: GradientBoostingRegressor under the squared error ---------------------------------------------------------------------
_REGRESSOR_DEFAULTS = dict(criterion="friedman_mse", subsample=1.0, max_features=None, init=None, alpha=0.9, n_iter_no_change=None, max_leaf_nodes=None,
                           ccp_alpha=0.0, min_impurity_decrease=0.0, min_weight_fraction_leaf=0.0, warm_start=False)
_REGRESSOR_IGNORED = ("verbose", "tol", "validation_fraction")      # accepted with any value: none changes the model (the last two act only with n_iter_no_change)
# The largest |y - mean(y)| a fit takes.  The split score squares n_r S_l - n_l S_r, at most 2 n^2 max |g| in size: with n <= 8 192 its square
# stays below 2^54 (1e140)^2 < 1.8e296 in the first stage, and so do sum g^2 <= n (1e140)^2 and (y - raw)^2.  That leaves the square twelve
# orders of magnitude, the residuals six, should a learning rate make them grow from stage to stage instead of shrink
MAX_TARGET_SPREAD = 1e140


def _regression_targets(y, n_rows, who):
    """The targets as finite float64 [n] on the host, unrounded, and their mean (scikit-learn's ``DummyRegressor`` constant, ``np.average``)."""
    y = _tree_host.targets_1d(y, n_rows, who, "more than one output column is not supported")
    with np.errstate(over="ignore", invalid="ignore"):
        init = float(np.average(y))
        spread = float(np.abs(y - init).max())
    if not np.isfinite(init) or not spread <= MAX_TARGET_SPREAD:
        raise ValueError(f"{who}: the targets are too large: |y - mean| must not exceed {MAX_TARGET_SPREAD:g}, beyond which the split score, and "
                         "further out (y - mean)^2 itself, overflows float64")
    return y, init


class GradientBoostingRegressor(_BoostedTrees):
    """``GradientBoostingRegressor(n_estimators=100, *, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1,
    loss="squared_error", random_state=None, device="cuda")``: scikit-learn's names for one output and the squared error -- the reference's
    ``GradientBoostingRegressor(n_estimators=200, learning_rate=0.1, max_depth=5, random_state=42)`` of the logBB stack's bake-off
    (Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:118-125).

    ``fit`` takes a numpy array or a CUDA tensor [n, d] (n <= 8 192, d <= 1 024; cast to float32) and finite float64 targets [n] or [n, 1],
    which reach the kernels unrounded.  Raw scores start at ``init_ = np.average(y)``; a stage fits one ``friedman_mse`` tree to ``g = y - raw``
    through the classifier's rounds (``bbbp_gbr_fit``), a node's value is ``sum g / m`` -- scikit-learn leaves this loss's leaves as the tree
    made them -- and ``raw += learning_rate * value[leaf]``.  Sets ``n_estimators_``, ``n_features_in_``, ``init_``, ``train_score_`` (the mean
    of ``(y - raw)^2`` after each stage) and ``trees_`` in the classifier's convention.  ``predict`` returns float64 [m] (numpy for numpy
    queries, a CUDA tensor for a CUDA tensor), ``staged_predict`` yields it after every stage, ``predict_device`` is ``predict`` for the
    device-resident features of ``ensemble.screen(boosters=...)``.  ``random_state`` is accepted and unused: among equal computed scores
    the lowest feature wins, then the lowest position, so trees are certified (``tests/gbr_replay.py``), not compared with scikit-learn's.
    ``get_params`` / ``set_params`` make ``sklearn.base.clone`` work, so ``ensemble.StackingRegressor`` takes this class as a base learner.

    Out of scope, each refused by name: other losses (``huber``, ``absolute_error``, ``quantile``) and ``alpha``, ``criterion !=
    "friedman_mse"``, ``subsample < 1``, ``max_features``, ``init`` estimators, ``n_iter_no_change``, ``max_leaf_nodes``, ``ccp_alpha``,
    ``min_impurity_decrease != 0``, ``warm_start``, ``sample_weight``, more than one output column, non-finite targets, targets further
    than 1e140 from their mean (``MAX_TARGET_SPREAD``: beyond it the split score overflows float64), ``max_depth > 7`` or None, fractional
    limits, more than 8 192 rows or 1 024 features.  ``verbose``, ``tol`` and ``validation_fraction`` are accepted and ignored: they do not
    change the model.  There is no regressor grid search (the reference has none) and no CPU path."""

    _who = "GradientBoostingRegressor"
    _params = ("n_estimators", "learning_rate", "max_depth", "min_samples_split", "min_samples_leaf", "loss", "random_state", "device")

    def __init__(self, n_estimators=100, *, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, loss="squared_error",
                 random_state=None, device="cuda", **other):
        who = self._who
        if loss != "squared_error":
            raise NotImplementedError(f"{who}: loss={loss!r} is not supported (only 'squared_error')")
        _tree_host.refuse_non_defaults(who, other, _REGRESSOR_DEFAULTS, _REGRESSOR_IGNORED)
        _check_params(n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf, who)
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU fallback)")
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.n_estimators, self.learning_rate, self.max_depth = n_estimators, learning_rate, max_depth
        self.min_samples_split, self.min_samples_leaf, self.loss = min_samples_split, min_samples_leaf, loss
        self.random_state, self.device = random_state, device          # random_state: accepted and unused, the tie rule is fixed

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._params}

    def set_params(self, **params):
        unknown = set(params) - set(self._params)
        if unknown:
            raise ValueError(f"{self._who}: unknown parameters {sorted(unknown)}")
        type(self)(**params)           # the constructor's checks, on what is being set alone: every parameter is judged by itself, and an
        for name, value in params.items():      # adopted model may hold a None where scikit-learn's value was not an int
            setattr(self, name, value)
        return self

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError(f"{self._who}: sample_weight is not supported")
        _fit_regressors([self], [(X, y)])
        return self

    def _checked(self, X, y):
        """(float32 X, the float64 targets, their mean), validated: no GPU call yet."""
        X32 = _training_matrix32(X, self._who)
        return (X32,) + _regression_targets(y, X32.shape[0], self._who)

    def _chain(self, X32, y, init):
        """The chain this regressor asks for, not yet fitted."""
        dev = torch.device(self.device)
        return _Chain(_Matrix(X32, dev), torch.from_numpy(y).to(dev), init, self.n_estimators, self.learning_rate, self.max_depth, self.min_samples_split,
                      self.min_samples_leaf)

    def _adopt(self, chain):
        """Fitted attributes from a fitted chain."""
        self._set_trees(chain.trees(), chain.init, chain.learning_rate, chain.mat.d)
        self.train_score_ = chain.train_score.cpu().numpy().copy()
        self._train_raw = chain.raw.cpu().numpy()              # the training rows' raw scores after the last stage (tests)

    @classmethod
    def from_sklearn(cls, fitted, device="cuda"):
        """Adopt a fitted scikit-learn ``GradientBoostingRegressor`` (``loss="squared_error"``, ``init=None``) for prediction only: ``predict``
        and every stage of ``staged_predict`` equal scikit-learn's bit for bit.  ``max_depth``, ``min_samples_split`` and ``min_samples_leaf``
        are kept where they are ints and None otherwise; ``set_params`` works on an adopted model, but ``sklearn.base.clone`` of one that
        holds such a None is refused, like any unfitted regressor with that value (an adopted model predicts, it is not refitted)."""
        from sklearn.dummy import DummyRegressor
        who = f"{cls.__name__}.from_sklearn"
        if hasattr(fitted, "classes_") or getattr(fitted, "loss", None) != "squared_error" or fitted.estimators_.shape[1] != 1:
            raise NotImplementedError(f"{who}: a fitted regressor with loss='squared_error' and one output is expected")
        if not isinstance(fitted.init_, DummyRegressor) or fitted.init_.strategy != "mean":
            raise NotImplementedError(f"{who}: init estimators are not supported (only init=None, the mean)")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{who}: device {device!r}: prediction runs on the GPU (no CPU fallback)")
        trees, d = _sklearn_trees(fitted)
        self = cls.__new__(cls)
        # the fitting parameters are kept only where this class would accept them (scikit-learn allows None and fractions): an adopted
        # model predicts, it is not refitted
        self.n_estimators, self.learning_rate, self.loss, self.random_state, self.device = len(trees["root"]) - 1, float(fitted.learning_rate), "squared_error", None, device
        for name in ("max_depth", "min_samples_split", "min_samples_leaf"):
            setattr(self, name, getattr(fitted, name) if _is_int(getattr(fitted, name)) else None)
        self._set_trees(trees, float(np.ravel(fitted.init_.constant_)[0]), float(fitted.learning_rate), d)
        self.train_score_ = np.asarray(fitted.train_score_, dtype=np.float64).copy()
        self._train_raw = None
        return self

    # ---- prediction -------------------------------------------------------------------------------------------------
    def predict(self, X):
        """[m] float64: ``init_`` plus ``learning_rate * value[leaf]`` of every tree in stage order."""
        Xq, was_numpy = self._queries(X)
        out = self._staged(Xq, [self.n_estimators_])[0]
        return out.cpu().numpy() if was_numpy else out

    def staged_predict(self, X):
        """Yields the predictions [m] after 1, 2, ... trees (computed in one pass over the trees)."""
        Xq, was_numpy = self._queries(X)
        out = self._staged(Xq, range(1, self.n_estimators_ + 1))
        out = out.cpu().numpy() if was_numpy else out
        for s in range(self.n_estimators_):
            yield out[s]

    def predict_device(self, X):
        """``predict`` for a CUDA tensor [m, d]: float64 [m] on the device (what ``ensemble.screen`` asks of its ``boosters``)."""
        if not isinstance(X, torch.Tensor):
            raise TypeError(f"{self._who}.predict_device: expected a CUDA (HIP) tensor, got {type(X).__name__}")
        return self.predict(X)


def _fit_regressors(regressors, problems):
    """Fit the chains of ``regressors[i]`` over ``problems[i] = (X, y)`` in one ``bbbp_gbr_fit`` batch and every regressor from its own."""
    checked = [reg._checked(X, y) for reg, (X, y) in zip(regressors, problems)]
    with torch.cuda.device(torch.device(regressors[0].device)):
        chains = [reg._chain(*c) for reg, c in zip(regressors, checked)]
        keep = _fit_chains(chains, "bbbp_gbr_fit")
        for reg, chain in zip(regressors, chains):
            reg._adopt(chain)
        del keep


def fit_regressors(problems, **params):
    """``[GradientBoostingRegressor(**params).fit(X, y) for X, y in problems]`` with every problem's chain in one batch: the bake-off's
    five folds and the refit are one call.  Each regressor equals its single ``fit`` bit for bit."""
    problems = list(problems)
    if not problems:
        raise ValueError("gradient_boosting.fit_regressors: no problems")
    regressors = [GradientBoostingRegressor(**params) for _ in problems]
    _fit_regressors(regressors, problems)
    return regressors
