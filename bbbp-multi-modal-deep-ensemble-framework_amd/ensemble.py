"""The reference's ensembles over fitted learners: the regression stack of the logBB scripts and the classifier stack of the BBB+/- scripts.

Regression half (float64, host side: k <= 4 columns, N ~ 1e3 rows).  The reference stacks out-of-fold predictions ``[nn, rf, xgb(, cat)]``
with a linear meta-learner -- ``Ridge(alpha=1.0)`` (Models/multi_input_data_regression_opt_transformer_cnn_opt.py:173-176),
``LinearRegression`` (..._morgan.py, same lines; final estimator of the StackingRegressor at ...20250113.py:394-403) -- or a fixed weighted
sum 0.4/0.3/0.3 (Models/multi_input_data_regression_opt_transformer_cnn.py:216-218), and later calls
``loaded_stacked_model.predict([[nn_out, rf_pred, xgb_pred]])`` (..._opt.py:202-203).  The meta-learner is a 3-4 parameter least-squares
problem, so it stays on the host in float64 like sklearn's (``StackedEnsemble``, ``StackingRegressor``, ``weighted_ensemble``);
``predict_device`` applies it to device-resident NN predictions during screening (``screen``).

Classification half (GPU).  Every classification script (Models/model_opt.py:208-222 and its ``_maccs``, ``_rdkit``, ``_all`` siblings)
tunes eight base learners and builds ``StackingClassifier(estimators, final_estimator=GradientBoostingClassifier(n_estimators=100,
learning_rate=0.1, max_depth=3), cv=5)`` and ``VotingClassifier(estimators, voting='soft')`` from them.  ``StackingClassifier``,
``VotingClassifier`` and ``fit_classifier_stack`` are those two with scikit-learn 1.7's names and semantics for two classes, over this
package's learners (``neighbors``, ``linear_model``, ``svm.PlattSVC``, ``naive_bayes``, ``random_forest``, ``gradient_boosting``,
``mlp.MLPClassifier``) or any object with ``fit``, ``get_params`` and a prediction method that takes what it is given:

* X is uploaded once; the labels are encoded to 0 / 1 through ``classes_ = np.unique(y)`` and the base learners and the final estimator are
  fitted on the encoded labels, as scikit-learn fits them, so a base learner's ``classes_`` must come out as ``[0, 1]``;
* ``_fit_rows`` fits one learner on several row sets -- all rows and the training rows of every fold -- side by side through the
  learner's own list-of-problems path (``random_forest._grow``, ``gradient_boosting._fit_chains``, ``GridMLPTrainer.fit`` with
  ``train_rows``, ``naive_bayes.fit_masks``, ``linear_model._solve``); each fit equals the one-at-a-time fit bit for bit.  kNN (nothing to
  fit), ``svm.PlattSVC`` / ``svm.SVC`` and foreign learners are looped;
* the folds are scikit-learn's ``StratifiedKFold(cv)`` without shuffling, or an explicit list of ``(train, test)`` index pairs;
* the out-of-fold matrix, ``transform`` and the votes are assembled on the device by the three entries of ``csrc/ensemble.hip``, one
  launch each, pinned bit for bit to ``tests/ensemble_numpy.py``.  The stack itself brings no probability back to the host before the
  final estimator is fitted, and seven of the eight learners answer a CUDA tensor from the device.  ``naive_bayes.BernoulliNB`` does
  not: its ``predict_proba`` normalises the joint log-likelihoods on the host with scipy's ``logsumexp`` and numpy's ``exp``, whatever the
  input was, to have scikit-learn's bits, and uploads the result again -- so its column crosses the bus once per fold, per ``transform`` and
  per vote.  That learner is not changed here, and a device ``exp`` / ``log`` would not give numpy's bits: this requirement is unmet for it;
* ``fit_classifier_stack`` returns both models from one set of full-data fits and one set of fold fits (the reference fits the full-data
  learners twice; every learner here is deterministic given its ``random_state``, so the shared fits are the same models).

Refused by name: more than two classes, ``sample_weight``, ``cv="prefit"`` or a splitter object, ``n_jobs`` other than None or 1, ``"drop"``
estimators, a device other than CUDA.  There is no CPU path for the classification half.
"""
from __future__ import annotations

import ctypes
import numbers

import numpy as np
import torch

from . import _dense, _estimator, _lib, _tree_host


def weighted_ensemble(nn_pred, rf_pred, xgb_pred, weights=(0.4, 0.3, 0.3)):
    """0.4*nn + 0.3*rf + 0.3*xgb (..._transformer_cnn.py:216-218)."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (nn_pred, rf_pred, xgb_pred))
    return weights[0] * a + weights[1] * b + weights[2] * c


class StackedEnsemble:
    """Linear meta-learner with sklearn's attribute names: ``alpha=0`` is LinearRegression, ``alpha=1`` the
    reference's Ridge.  The intercept is not penalised (sklearn semantics)."""

    def __init__(self, alpha: float = 0.0):
        if alpha < 0:
            raise ValueError("alpha must be >= 0")
        self.alpha = float(alpha)
        self.coef_ = None
        self.intercept_ = None

    @classmethod
    def from_coefficients(cls, coef, intercept, alpha: float = 0.0):
        """Rebuild a fitted meta-learner, e.g. from the values stored in the reference's stacked_model*.pkl."""
        self = cls(alpha)
        self.coef_ = np.asarray(coef, dtype=np.float64).copy()
        self.intercept_ = float(intercept)
        return self

    def fit(self, X, y):
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError(f"X {X.shape} and y {y.shape} do not match")
        xm, ym = X.mean(axis=0), y.mean()
        Xc, yc = X - xm, y - ym
        if self.alpha == 0.0:
            self.coef_ = np.linalg.lstsq(Xc, yc, rcond=None)[0]
        else:
            self.coef_ = np.linalg.solve(Xc.T @ Xc + self.alpha * np.eye(X.shape[1]), Xc.T @ yc)
        self.intercept_ = float(ym - xm @ self.coef_)
        return self

    def predict(self, X):
        if self.coef_ is None:
            raise RuntimeError("StackedEnsemble is not fitted")
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.coef_.shape[0]:
            raise ValueError(f"X has shape {X.shape}, expected [N, {self.coef_.shape[0]}]")
        return X @ self.coef_ + self.intercept_

    def predict_device(self, nn_pred, *other_columns):
        """Same arithmetic on torch tensors (float64 on the tensors' device): screening keeps NN outputs on the GPU."""
        import torch
        cols = [nn_pred.reshape(-1).to(torch.float64)] + [torch.as_tensor(c, device=nn_pred.device).reshape(-1).to(torch.float64)
                                                          for c in other_columns]
        if len(cols) != self.coef_.shape[0]:
            raise ValueError(f"{len(cols)} columns given, meta-learner has {self.coef_.shape[0]} coefficients")
        out = torch.full_like(cols[0], self.intercept_)
        for c, w in zip(cols, self.coef_):
            out = out + float(w) * c
        return out


class StackingRegressor:
    """``sklearn.ensemble.StackingRegressor(estimators, final_estimator=LinearRegression())`` as the published script builds
    and uses it (Models/multi_input_data_regression_opt_transformer_cnn_20250113.py:394-403) -- NOT ``X c + b`` on the input
    columns: ``fit(X, y)`` (X = the [N,4] out-of-fold matrix ``[nn, rf, xgb, cat]``) fits every base learner on ALL of X,
    builds the meta-features from 5-fold ``cross_val_predict`` of clones (``KFold(5)`` without shuffling, scikit-learn's default
    for regressors) and fits the final linear model on those [N, n_estimators] columns; ``predict(X)`` runs the full-data base
    learners and the final model on their outputs.  Base learners are anything with scikit-learn's ``fit`` / ``predict``
    (third-party CPU code, as in the reference); fitted random forests / extra-trees predict through ``trees.ForestGPU`` when
    ``device`` is given.  The final estimator is this module's ``StackedEnsemble`` (OLS by default)."""

    def __init__(self, estimators, final_estimator=None, cv: int = 5, device=None):
        self.estimators = list(estimators)
        self.final_estimator = final_estimator if final_estimator is not None else StackedEnsemble(0.0)
        self.cv, self.device = int(cv), device
        self.estimators_ = None
        self.final_estimator_ = None

    def _predict_one(self, est, X):
        if self.device is not None and hasattr(est, "estimators_") and hasattr(est.estimators_[0], "tree_"):
            from .trees import ForestGPU
            return ForestGPU.from_sklearn(est, device=self.device).predict(X)
        return np.asarray(est.predict(X), dtype=np.float64)

    def fit(self, X, y):
        from sklearn.base import clone
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        n = X.shape[0]
        if X.ndim != 2 or n != y.shape[0]:
            raise ValueError(f"X {X.shape} and y {y.shape} do not match")
        if n < self.cv:
            raise ValueError(f"cv={self.cv} folds need at least as many rows, got {n}")
        self.estimators_ = [(name, clone(est).fit(X, y)) for name, est in self.estimators]
        # KFold(cv) without shuffling: the first n % cv folds have one row more
        sizes = np.full(self.cv, n // self.cv); sizes[: n % self.cv] += 1
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        meta = np.zeros((n, len(self.estimators)))
        for f in range(self.cv):
            test = np.arange(bounds[f], bounds[f + 1])
            train = np.concatenate([np.arange(0, bounds[f]), np.arange(bounds[f + 1], n)])
            for j, (_, est) in enumerate(self.estimators):
                meta[test, j] = self._predict_one(clone(est).fit(X[train], y[train]), X[test])
        self.final_estimator_ = StackedEnsemble(getattr(self.final_estimator, "alpha", 0.0)).fit(meta, y)
        return self

    def transform(self, X):
        if self.estimators_ is None:
            raise RuntimeError("StackingRegressor is not fitted")
        X = np.asarray(X, dtype=np.float64)
        return np.stack([self._predict_one(est, X) for _, est in self.estimators_], axis=1)

    def predict(self, X):
        return self.final_estimator_.predict(self.transform(X))


def screen(model, forest, stack, fingerprints, images, extra_columns=(), batch_size: int = 4096, boosters=()):
    """Stacked prediction over a library (BASELINE config 5; ``Descriptors/virtualscreening.py`` + ...20250113.py:394-403):
    per batch, the multi-modal network in eval mode, the random forest on ``hstack([fingerprint, image])`` (``trees.ForestGPU``),
    fitted gradient-boosted learners (``boosters``: ``boosters.XGBTrees`` / ``boosters.CatBoostTrees``, the xgb and cat columns of
    ...20250108.py:186-207, on the same hstack) and any precomputed columns go through the linear meta-learner, all on the GPU.  Column order:
    nn, rf, boosters..., extra_columns...
    Returns float64 predictions on the device.  Like the reference, the network attends ACROSS the batch, so its
    column depends on ``batch_size`` and on the order of the library."""
    import torch
    n = fingerprints.shape[0]
    if images.shape[0] != n or any(len(c) != n for c in extra_columns):
        raise ValueError("fingerprints, images and extra columns must have the same number of rows")
    was_training = model.training
    model.eval()
    out = []
    try:
        with torch.no_grad():
            for i in range(0, n, batch_size):
                fp, im = fingerprints[i:i + batch_size], images[i:i + batch_size]
                nn_col = model(fp, im).reshape(-1)
                cols = []
                # the tree learners all read hstack([fingerprint, image]) (805 MB per 4096 molecules): built once per batch
                feats = torch.cat([fp, im], dim=1) if (forest is not None or boosters) else None
                if forest is not None:
                    cols.append(forest.predict_device(feats))
                cols += [bst.predict_device(feats).double() for bst in boosters]
                del feats
                cols += [torch.as_tensor(c[i:i + batch_size], device=nn_col.device) for c in extra_columns]
                out.append(stack.predict_device(nn_col, *cols))
    finally:
        model.train(was_training)
    return torch.cat(out) if out else torch.empty(0, dtype=torch.float64, device=fingerprints.device)


# ---- the classifier stack: StackingClassifier, VotingClassifier and what they share -----------------------------------------------------
STACK_METHODS = ("predict_proba", "decision_function", "predict")
MAX_ENTRIES = MAX_ESTIMATORS = 65535               # BBBP_ENS_MAX_ENTRIES, BBBP_ENS_MAX_ESTIMATORS
_LAUNCHES = {"meta_scatter": 0, "soft_vote": 0, "hard_vote": 0}      # launches of this process (tests and the bench tool count them)


def _ours(obj):
    """Whether ``obj`` is one of this package's estimators: those take CUDA tensors and answer with CUDA tensors."""
    return type(obj).__module__.split(".")[0] == __name__.split(".")[0]


def _clone(est):
    """An unfitted estimator with ``est``'s parameters (``sklearn.base.clone`` without its identity test, which a parameter that the
    constructor normalises, such as a device, does not pass)."""
    if not hasattr(est, "get_params") or not hasattr(est, "fit"):
        raise TypeError(f"ensemble: {type(est).__name__} lacks fit or get_params and cannot be cloned")
    return type(est)(**est.get_params(deep=False))


def _check_device(device, who):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: device {device!r}: the stack is fitted and assembled on the GPU (no CPU fallback)")
    return dev


def _check_n_jobs(n_jobs, who):
    if n_jobs is not None and not (isinstance(n_jobs, numbers.Integral) and not isinstance(n_jobs, bool) and n_jobs == 1):
        raise NotImplementedError(f"{who}: n_jobs={n_jobs!r} is not supported (only None or 1: one learner's fits run side by side on the GPU)")


def _check_estimators(estimators, who):
    """(names, estimators) of a list of (name, estimator) pairs, as scikit-learn checks them; ``"drop"`` is refused."""
    try:
        pairs = [(name, est) for name, est in estimators]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: estimators must be a non-empty list of (name, estimator) pairs") from None
    if not pairs:
        raise ValueError(f"{who}: estimators must be a non-empty list of (name, estimator) pairs")
    if len(pairs) > MAX_ESTIMATORS:
        raise ValueError(f"{who}: {len(pairs)} estimators, at most {MAX_ESTIMATORS} are supported (BBBP_ENS_MAX_ESTIMATORS)")
    names = [name for name, _ in pairs]
    if not all(isinstance(name, str) for name in names) or len(set(names)) != len(names) or any("__" in name for name in names):
        raise ValueError(f"{who}: estimator names must be distinct strings without '__', got {names!r}")
    for name, est in pairs:
        if est is None or (isinstance(est, str) and est == "drop"):
            raise NotImplementedError(f"{who}: estimator {name!r} is {est!r}: dropped estimators are not supported (leave it out of the list)")
        if not hasattr(est, "fit") or not hasattr(est, "get_params") or not any(hasattr(est, m) for m in STACK_METHODS):
            raise TypeError(f"{who}: estimator {name!r} ({type(est).__name__}) needs fit, get_params and one of {STACK_METHODS}")
    return names, [est for _, est in pairs]


def _check_cv(cv, who):
    """An int >= 2 or a list of (train, test) index pairs; everything else is refused by name."""
    if isinstance(cv, str):
        raise NotImplementedError(f"{who}: cv={cv!r} is not supported (an int or a list of (train, test) index pairs; prefitted base learners "
                                  "are not taken over)")
    if isinstance(cv, numbers.Integral) and not isinstance(cv, bool):
        if cv < 2:
            raise ValueError(f"{who}: cv must be at least 2, got {cv}")
        return
    if isinstance(cv, (list, tuple)) and cv and all(isinstance(p, (list, tuple)) and len(p) == 2 for p in cv):
        return
    raise NotImplementedError(f"{who}: cv={cv!r} is not supported: pass an int (StratifiedKFold without shuffling) or a list of "
                              "(train, test) index pairs")


def _check_weights(weights, n_estimators, who):
    """The weights as a float64 vector and their sum as ``np.average`` forms it, or (None, None)."""
    if weights is None:
        return None, None
    try:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: weights must be numbers, got {weights!r}") from None
    if len(w) != n_estimators:
        raise ValueError(f"{who}: Number of `estimators` and weights must be equal; got {len(w)} weights, {n_estimators} estimators")
    if not np.isfinite(w).all():
        raise ValueError(f"{who}: weights must be finite, got {weights!r}")
    # numpy sums a contiguous vector of eight or more weights pairwise: the kernel takes numpy's sum, it does not add the weights again
    scl = float(np.asarray(weights).sum(dtype=np.float64))
    if scl == 0.0:
        raise ZeroDivisionError(f"{who}: Weights sum to zero, can't be normalized")
    return w, scl


def _encode(y, who):
    """(classes_, t int64 in {0, 1}): scikit-learn's LabelEncoder for two classes."""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{who}: y must be 1-D, got shape {y.shape}")
    classes, t = np.unique(y, return_inverse=True)
    if len(classes) != 2:
        raise NotImplementedError(f"{who}: {len(classes)} classes in y, exactly two are supported")
    return classes, t.astype(np.int64)


def _folds(cv, t, who):
    """The (train, test) pairs as int64 arrays whose test parts partition the rows: scikit-learn's ``StratifiedKFold(cv)`` without
    shuffling for an int (taken from scikit-learn, as the grid searches of the other modules take theirs), or the given pairs."""
    n = len(t)
    _check_cv(cv, who)
    if isinstance(cv, numbers.Integral):
        from sklearn.model_selection import StratifiedKFold
        cv = list(StratifiedKFold(n_splits=int(cv)).split(np.zeros((n, 1)), t))
    try:
        pairs = [(np.asarray(tr).reshape(-1), np.asarray(te).reshape(-1)) for tr, te in cv]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: cv must be an int or a list of (train, test) index pairs") from None
    for tr, te in pairs:
        for part in (tr, te):
            if part.dtype.kind not in "iu" or len(part) == 0 or part.min() < 0 or part.max() >= n:
                raise ValueError(f"{who}: cv: a fold's row ids must be a non-empty integer array inside [0, {n})")
    seen = np.bincount(np.concatenate([te for _, te in pairs]), minlength=n)
    if (seen != 1).any():
        raise ValueError(f"{who}: cv: the test parts must partition the rows (every row in exactly one test part)")
    return [(tr.astype(np.int64), te.astype(np.int64)) for tr, te in pairs]


def _resolve_stack_method(est, stack_method, name, who):
    if stack_method == "auto":
        for method in STACK_METHODS:
            if hasattr(est, method):
                return method
        raise ValueError(f"{who}: estimator {name!r} has none of {STACK_METHODS}")
    if not hasattr(est, stack_method):
        raise ValueError(f"{who}: Underlying estimator {name} does not implement the method {stack_method}.")
    return stack_method


def _subset(X_dev, t, rows):
    """The rows ``rows`` (None: all) of the device matrix, gathered on the device, and of the encoded labels."""
    if rows is None:
        return X_dev, t
    return X_dev.index_select(0, torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(X_dev.device)), t[rows]


def _batched_path(est):
    """The name of the list-of-problems path ``_fit_rows`` takes for ``est``, or None when its fits are looped.  A subclass that brings a
    ``fit`` of its own is looped: its fits go through that ``fit``."""
    from . import cat, gradient_boosting, linear_model, mlp, naive_bayes, random_forest, xgb
    for cls, path in ((random_forest.RandomForestClassifier, "random_forest._grow"), (gradient_boosting.GradientBoostingClassifier, "gradient_boosting._fit_chains"),
                      (mlp.MLPClassifier, "GridMLPTrainer.fit"), (naive_bayes.BernoulliNB, "naive_bayes.fit_masks"), (linear_model.LogisticRegression, "linear_model._solve"),
                      (xgb.XGBClassifier, "xgb._fit_classifiers"), (cat.CatBoostClassifier, "cat._fit_classifiers")):
        if isinstance(est, cls) and type(est).fit is cls.fit:
            return path
    return None


def _fit_rows(estimator, X_dev, t, row_sets):
    """One fitted clone of ``estimator`` per entry of ``row_sets`` (int64 row ids into ``X_dev``, None: all rows) on the encoded labels
    ``t``: through the learner's own list-of-problems path where it has one (``_batched_path``; each module keeps that path next to its
    ``fit``, which goes through it too), so that the fits of one learner run side by side and each equals the one-at-a-time fit bit for
    bit; looped otherwise.  Learners of this package get row-gathered device tensors, foreign ones the rows on the host."""
    from . import cat, gradient_boosting, linear_model, mlp, naive_bayes, random_forest, xgb
    path = _batched_path(estimator)
    clones = [_clone(estimator) for _ in row_sets]
    if path == "naive_bayes.fit_masks":                  # row masks over the one packed matrix: nothing is gathered
        e = estimator
        models = naive_bayes.fit_masks(X_dev, t, row_sets, [e.binarize], [e.alpha], fit_prior=e.fit_prior, class_prior=e.class_prior,
                                       force_alpha=e.force_alpha, device=e.device, who=e._who)
        for c, m in zip(clones, models):
            c._adopt(m.classes_, m.feature_count_, m.class_count_, m.feature_log_prob_, m.class_log_prior_, m._w, m._c)
        return clones
    if path == "GridMLPTrainer.fit":                     # the kernel gathers the rows itself
        return mlp.MLPClassifier._fit_rows(clones, X_dev, t, row_sets)
    X_host = None if _ours(estimator) else X_dev.cpu().numpy()
    problems = [_subset(X_dev, t, rows) if X_host is None else ((X_host, t) if rows is None else (X_host[rows], t[rows])) for rows in row_sets]
    if path is None:
        for c, (Xr, tr) in zip(clones, problems):
            c.fit(Xr, tr)
    else:
        module = {"random_forest._grow": random_forest, "gradient_boosting._fit_chains": gradient_boosting, "linear_model._solve": linear_model,
                  "xgb._fit_classifiers": xgb, "cat._fit_classifiers": cat}[path]
        module._fit_classifiers(clones, problems)
    return clones


def _fit_base(estimators, X_dev, t, pairs):
    """Per estimator the fitted clones [all rows, fold 0's training rows, fold 1's, ...]: one ``_fit_rows`` call per learner."""
    row_sets = [None] + [tr for tr, _ in pairs]
    return [_fit_rows(est, X_dev, t, row_sets) for est in estimators]


def _check_classes(fitted, name, who):
    classes = getattr(fitted, "classes_", None)
    if classes is None or not np.array_equal(np.asarray(classes), np.array([0, 1])):
        raise ValueError(f"{who}: estimator {name!r} was fitted on the encoded labels 0 / 1 and reports classes_ = {classes!r}: its classes must "
                         "equal the ensemble's")


def _upload(X, dev, who):
    """(X on the device as float32 / float64 [n, d] with dense rows, was_numpy): the one upload of a call."""
    X, was_numpy = _dense.to_device_matrix(X, dev, who, allow_row_stride=False)
    if X.shape[1] < 1:
        raise ValueError(f"{who}: X must have at least one feature, got shape {tuple(X.shape)}")
    return X, was_numpy


def _device_f64(values, dev):
    """What a learner's prediction method returned as a float64 tensor on the device (a foreign learner answers on the host)."""
    if not isinstance(values, torch.Tensor):
        values = torch.from_numpy(np.ascontiguousarray(np.asarray(values), dtype=np.float64))
    return values.to(dev, torch.float64)


def _query(est, X_dev):
    """The queries as ``est`` takes them: the device tensor for this package's learners, a host copy otherwise."""
    return X_dev if _ours(est) else X_dev.cpu().numpy()


def _column(est, method, X_dev):
    """(float64 device tensor, column): where one learner's meta column for the rows of ``X_dev`` stands -- column 1 of a
    ``predict_proba``, the values of a ``decision_function`` or of a ``predict``."""
    out = _device_f64(getattr(est, method)(_query(est, X_dev)), X_dev.device)
    m = X_dev.shape[0]
    if method == "predict_proba":
        if out.dim() != 2 or tuple(out.shape) != (m, 2):
            raise ValueError(f"ensemble: {type(est).__name__}.predict_proba returned shape {tuple(out.shape)}, expected {(m, 2)}")
        return out, 1
    out = out.reshape(-1)
    if out.numel() != m:
        raise ValueError(f"ensemble: {type(est).__name__}.{method} returned {out.numel()} values for {m} rows")
    return out, 0


def _strides(t, width):
    """(tensor, row stride in elements) of a 1-D vector or a 2-D matrix whose rows hold ``width`` adjacent elements from the column on."""
    if t.dim() == 1:
        return t, (t.stride(0) if t.numel() > 1 else 1)
    if t.dim() != 2:
        raise ValueError(f"ensemble: a source must be 1-D or 2-D, got shape {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1])


def _meta_scatter(entries, meta, n_columns):
    """``bbbp_ens_meta_scatter``: ``entries`` is a list of (float64 device source, column, destination row ids on the host or None for
    row i to row i, destination column); ``meta`` [n, >= n_columns] float64 with unit inner stride receives every cell of its first
    ``n_columns`` columns exactly once.  One launch."""
    dev = meta.device
    n = meta.shape[0]
    table, keep, ids = [], [], []
    for src, col, rows, dst in entries:
        if src.dtype != torch.float64 or src.device != dev:
            raise ValueError("ensemble: a source must be a float64 tensor on the destination's device")
        src, stride = _strides(src, 1)
        count = src.shape[0]
        rows_d = None
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if len(rows) != count:
                raise ValueError(f"ensemble: a source of {count} rows came with {len(rows)} row ids")
            rows_d = torch.from_numpy(rows).to(dev)
            ids.append(rows)
        keep += [src, rows_d]
        table.append(_lib.EnsSource(src.data_ptr() if count else None, stride, col, None if rows_d is None else rows_d.data_ptr(), count, dst))
    if not 1 <= len(table) <= MAX_ENTRIES:
        raise ValueError(f"ensemble: {len(table)} (estimator, fold) entries, 1 .. {MAX_ENTRIES} are supported (BBBP_ENS_MAX_ENTRIES)")
    if meta.dtype != torch.float64 or meta.dim() != 2 or (meta.shape[1] > 1 and meta.stride(1) != 1):
        raise ValueError("ensemble: the destination must be a float64 matrix with unit inner stride")
    arr = (_lib.EnsSource * len(table))(*table)
    ids_host = np.concatenate(ids) if ids else None
    with torch.cuda.device(dev):
        on_device = _tree_host.upload(arr, dev)
        _lib.check(_lib.lib().bbbp_ens_meta_scatter(_dense.stream(), arr, on_device.data_ptr(), len(table),
                                                    None if ids_host is None else ids_host.ctypes.data_as(ctypes.POINTER(ctypes.c_long)), n, n_columns,
                                                    meta.data_ptr() if n else None, _dense.ld(meta)), "bbbp_ens_meta_scatter")
    if n:
        _LAUNCHES["meta_scatter"] += 1
    del keep, on_device
    return meta


def _columns_table(sources, width, dev):
    """The ctypes table of a vote's columns, its copy on the device and what both point to."""
    table, keep = [], []
    for src, col in sources:
        src, stride = _strides(src, width)
        keep.append(src)
        table.append(_lib.EnsColumn(src.data_ptr() if src.numel() else None, stride, col))
    arr = (_lib.EnsColumn * len(table))(*table)
    return arr, _tree_host.upload(arr, dev), keep


def _weights_device(weights, dev):
    return None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(dev)


def _soft_vote(probas, weights=None, scl=None, cols=None):
    """``bbbp_ens_soft_vote`` over M float64 device matrices whose columns ``cols[j]``, ``cols[j] + 1`` (default 0, 1) hold the pair:
    (average [m, 2] float64, label [m] uint8) on the device.  ``weights``: M float64 numbers with ``scl`` their sum as numpy forms it."""
    M = len(probas)
    if not 1 <= M <= MAX_ESTIMATORS:
        raise ValueError(f"ensemble: {M} estimators, 1 .. {MAX_ESTIMATORS} are supported (BBBP_ENS_MAX_ESTIMATORS)")
    dev, m = probas[0].device, probas[0].shape[0]
    cols = [0] * M if cols is None else list(cols)
    for p in probas:
        if p.dtype != torch.float64 or p.device != dev or p.dim() != 2 or p.shape[0] != m:
            raise ValueError("ensemble: the probabilities must be float64 [m, 2] matrices of one length on one device")
    if weights is not None and (len(weights) != M or scl is None):
        raise ValueError("ensemble: one weight per estimator and their sum are needed")
    with torch.cuda.device(dev):
        out = torch.empty((m, 2), dtype=torch.float64, device=dev)
        label = torch.empty(m, dtype=torch.uint8, device=dev)
        arr, on_device, keep = _columns_table(list(zip(probas, cols)), 2, dev)
        w_d = _weights_device(weights, dev)
        _lib.check(_lib.lib().bbbp_ens_soft_vote(_dense.stream(), arr, on_device.data_ptr(), M, None if w_d is None else w_d.data_ptr(),
                                                 0.0 if scl is None else float(scl), m, out.data_ptr() if m else None, label.data_ptr() if m else None),
                   "bbbp_ens_soft_vote")
    if m:
        _LAUNCHES["soft_vote"] += 1
    del keep, on_device, w_d
    return out, label


def _hard_vote(predictions, weights=None, cols=None):
    """``bbbp_ens_hard_vote`` over M uint8 device vectors (or matrices with the prediction in column ``cols[j]``) of 0 / 1 predictions:
    (counts [m, 2] float64, label [m] uint8) on the device."""
    M = len(predictions)
    if not 1 <= M <= MAX_ESTIMATORS:
        raise ValueError(f"ensemble: {M} estimators, 1 .. {MAX_ESTIMATORS} are supported (BBBP_ENS_MAX_ESTIMATORS)")
    dev, m = predictions[0].device, predictions[0].shape[0]
    cols = [0] * M if cols is None else list(cols)
    for p in predictions:
        if p.dtype != torch.uint8 or p.device != dev or p.shape[0] != m:
            raise ValueError("ensemble: the predictions must be uint8 tensors of one length on one device")
    if weights is not None and len(weights) != M:
        raise ValueError("ensemble: one weight per estimator is needed")
    with torch.cuda.device(dev):
        counts = torch.empty((m, 2), dtype=torch.float64, device=dev)
        label = torch.empty(m, dtype=torch.uint8, device=dev)
        arr, on_device, keep = _columns_table(list(zip(predictions, cols)), 1, dev)
        w_d = _weights_device(weights, dev)
        _lib.check(_lib.lib().bbbp_ens_hard_vote(_dense.stream(), arr, on_device.data_ptr(), M, None if w_d is None else w_d.data_ptr(), m,
                                                 counts.data_ptr() if m else None, label.data_ptr() if m else None), "bbbp_ens_hard_vote")
    if m:
        _LAUNCHES["hard_vote"] += 1
    del keep, on_device, w_d
    return counts, label


class StackingClassifier(_estimator.Params):
    """``StackingClassifier(estimators, final_estimator=None, *, cv=5, stack_method="auto", passthrough=False, device="cuda")``:
    scikit-learn 1.7's names and semantics for two classes.

    ``fit`` takes a numpy array or a CUDA tensor [n, d] and labels of any dtype with two distinct values.  It encodes them through
    ``classes_ = np.unique(y)``, fits a clone of every base learner on all rows (``estimators_``, ``named_estimators_``) and on the
    training rows of every fold, builds the out-of-fold matrix -- one float64 column per learner: P(``classes_[1]``) of a
    ``predict_proba``, else the ``decision_function``, else ``predict`` (``stack_method_``); X's columns behind them with ``passthrough``
    -- and fits a clone of ``final_estimator`` (None: ``linear_model.LogisticRegression()``; the reference's
    ``gradient_boosting.GradientBoostingClassifier(100, 0.1, 3)``) on it and the encoded labels.  ``oof_`` keeps that matrix (not
    scikit-learn's; the final estimator's explanations need it).  ``cv``: an int (``StratifiedKFold`` without shuffling) or a list of
    ``(train, test)`` index pairs whose test parts partition the rows.  ``transform`` returns the full-data learners' columns;
    ``predict_proba``, ``decision_function`` and ``predict`` go through ``final_estimator_``.  Numpy in, numpy out; for a CUDA tensor
    the matrices come back as CUDA tensors and the labels as a numpy array of ``classes_``' dtype.  ``fit_paths_`` names, per learner, the
    list-of-problems path its fits took, or "looped"."""

    _who = "StackingClassifier"
    _params = ("estimators", "final_estimator", "cv", "stack_method", "passthrough", "n_jobs", "device")

    def __init__(self, estimators, final_estimator=None, *, cv=5, stack_method="auto", passthrough=False, n_jobs=None, device="cuda"):
        who = self._who
        _check_estimators(estimators, who)
        _check_cv(cv, who)
        _check_n_jobs(n_jobs, who)
        if stack_method != "auto" and stack_method not in STACK_METHODS:
            raise ValueError(f"{who}: stack_method must be 'auto' or one of {STACK_METHODS}, got {stack_method!r}")
        if not isinstance(passthrough, (bool, np.bool_)):
            raise ValueError(f"{who}: passthrough must be a bool, got {passthrough!r}")
        if final_estimator is not None and (not hasattr(final_estimator, "fit") or not hasattr(final_estimator, "get_params")):
            raise TypeError(f"{who}: final_estimator ({type(final_estimator).__name__}) needs fit and get_params")
        _check_device(device, who)
        self.estimators, self.final_estimator, self.cv, self.stack_method = estimators, final_estimator, cv, stack_method
        self.passthrough, self.n_jobs, self.device = passthrough, n_jobs, device

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        who = self._who
        if sample_weight is not None:
            raise NotImplementedError(f"{who}: sample_weight is not supported")
        names, ests = _check_estimators(self.estimators, who)
        classes, t = _encode(y, who)
        dev = _check_device(self.device, who)
        X_dev, was_numpy = _upload(X, dev, who)
        if X_dev.shape[0] != len(t):
            raise ValueError(f"{who}: X has {X_dev.shape[0]} rows, y has {len(t)}")
        pairs = _folds(self.cv, t, who)
        for name, est in zip(names, ests):               # a learner without the method asked for is refused before anything is fitted
            _resolve_stack_method(est, self.stack_method, name, who)
        return self._finish(classes, t, X_dev, was_numpy, names, ests, _fit_base(ests, X_dev, t, pairs), pairs)

    def _finish(self, classes, t, X_dev, was_numpy, names, ests, fits, pairs):
        """Fitted attributes from the base fits ``fits[j] = [all rows, fold 0, fold 1, ...]``: the out-of-fold matrix in one launch, then
        the final estimator on it."""
        who = self._who
        dev, n, M = X_dev.device, X_dev.shape[0], len(ests)
        if M * len(pairs) > MAX_ENTRIES:
            raise ValueError(f"{who}: {M} estimators x {len(pairs)} folds exceed one launch (BBBP_ENS_MAX_ENTRIES {MAX_ENTRIES})")
        for name, fitted in zip(names, fits):
            for f in fitted:
                _check_classes(f, name, who)
        self.classes_ = classes
        self.estimators_ = [fitted[0] for fitted in fits]
        self.named_estimators_ = dict(zip(names, self.estimators_))
        self.stack_method_ = [_resolve_stack_method(est, self.stack_method, name, who) for name, est in zip(names, self.estimators_)]
        self.fit_paths_ = {name: _batched_path(est) or "looped" for name, est in zip(names, ests)}
        self.n_features_in_ = int(X_dev.shape[1])
        with torch.cuda.device(dev):
            meta = torch.empty((n, M + (self.n_features_in_ if self.passthrough else 0)), dtype=torch.float64, device=dev)
            entries = []
            for f, (_, te) in enumerate(pairs):
                X_te = X_dev.index_select(0, torch.from_numpy(te).to(dev))          # gathered once per fold, shared by the learners
                for j, method in enumerate(self.stack_method_):
                    entries.append(_column(fits[j][1 + f], method, X_te) + (te, j))
            _meta_scatter(entries, meta, M)
            if self.passthrough:
                meta[:, M:] = X_dev
            final = _clone(self.final_estimator) if self.final_estimator is not None else self._default_final()
            self.final_estimator_ = final.fit(meta if _ours(final) else meta.cpu().numpy(), t)
        self.oof_ = meta.cpu().numpy() if was_numpy else meta
        return self

    def _default_final(self):
        from .linear_model import LogisticRegression
        return LogisticRegression(device=self.device)

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _meta(self, X):
        """(the full-data learners' columns for X, float64 [m, M (+ d)] on the device; was_numpy): one upload, one launch."""
        who = self._who
        if not hasattr(self, "final_estimator_"):
            raise RuntimeError(f"{who}: not fitted")
        dev = _check_device(self.device, who)
        X_dev, was_numpy = _upload(X, dev, who)
        if X_dev.shape[1] != self.n_features_in_:
            raise ValueError(f"{who}: X has {X_dev.shape[1]} features, the fit saw {self.n_features_in_}")
        m, M = X_dev.shape[0], len(self.estimators_)
        with torch.cuda.device(dev):
            meta = torch.empty((m, M + (self.n_features_in_ if self.passthrough else 0)), dtype=torch.float64, device=dev)
            if m:
                _meta_scatter([_column(est, method, X_dev) + (None, j) for j, (est, method) in enumerate(zip(self.estimators_, self.stack_method_))],
                              meta, M)
                if self.passthrough:
                    meta[:, M:] = X_dev
        return meta, was_numpy

    def transform(self, X):
        meta, was_numpy = self._meta(X)
        return meta.cpu().numpy() if was_numpy else meta

    def _final(self, method, X):
        meta, was_numpy = self._meta(X)
        ours = _ours(self.final_estimator_)
        out = getattr(self.final_estimator_, method)(meta if ours else meta.cpu().numpy())
        if was_numpy:
            return out.cpu().numpy() if isinstance(out, torch.Tensor) else out
        return out if isinstance(out, torch.Tensor) else torch.from_numpy(np.asarray(out)).to(meta.device)

    def predict_proba(self, X):
        return self._final("predict_proba", X)

    def decision_function(self, X):
        return self._final("decision_function", X)

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype: the final estimator's prediction, decoded."""
        meta, _ = self._meta(X)
        pred = self.final_estimator_.predict(meta if _ours(self.final_estimator_) else meta.cpu().numpy())
        return self.classes_[np.asarray(pred).astype(np.intp)]


class VotingClassifier(_estimator.Params):
    """``VotingClassifier(estimators, *, voting="hard", weights=None, flatten_transform=True, device="cuda")``: scikit-learn 1.7's names
    and semantics for two classes.

    ``fit`` encodes the labels through ``classes_ = np.unique(y)`` and fits a clone of every learner on all rows (``estimators_``,
    ``named_estimators_``).  Soft voting: ``predict_proba`` is ``np.average`` of the learners' probabilities over the estimator axis --
    ``s = P_0 (* w_0)``, ``s = s + P_j (* w_j)`` in estimator order, divided by the sum of the weights as numpy forms it (by M without
    weights), every operation rounded on its own -- and ``predict`` its first maximum.  Hard voting: per row the float64 sum, in estimator
    order, of the weights (1.0 without) of the learners that predict each class, as ``np.bincount(weights=)`` adds them; the first
    maximum wins, so ties go to ``classes_[0]``.  ``transform`` is scikit-learn's: the probabilities side by side [m, 2 M]
    (``flatten_transform=False``: [M, m, 2]) for soft voting, the encoded predictions [m, M] for hard voting.  Numpy in, numpy out; for a
    CUDA tensor probabilities come back as CUDA tensors and labels as a numpy array of ``classes_``' dtype."""

    _who = "VotingClassifier"
    _params = ("estimators", "voting", "weights", "flatten_transform", "n_jobs", "device")

    def __init__(self, estimators, *, voting="hard", weights=None, flatten_transform=True, n_jobs=None, device="cuda"):
        who = self._who
        names, _ = _check_estimators(estimators, who)
        if voting not in ("soft", "hard"):
            raise ValueError(f"{who}: Voting must be 'soft' or 'hard'; got (voting={voting!r})")
        _check_weights(weights, len(names), who)
        if not isinstance(flatten_transform, (bool, np.bool_)):
            raise ValueError(f"{who}: flatten_transform must be a bool, got {flatten_transform!r}")
        _check_n_jobs(n_jobs, who)
        _check_device(device, who)
        self.estimators, self.voting, self.weights, self.flatten_transform = estimators, voting, weights, flatten_transform
        self.n_jobs, self.device = n_jobs, device

    def fit(self, X, y, sample_weight=None):
        who = self._who
        if sample_weight is not None:
            raise NotImplementedError(f"{who}: sample_weight is not supported")
        names, ests = _check_estimators(self.estimators, who)
        _check_weights(self.weights, len(ests), who)
        classes, t = _encode(y, who)
        dev = _check_device(self.device, who)
        X_dev, _ = _upload(X, dev, who)
        if X_dev.shape[0] != len(t):
            raise ValueError(f"{who}: X has {X_dev.shape[0]} rows, y has {len(t)}")
        return self._finish(classes, names, ests, [fitted[0] for fitted in _fit_base(ests, X_dev, t, [])], int(X_dev.shape[1]))

    def _finish(self, classes, names, ests, fitted, n_features):
        who = self._who
        for name, f in zip(names, fitted):
            _check_classes(f, name, who)
            need = "predict_proba" if self.voting == "soft" else "predict"
            if not hasattr(f, need):
                raise ValueError(f"{who}: estimator {name!r} has no {need}, which voting={self.voting!r} needs")
        self.classes_, self.estimators_, self.named_estimators_ = classes, list(fitted), dict(zip(names, fitted))
        self.fit_paths_ = {name: _batched_path(est) or "looped" for name, est in zip(names, ests)}
        self.n_features_in_ = n_features
        return self

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _queries(self, X):
        who = self._who
        if not hasattr(self, "estimators_"):
            raise RuntimeError(f"{who}: not fitted")
        X_dev, was_numpy = _upload(X, _check_device(self.device, who), who)
        if X_dev.shape[1] != self.n_features_in_:
            raise ValueError(f"{who}: X has {X_dev.shape[1]} features, the fit saw {self.n_features_in_}")
        return X_dev, was_numpy

    def _probas(self, X_dev):
        return [_column(est, "predict_proba", X_dev)[0] for est in self.estimators_]

    def _predictions(self, X_dev):
        """The learners' encoded predictions as uint8 [M, m] on the host."""
        out = np.empty((len(self.estimators_), X_dev.shape[0]), dtype=np.uint8)
        for j, est in enumerate(self.estimators_):
            pred = np.asarray(est.predict(_query(est, X_dev)))
            if not np.isin(pred, (0, 1)).all():
                raise ValueError(f"{self._who}: {type(est).__name__}.predict returned labels outside the encoded classes 0 / 1")
            out[j] = pred
        return out

    def _vote(self, X_dev):
        w, scl = _check_weights(self.weights, len(self.estimators_), self._who)
        if self.voting == "soft":
            return _soft_vote(self._probas(X_dev), w, scl)
        preds = torch.from_numpy(self._predictions(X_dev)).to(X_dev.device)
        return _hard_vote(list(preds), w)

    def predict_proba(self, X):
        if self.voting == "hard":
            raise AttributeError(f"predict_proba is not available when voting={self.voting!r}")
        X_dev, was_numpy = self._queries(X)
        avg, _ = self._vote(X_dev)
        return avg.cpu().numpy() if was_numpy else avg

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype: the first maximum of the vote."""
        X_dev, _ = self._queries(X)
        return self.classes_[self._vote(X_dev)[1].cpu().numpy().astype(np.intp)]

    def transform(self, X):
        X_dev, was_numpy = self._queries(X)
        if self.voting == "hard":
            return self._predictions(X_dev).T.astype(np.int64)
        probas = self._probas(X_dev)
        out = torch.cat(probas, dim=1) if self.flatten_transform else torch.stack(probas)
        return out.cpu().numpy() if was_numpy else out


def fit_classifier_stack(estimators, X, y, final_estimator=None, cv=5, weights=None, voting="soft", device="cuda"):
    """``(StackingClassifier(estimators, final_estimator, cv=cv).fit(X, y), VotingClassifier(estimators, voting=voting,
    weights=weights).fit(X, y))`` from one upload of X, one set of full-data fits and one set of fold fits: per learner one ``_fit_rows``
    call over all rows and every fold's training rows.  The two models share their fitted full-data learners and equal, bit for bit, the
    ones their own ``fit`` gives."""
    who = "ensemble.fit_classifier_stack"
    stacking = StackingClassifier(estimators, final_estimator, cv=cv, device=device)
    vote = VotingClassifier(estimators, voting=voting, weights=weights, device=device)
    names, ests = _check_estimators(estimators, who)
    classes, t = _encode(y, who)
    dev = _check_device(device, who)
    X_dev, was_numpy = _upload(X, dev, who)
    if X_dev.shape[0] != len(t):
        raise ValueError(f"{who}: X has {X_dev.shape[0]} rows, y has {len(t)}")
    pairs = _folds(cv, t, who)
    fits = _fit_base(ests, X_dev, t, pairs)
    stacking._finish(classes, t, X_dev, was_numpy, names, ests, fits, pairs)
    vote._finish(classes, names, ests, [fitted[0] for fitted in fits], int(X_dev.shape[1]))
    return stacking, vote
