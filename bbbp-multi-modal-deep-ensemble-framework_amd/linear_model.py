"""``sklearn.linear_model.LogisticRegression`` for the GPU: binary, L2-penalised, float64, solved by a batched damped Newton iteration.

The classification stack of the reference (``Models/model_opt_maccs.py:124-180``) searches ``LogisticRegression(max_iter=1000)`` over
``C in {0.1, 1, 10}``, ``penalty='l2'`` under ``GridSearchCV(cv=5, scoring='f1')``, behind StandardScaler, ``PCA(100)`` and SMOTE.  The
entry points of ``csrc/logreg.hip`` carry it:

* a round of the solver is three launches over all problems of a batch: the row pass (z = X w + b, residual, curvature and per-block
  partial sums of the loss, the gradient and the Hessian's intercept row), the weighted Gram matrix ``X^T diag(w) X`` on the float64
  matrix pipe (the tile product ``decomposition``, ``neighbors`` and ``svm`` share, with one extra factor per row), and the step (one
  work-group per problem: scikit-learn's ``NewtonSolver`` accept / reject rule, convergence test, Cholesky factorisation and solve);
* the host enqueues ``ROUNDS_PER_SYNC`` rounds per read of the done flags; finished problems leave every kernel at once;
* the decision function is the row pass's dot product, so decision values of training rows are bitwise those the solver saw.

The objective is scikit-learn's, with its scaling, ``f(w, b) = 1/n sum log(1 + exp(-y_i z_i)) + |w|^2 / (2 C n)``, and a fit stops once
``max |grad f| <= tol``.  It is strictly convex: the optimum is unique and does not depend on the solver, which is why ``solver="lbfgs"``
(scikit-learn's default, what the reference gets) and ``solver="newton-cholesky"`` both run the one Newton solver here.  Results are
bit-identical from run to run and do not depend on what else is solved in the same batch.

Out of scope: penalties other than ``"l2"``, ``class_weight``, sample weights, more than two classes, more than 255 features, more
than one GPU.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import numbers
import warnings

import numpy as np
import torch

from . import _estimator, _dense, _lib

SOLVERS = ("lbfgs", "newton-cholesky")
MAX_FEATURES = 255                         # BBBP_LOGREG_MAX_D
ROUNDS_PER_SYNC = 4                        # rounds enqueued per host read of the done flags: DESIGN.md gives the reason
STATUS = {0: "converged", 1: "max_iter", 2: "line search failed", 3: "non-positive Cholesky pivot"}      # BBBP_LOGREG_*


def _check_params(C, tol, max_iter, fit_intercept, penalty, solver, who="LogisticRegression"):
    if isinstance(C, bool) or not isinstance(C, numbers.Real) or not (0.0 < float(C) < float("inf")):
        raise ValueError(f"{who}: C must be a positive finite number, got {C!r}")
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not (0.0 < float(tol) < float("inf")):
        raise ValueError(f"{who}: tol must be a positive finite number, got {tol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 1:
        raise ValueError(f"{who}: max_iter must be a positive int, got {max_iter!r}")
    if not isinstance(fit_intercept, (bool, np.bool_)):
        raise ValueError(f"{who}: fit_intercept must be a bool, got {fit_intercept!r}")
    if penalty != "l2":
        raise ValueError(f"{who}: penalty must be 'l2', got {penalty!r}")
    if solver not in SOLVERS:
        raise ValueError(f"{who}: solver must be one of {SOLVERS}, got {solver!r}")


def _binary_targets(y, n, who="LogisticRegression"):
    """(classes, t in {0.0, 1.0} float64): 1 marks ``classes[1]``, the positive class."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{who}: y must be 1-D, got shape {y.shape}")
    if n is not None and len(y) != n:
        raise ValueError(f"{who}: X has {n} rows, y has {len(y)}")
    classes = np.unique(y)
    if len(classes) != 2:
        raise ValueError(f"{who}: {len(classes)} classes in y, exactly two are supported")
    return classes, np.where(y == classes[1], 1.0, 0.0)


def _check_finite(X, what):
    """ValueError when X holds NaN or infinity (bbbp_knn_row_norms' flag: one host read)."""
    n, d = X.shape
    norms = torch.empty(n, dtype=torch.float64, device=X.device)
    flag = torch.zeros(1, dtype=torch.int32, device=X.device)
    _lib.check(_lib.lib().bbbp_knn_row_norms(_dense.stream(), X.data_ptr(), _dense.DT[X.dtype], n, d, _dense.ld(X), None, norms.data_ptr(),
                                             flag.data_ptr()), "bbbp_knn_row_norms")
    if int(flag.item()):
        raise ValueError(f"linear_model: {what} contains NaN or infinity (or values whose squares overflow float64)")


def _check_shape(X, who):
    n, d = X.shape
    if n < 1 or d < 1:
        raise ValueError(f"{who}: need at least one row and one feature, got shape {(n, d)}")
    if d > MAX_FEATURES:
        raise ValueError(f"{who}: {d} features, at most {MAX_FEATURES} are supported")


class _Problem:
    """One problem on the device: the point, the solver's state and the descriptor ``bbbp_logreg_rounds`` takes.  Everything starts zeroed:
    theta = 0 is the starting point."""

    def __init__(self, X, t_d, C, tol, max_iter, fit_intercept):
        dev = X.device
        n, d = X.shape
        L = _lib.lib()
        nbytes = L.bbbp_logreg_state_bytes(n, d)
        if not nbytes:
            raise ValueError("linear_model: " + L.bbbp_last_error().decode("utf-8", "replace"))
        self.X, self.t, self.n, self.d = X, t_d, n, d
        self.theta = torch.zeros(d + 1, dtype=torch.float64, device=dev)
        self.trial = torch.zeros(d + 1, dtype=torch.float64, device=dev)
        self.state = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
        self.flags = torch.zeros(4, dtype=torch.int32, device=dev)       # n_iter, status, done, trials
        self.desc = _lib.LogregProblem(X.data_ptr(), _dense.DT[X.dtype], _dense.ld(X), n, d, t_d.data_ptr(), float(C), float(tol), int(bool(fit_intercept)),
                                       int(max_iter), self.theta.data_ptr(), self.trial.data_ptr(), self.state.data_ptr(), self.flags.data_ptr())


def _solve(problems, rounds_per_sync=None):
    """Run ``bbbp_logreg_rounds`` until every problem is done.  Returns per problem (n_iter, status).  A problem ends by itself: converged,
    ``max_iter`` accepted steps, a failed line search (21 evaluations) or a failed factorisation, so the loop is bounded."""
    per = int(rounds_per_sync or ROUNDS_PER_SYNC)
    L = _lib.lib()
    state = [None] * len(problems)
    live = list(range(len(problems)))
    while live:
        arr = (_lib.LogregProblem * len(live))(*[problems[q].desc for q in live])
        _lib.check(L.bbbp_logreg_rounds(_dense.stream(), arr, len(live), per), "bbbp_logreg_rounds")
        flags = torch.stack([problems[q].flags for q in live]).cpu().numpy()      # the host read that ends the rounds
        for q, (n_iter, status, done, _) in zip(live, flags):
            state[q] = (int(n_iter), int(status), bool(done))
        live = [q for q in live if not state[q][2]]
    return [(s[0], s[1]) for s in state]


def _evaluate(X, t, theta, C=1.0, fit_intercept=True, device="cuda"):
    """``bbbp_logreg_eval`` at ``theta`` [d + 1] (w, b): dict of the loss, the gradient [p], the Hessian [p, p] (p = d + fit_intercept) and
    z, r, w [n], as numpy float64.  What the tests compare with the numpy oracle; ``fit`` does not use it."""
    dev = torch.device(device)
    X, _ = _dense.to_device_matrix(X, dev, "linear_model", allow_row_stride=True)
    _check_shape(X, "linear_model")
    n, d = X.shape
    with torch.cuda.device(dev):
        pr = _Problem(X, torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev), C, 1.0, 1, fit_intercept)
        pr.trial.copy_(torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float64)))
        L = _lib.lib()
        _lib.check(L.bbbp_logreg_eval(_dense.stream(), ctypes.byref(pr.desc)), "bbbp_logreg_eval")
        off = (ctypes.c_long * 6)()
        _lib.check(L.bbbp_logreg_state_layout(n, d, off), "bbbp_logreg_state_layout")
        st = pr.state.cpu().numpy()
    p = d + int(bool(fit_intercept))
    H = np.zeros((p, p))
    H[np.triu_indices(p)] = st[off[5]:off[5] + p * (p + 1) // 2]          # packed by rows: row a holds columns a .. p - 1
    H = H + np.triu(H, 1).T
    return dict(loss=float(st[off[0]]), grad=st[off[1]:off[1] + p].copy(), hess=H, z=st[off[2]:off[2] + n].copy(), r=st[off[3]:off[3] + n].copy(),
                w=st[off[4]:off[4] + n].copy())


class LogisticRegression(_estimator.Params):
    """``LogisticRegression(C=1.0, tol=1e-4, max_iter=100, fit_intercept=True, penalty="l2", solver="lbfgs", *, device="cuda")``:
    scikit-learn's names for two classes.

    ``fit`` takes a CUDA tensor or a numpy array, float32 or float64, [n, d] with d <= 255, and labels of any sortable kind with two
    distinct values; ``classes_[1]`` is the positive class.  It sets ``coef_`` [1, d], ``intercept_`` [1], ``classes_``, ``n_iter_`` [1]
    (the accepted Newton steps) and ``n_features_in_``.  ``decision_function`` returns float64 [m]: a numpy array for numpy input, a CUDA
    tensor for a CUDA tensor; ``predict_proba`` returns [m, 2] as ``[1 - p, p]`` with ``p = expit(decision)``, scikit-learn's binary rule.

    ``solver`` accepts ``"lbfgs"`` and ``"newton-cholesky"``; both run the damped Newton solver of ``csrc/logreg.hip``.  The objective
    is strictly convex, so its optimum is unique: solvers differ in the path, not in where a fit to a tight ``tol`` ends.  ``max_iter``
    counts accepted Newton steps.  Stopping at ``max_iter`` or on a failed line search warns with ``ConvergenceWarning``."""

    def __init__(self, C=1.0, tol=1e-4, max_iter=100, fit_intercept=True, penalty="l2", solver="lbfgs", *, device="cuda", class_weight=None,
                 multi_class=None, **unsupported):
        if unsupported:
            raise ValueError(f"LogisticRegression: unsupported parameters {sorted(unsupported)}")
        if class_weight is not None:
            raise ValueError("LogisticRegression: class_weight is not supported")
        if multi_class is not None:
            raise ValueError("LogisticRegression: multi_class is not supported (two classes only)")
        _check_params(C, tol, max_iter, fit_intercept, penalty, solver)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"LogisticRegression: device {device!r}: the solver runs on the GPU (no CPU fallback)")
        self.C, self.tol, self.max_iter, self.fit_intercept = float(C), float(tol), int(max_iter), bool(fit_intercept)
        self.penalty, self.solver = penalty, solver

    _params = ("C", "tol", "max_iter", "fit_intercept", "penalty", "solver", "device")

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("LogisticRegression: sample weights are not supported")
        _fit_classifiers([self], [(X, y)])
        return self

    def _adopt(self, classes, pr, n_iter, status):
        """Fitted attributes from a solved problem."""
        if status != 0:
            from sklearn.exceptions import ConvergenceWarning
            why = f"max_iter={self.max_iter} Newton steps" if status == 1 else STATUS.get(status, f"status {status}")
            warnings.warn(f"LogisticRegression: solver stopped ({why}) before reaching tol={self.tol}", ConvergenceWarning)
        theta = pr.theta.cpu().numpy()
        self._theta_d = pr.theta
        self.classes_ = classes
        self.coef_ = theta[None, :pr.d].copy()
        self.intercept_ = np.array([theta[pr.d] if self.fit_intercept else 0.0])
        self.n_iter_ = np.array([n_iter], dtype=np.int32)
        self.n_features_in_ = pr.d
        self.fit_status_ = status

    # ---- decision ---------------------------------------------------------------------------------------------------
    def _decision(self, Xq):
        m, d = Xq.shape
        if d != self.n_features_in_:
            raise ValueError(f"linear_model: the queries have {d} features, the fit saw {self.n_features_in_}")
        out = torch.empty(m, dtype=torch.float64, device=self.device)
        if m == 0:
            return out
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bbbp_logreg_decision(_dense.stream(), Xq.data_ptr(), _dense.DT[Xq.dtype], _dense.ld(Xq), m, d, self._theta_d.data_ptr(),
                                                       int(self.fit_intercept), out.data_ptr()), "bbbp_logreg_decision")
        return out

    def _queries(self, X):
        if not hasattr(self, "_theta_d"):
            raise RuntimeError("linear_model: not fitted")
        return _dense.to_device_matrix(X, self.device, "linear_model", allow_row_stride=True)

    def decision_function(self, X):
        """z = X w + b for every row of X; positive means ``classes_[1]``."""
        Xq, was_numpy = self._queries(X)
        out = self._decision(Xq)
        return out.cpu().numpy() if was_numpy else out

    def predict_proba(self, X):
        """[m, 2]: ``[1 - p, p]`` with ``p = expit(decision_function(X))``."""
        Xq, was_numpy = self._queries(X)
        p = torch.special.expit(self._decision(Xq))
        out = torch.stack([1.0 - p, p], dim=1)
        return out.cpu().numpy() if was_numpy else out

    def predict_log_proba(self, X):
        """log of ``predict_proba``, each column from ``logsigmoid`` of the decision value (no log of a rounded probability)."""
        Xq, was_numpy = self._queries(X)
        z = self._decision(Xq)
        out = torch.stack([torch.nn.functional.logsigmoid(-z), torch.nn.functional.logsigmoid(z)], dim=1)
        return out.cpu().numpy() if was_numpy else out

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype (labels need not be numbers, so they stay on the host)."""
        Xq, _ = self._queries(X)
        return self.classes_[(self._decision(Xq) > 0).cpu().numpy().astype(np.intp)]


def _fit_classifiers(classifiers, problems):
    """Solve ``classifiers[i]`` over ``problems[i] = (X, y)`` in one ``_solve`` batch and fit every classifier from its own problem: what
    ``fit`` does, for one or many (``ensemble`` fits a learner on all rows and on every fold's training rows this way).  Each classifier
    equals its single ``fit`` bit for bit."""
    checked = []
    for clf, (X, y) in zip(classifiers, problems):
        classes, t = _binary_targets(y, None)
        X, _ = _dense.to_device_matrix(X, clf.device, "linear_model", allow_row_stride=True)
        if X.shape[0] != len(t):
            raise ValueError(f"LogisticRegression: X has {X.shape[0]} rows, y has {len(t)}")
        _check_shape(X, "LogisticRegression")
        checked.append((classes, t, X))
    with torch.cuda.device(classifiers[0].device):
        solving = []
        for clf, (_, t, X) in zip(classifiers, checked):
            _check_finite(X, "the training set")
            solving.append(_Problem(X, torch.from_numpy(t).to(clf.device), clf.C, clf.tol, clf.max_iter, clf.fit_intercept))
        for clf, pr, (classes, _, _), (n_iter, status) in zip(classifiers, solving, checked, _solve(solving)):
            clf._adopt(classes, pr, n_iter, status)


def grid_search_cv(X, y, param_grid, cv: int = 5, device="cuda", *, tol=1e-4, max_iter=100):
    """The reference's ``GridSearchCV(LogisticRegression(max_iter=1000), param_grid, cv=5, scoring='f1')`` (model_opt_maccs.py:124-180)
    over ``C`` and ``penalty``.

    Same conventions as ``svm.grid_search_cv``: sorted keys, ``itertools.product`` order, scikit-learn's ``StratifiedKFold(cv)``,
    ``f1_score`` of ``classes_[1]``, the first maximum wins; ``param_grid`` is a dict or, as for scikit-learn, a list of dicts.  Each
    fold's training rows are gathered once on the device and every (fold, C) problem is solved in one batch, so every grid point equals
    a single ``LogisticRegression(...).fit`` on that fold bit for bit; the refit follows.
    Returns (best_params, mean F1 per point, the classifier refitted on all rows with best_params)."""
    from itertools import product
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    who = "linear_model.grid_search_cv"
    points = []
    for sub in ([param_grid] if isinstance(param_grid, dict) else list(param_grid)):      # a list of grids: one after the other, as ParameterGrid
        unknown = set(sub) - {"C", "penalty"}
        if unknown:
            raise ValueError(f"{who}: unsupported grid keys {sorted(unknown)}")
        keys = sorted(sub)
        points += [dict(zip(keys, vals)) for vals in product(*(sub[k] for k in keys))]
    if not points:
        raise ValueError(f"{who}: the grid is empty")
    full = [(pt.get("C", 1.0), pt.get("penalty", "l2")) for pt in points]
    for C, penalty in full:
        _check_params(C, tol, max_iter, True, penalty, "lbfgs", who)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: device {device!r}: the solver runs on the GPU (no CPU fallback)")
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    y = np.asarray(y)
    classes, t_all = _binary_targets(y, X.shape[0], who)
    pos = classes[1]
    folds = list(StratifiedKFold(n_splits=cv).split(X, y))
    f1 = np.zeros((len(points), len(folds)))
    with torch.cuda.device(dev):
        X_d = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        _check_shape(X_d, who)
        _check_finite(X_d, "the training set")
        Cs = sorted({float(C) for C, _ in full})
        problems, parts = {}, []
        for fi, (tr, te) in enumerate(folds):
            Xtr, Xte = X_d[torch.from_numpy(tr).to(dev)], X_d[torch.from_numpy(te).to(dev)]      # gathered once per fold
            t_d = torch.from_numpy(t_all[tr]).to(dev)
            parts.append(Xte)
            for C in Cs:
                problems[(fi, C)] = _Problem(Xtr, t_d, C, tol, max_iter, True)
        order = list(problems)
        solved = dict(zip(order, _solve([problems[k] for k in order])))
        for fi, (tr, te) in enumerate(folds):
            preds = {}
            for C in Cs:
                clf = LogisticRegression(C, tol, max_iter, device=dev)
                clf._adopt(classes, problems[(fi, C)], *solved[(fi, C)])
                preds[C] = clf.predict(parts[fi])
            for pi, (C, _) in enumerate(full):
                f1[pi, fi] = f1_score(y[te], preds[float(C)], pos_label=pos)
        del problems, parts
    scores = [float(v) for v in f1.mean(axis=1)]
    best = int(np.argmax(scores))
    fitted = LogisticRegression(full[best][0], tol, max_iter, penalty=full[best][1], device=dev).fit(X, y)
    return points[best], scores, fitted
