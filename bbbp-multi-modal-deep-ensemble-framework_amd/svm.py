"""``sklearn.svm.SVC`` and ``sklearn.svm.SVR`` for the GPU: binary C-support-vector classification and epsilon-support-vector regression in
float64, linear and RBF kernels.

The classification stack of the reference (``Models/model_opt_maccs.py:124-180``) searches ``SVC()`` over ``C in {0.1, 1, 10} x kernel in
{linear, rbf}`` under ``GridSearchCV(cv=5, scoring='f1')``, behind StandardScaler, ``PCA(100)`` and SMOTE.  Three entry points of
``csrc/svm.hip`` carry it:

* the [n, n] kernel matrix is the tile product ``decomposition`` and ``neighbors`` share, with the kernel in the epilogue: X X^T for the
  linear kernel; for RBF the squared distance from rows centred at the training mean, clamped at 0, and ``exp`` while the block is still in
  registers.  The matrix is bitwise symmetric and the RBF diagonal is exactly 1;
* the solver is libsvm's (second-order working-set selection, its clipping, ties to the later index) without shrinking, one work-group per
  problem: all C values of a fold are solved side by side over one matrix, a fold being a row-index list into it.  A launch runs a bounded
  number of iterations (``ITERS_PER_LAUNCH``, fewer in proportion beyond 8 000 rows); the host reads the done flags and launches the unfinished problems again;
* the decision function multiplies the kernel block of 64 queries x 64 support vectors by the coefficients and reduces it inside the kernel.

``SVC``: ``fit`` / ``decision_function`` / ``predict`` with scikit-learn's attributes and sign convention (a positive decision value means
``classes_[1]``); ``grid_search_cv``: the reference's grid, one batch of problems per fold.

``SVR``: epsilon-support-vector regression, the kernel learner of the regression stack
(``Models/multi_input_data_regression_opt_transformer_cnn_opt_more.py:117-149``), over the same matrix and decision function; its 2n-variable
dual is ``bbbp_svr_smo`` of ``csrc/svr.hip``, which keeps a problem's state in registers for a whole launch.  ``fit_svr_folds``: the
reference's five folds in one batch; ``grid_search_cv_svr``: ``GridSearchCV(SVR(), grid)`` with R^2 over unshuffled folds.

Two correct SMO runs of one problem agree to about ``tol``, not to rounding: scikit-learn itself moves by that much between a data set and
its reversal.  Results here are bit-identical from run to run and do not depend on what else is solved in the same batch.

``PlattSVC``: ``SVC(probability=True)`` of the reference's classification scripts (``Models/model_opt_maccs.py:128``), whose ROC AUC, stacking
and soft voting read ``predict_proba``.  libsvm's scheme -- ``cv`` fold problems, their out-of-fold decision values, a sigmoid fitted to
them, one more fit on all rows -- runs over ONE kernel matrix: the fold problems are row lists into it and stand in one solver batch beside
the all-rows problem, ``bbbp_svm_oof_decision`` reads the held-out decision values from the resident matrix, ``bbbp_svm_platt_fit`` is
libsvm's ``sigmoid_train`` in one work-group and ``bbbp_svm_platt_proba`` its ``sigmoid_predict`` (``csrc/svm_proba.hip``).  ``platt_scale``
is the sigmoid fit on its own.  The folds are libsvm's unstratified slices of a permutation, drawn from numpy's generator where libsvm draws
from its own: see ``PlattSVC``.

Out of scope: ``probability=True`` as a mode of ``SVC`` (``PlattSVC`` is the class for it), more than two classes,
``class_weight``, kernels other than linear and RBF, shrinking (accepted and ignored: the optimum is the same), a kernel matrix larger than
free device memory, more than one GPU.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import numbers
import warnings

import numpy as np
import torch

from . import _dense, _estimator, _lib

KERNELS = {"linear": 0, "rbf": 1}          # BBBP_SVM_LINEAR / BBBP_SVM_RBF
ITERS_PER_LAUNCH = 2000                    # iterations per problem and launch up to ITERS_REFERENCE_N rows: DESIGN.md gives the measured time of one
SVR_ITERS_PER_LAUNCH = 2000                # the same for bbbp_svr_smo: 5.3 us an iteration at 850 rows, 27 us at 8 000
ITERS_REFERENCE_N = 8000                   # an iteration reads O(n): beyond this n the count shrinks in proportion, so a launch keeps its length


def _check_params(C, kernel, gamma, tol, max_iter, who="SVC"):
    if isinstance(C, bool) or not isinstance(C, numbers.Real) or not (0.0 < float(C) < float("inf")):
        raise ValueError(f"{who}: C must be a positive finite number, got {C!r}")
    if kernel not in KERNELS:
        raise ValueError(f"{who}: kernel must be 'linear' or 'rbf', got {kernel!r}")
    if isinstance(gamma, str):
        if gamma not in ("scale", "auto"):
            raise ValueError(f"{who}: gamma must be 'scale', 'auto' or a positive number, got {gamma!r}")
    elif isinstance(gamma, bool) or not isinstance(gamma, numbers.Real) or not (0.0 < float(gamma) < float("inf")):
        raise ValueError(f"{who}: gamma must be 'scale', 'auto' or a positive number, got {gamma!r}")
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not (0.0 < float(tol) < float("inf")):
        raise ValueError(f"{who}: tol must be a positive finite number, got {tol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or not (max_iter == -1 or max_iter >= 1):
        raise ValueError(f"{who}: max_iter must be -1 (no limit) or a positive int, got {max_iter!r}")


def _binary_labels(y, n, who="SVC"):
    """(classes, solver y in {+1, -1} float64): libsvm gives +1 to the first of the sorted classes."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{who}: y must be 1-D, got shape {y.shape}")
    if n is not None and len(y) != n:
        raise ValueError(f"{who}: X has {n} rows, y has {len(y)}")
    classes = np.unique(y)
    if len(classes) != 2:
        raise ValueError(f"{who}: {len(classes)} classes in y, exactly two are supported")
    return classes, np.where(y == classes[0], 1.0, -1.0)


def _norms(X, mu, what):
    """bbbp_knn_row_norms of X about mu (None: about 0); ValueError when X holds NaN or infinity (one host read of the flag)."""
    n, d = X.shape
    norms = torch.empty(n, dtype=torch.float64, device=X.device)
    flag = torch.zeros(1, dtype=torch.int32, device=X.device)
    _lib.check(_lib.lib().bbbp_knn_row_norms(_dense.stream(), X.data_ptr(), _dense.DT[X.dtype], n, d, _dense.ld(X), None if mu is None else mu.data_ptr(),
                                             norms.data_ptr(), flag.data_ptr()), "bbbp_knn_row_norms")
    if int(flag.item()):
        raise ValueError(f"svm: {what} contains NaN or infinity (or values whose squares overflow float64)")
    return norms


def _col_mean(X):
    n, d = X.shape
    mean = torch.empty(d, dtype=torch.float64, device=X.device)
    _lib.check(_lib.lib().bbbp_pca_col_mean(_dense.stream(), X.data_ptr(), _dense.DT[X.dtype], n, d, _dense.ld(X), mean.data_ptr()), "bbbp_pca_col_mean")
    return mean


def _resolve_gamma(gamma, X):
    """scikit-learn's ``_gamma``: "scale" = 1 / (d X.var()) (1 for constant X), "auto" = 1 / d."""
    d = X.shape[1]
    if gamma == "scale":
        var = float(X.to(torch.float64).var(unbiased=False).item())
        return 1.0 / (d * var) if var != 0.0 else 1.0
    if gamma == "auto":
        return 1.0 / d
    return float(gamma)


def kernel_matrix(X, kernel="rbf", gamma=1.0):
    """``bbbp_svm_kernel_matrix`` of a device matrix X [n, d] (float32 / float64, unit inner stride): (K [n, n] float64 on X's device,
    the float64 column mean the RBF form centres on, the row norms about it).  ValueError for non-finite X or a matrix that does not fit
    in free device memory."""
    if kernel not in KERNELS:
        raise ValueError(f"svm: kernel must be 'linear' or 'rbf', got {kernel!r}")
    n, d = X.shape
    if n < 1 or d < 1:
        raise ValueError(f"svm: need at least one row and one feature, got shape {(n, d)}")
    with torch.cuda.device(X.device):
        free = torch.cuda.mem_get_info(X.device)[0]
        if 8 * n * n > free:
            raise ValueError(f"svm: the {n} x {n} float64 kernel matrix ({8 * n * n / 2 ** 30:.1f} GiB) does not fit in free device memory "
                             f"({free / 2 ** 30:.1f} GiB)")
        rbf = kernel == "rbf"
        mean = _col_mean(X) if rbf else None
        norms = _norms(X, mean, "the training set")          # linear: only the non-finite check
        K = torch.empty((n, n), dtype=torch.float64, device=X.device)
        desc = _lib.SvmKernelDesc(n, d, KERNELS[kernel], float(gamma), X.data_ptr(), _dense.DT[X.dtype], _dense.ld(X),
                                  mean.data_ptr() if rbf else None, norms.data_ptr() if rbf else None, K.data_ptr(), n)
        _lib.check(_lib.lib().bbbp_svm_kernel_matrix(_dense.stream(), ctypes.byref(desc)), "bbbp_svm_kernel_matrix")
    return K, mean, (norms if rbf else None)


class _Problem:
    """One dual problem on the device: state, outputs and the descriptor ``bbbp_svm_smo`` takes."""

    def __init__(self, K, y_d, C, tol, rows=None):
        dev = K.device
        n = y_d.numel()
        self.K, self.y, self.rows, self.n, self.C = K, y_d, rows, n, float(C)
        self.alpha = torch.zeros(n, dtype=torch.float64, device=dev)
        self.grad = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        self.diag = torch.empty(n, dtype=torch.float64, device=dev)
        self.rho = torch.zeros(1, dtype=torch.float64, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)       # n_iter, done
        self.desc = _lib.SvmProblem(K.data_ptr(), K.stride(0), None if rows is None else rows.data_ptr(), y_d.data_ptr(), self.alpha.data_ptr(),
                                    self.grad.data_ptr(), self.diag.data_ptr(), self.rho.data_ptr(), self.flags.data_ptr(),
                                    self.flags.data_ptr() + 4, n, float(C), float(tol))


def _solve(problems, max_iter=-1, iters_per_launch=None, entry="bbbp_svm_smo"):
    """Run ``bbbp_svm_smo`` (or ``entry``, for ``_SvrProblem``s) until every problem is done (or has run ``max_iter`` iterations).
    Returns per problem (n_iter, converged)."""
    n_max = max(p.n for p in problems)
    base = ITERS_PER_LAUNCH if entry == "bbbp_svm_smo" else SVR_ITERS_PER_LAUNCH
    per = int(iters_per_launch or max(1, base * ITERS_REFERENCE_N // max(n_max, ITERS_REFERENCE_N)))
    L = _lib.lib()
    kind = type(problems[0].desc)
    state = [[0, False] for _ in problems]
    live = list(range(len(problems)))
    ran = 0
    while live:
        step = per if max_iter < 0 else min(per, max_iter - ran)
        if step <= 0:
            break
        arr = (kind * len(live))(*[problems[q].desc for q in live])
        _lib.check(getattr(L, entry)(_dense.stream(), arr, len(live), step), entry)
        ran += step
        flags = torch.stack([problems[q].flags for q in live]).cpu().numpy()      # the host read that ends the launch
        for q, (n_iter, done) in zip(live, flags):
            state[q] = [int(n_iter), bool(done)]
        live = [q for q in live if not state[q][1]]
    return [tuple(s) for s in state]


def _decision(model, dev, Xq, slices=0):
    """``bbbp_svm_decision`` of a fitted ``SVC`` or ``SVR`` on the device matrix Xq: sum_s coef_s k(sv_s, x) + intercept, float64 [m]."""
    if not hasattr(model, "_sv"):
        raise RuntimeError("svm: not fitted")
    m, d = Xq.shape
    if d != model.n_features_in_:
        raise ValueError(f"svm: the queries have {d} features, the fit saw {model.n_features_in_}")
    with torch.cuda.device(dev):
        qn = _norms(Xq, model._mean_d, "the query set") if m else None
        out = torch.full((m,), float(model.intercept_[0]), dtype=torch.float64, device=dev)
        n_sv = model._sv.shape[0]
        if m == 0 or n_sv == 0:
            return out
        rbf = model.kernel == "rbf"
        desc = _lib.SvmDecisionDesc(m, n_sv, d, KERNELS[model.kernel], float(model._gamma), Xq.data_ptr(), _dense.DT[Xq.dtype], _dense.ld(Xq),
                                    model._sv.data_ptr(), _dense.DT[model._sv.dtype], _dense.ld(model._sv), model._mean_d.data_ptr() if rbf else None,
                                    qn.data_ptr() if rbf else None, model._sv_norms.data_ptr() if rbf else None, model._coef_d.data_ptr(),
                                    float(model.intercept_[0]), out.data_ptr(), int(slices))
        L = _lib.lib()
        _dense.launch_with_workspace(L.bbbp_svm_decision_workspace_bytes, L.bbbp_svm_decision, desc, dev, "bbbp_svm_decision")
    return out


class SVC(_estimator.Params):
    """``SVC(C=1.0, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, *, device="cuda")``: scikit-learn's names for two classes.

    ``fit`` takes a CUDA tensor or a numpy array, float32 or float64, [n, d], and labels of any sortable kind with two distinct values.
    ``decision_function`` returns float64 [m]: a numpy array for numpy input, a CUDA tensor for a CUDA tensor; ``predict`` returns a numpy
    array of ``classes_``' dtype.  ``support_`` lists the first class's support vectors in ascending order, then the second's, as
    scikit-learn does; ``dual_coef_`` [1, n_SV], ``intercept_`` [1] and ``n_support_`` [2] follow it.  ``shrinking`` is accepted and
    ignored."""

    def __init__(self, C=1.0, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, *, device="cuda", shrinking=False, probability=False,
                 class_weight=None, **unsupported):
        if unsupported:
            raise ValueError(f"SVC: unsupported parameters {sorted(unsupported)}")
        if probability:
            raise ValueError("SVC: probability=True is not a mode of this class: svm.PlattSVC fits the Platt-scaled probabilities "
                             "(its folds come from numpy's generator, not from libsvm's own)")
        if class_weight is not None:
            raise ValueError("SVC: class_weight is not supported")
        _check_params(C, kernel, gamma, tol, max_iter)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SVC: device {device!r}: the solver runs on the GPU (no CPU fallback)")
        self.C, self.kernel, self.gamma, self.tol, self.max_iter = float(C), kernel, gamma, float(tol), int(max_iter)

    _params = ("C", "kernel", "gamma", "tol", "max_iter", "device")

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y):
        classes, ys = _binary_labels(y, None)
        X, _ = _dense.to_device_matrix(X, self.device, "svm", allow_row_stride=True)
        if X.shape[0] != len(ys):
            raise ValueError(f"SVC: X has {X.shape[0]} rows, y has {len(ys)}")
        with torch.cuda.device(self.device):
            g = _resolve_gamma(self.gamma, X)
            K, mean, norms = kernel_matrix(X, self.kernel, g)
            pr = _Problem(K, torch.from_numpy(ys).to(self.device), self.C, self.tol)
            (n_iter, done), = _solve([pr], self.max_iter)
            self._adopt(X, classes, ys, g, mean, norms, pr, n_iter, done)
        return self

    def _adopt(self, X, classes, ys, g, mean, norms, pr, n_iter, done):
        """Fitted attributes from a solved problem over the rows X (``pr``'s own row order)."""
        if not done:
            from sklearn.exceptions import ConvergenceWarning
            warnings.warn(f"SVC: solver stopped after max_iter={self.max_iter} iterations before reaching tol={self.tol}", ConvergenceWarning)
        alpha = pr.alpha.cpu().numpy()
        sv = np.flatnonzero(alpha > 0)
        sup = np.concatenate([sv[ys[sv] > 0], sv[ys[sv] < 0]])
        self.classes_, self._gamma, self.n_iter_ = classes, g, n_iter
        self.support_ = sup.astype(np.int32)
        self.n_support_ = np.array([int((ys[sv] > 0).sum()), int((ys[sv] < 0).sum())], dtype=np.int32)
        self.dual_coef_ = (-ys * alpha)[sup][None, :]
        self.intercept_ = np.array([float(pr.rho.item())])
        self.alpha_ = alpha
        sup_d = torch.from_numpy(sup).to(self.device)
        self._sv = X.index_select(0, sup_d)
        self._coef_d = torch.from_numpy(np.ascontiguousarray(self.dual_coef_[0])).to(self.device)
        self._mean_d = mean
        self._sv_norms = None if norms is None else norms.index_select(0, sup_d)
        self.support_vectors_ = self._sv.cpu().numpy()
        self.n_features_in_ = X.shape[1]
        self.fit_status_ = 0 if done else 1

    # ---- decision ---------------------------------------------------------------------------------------------------
    def _decision(self, Xq, slices=0):
        return _decision(self, self.device, Xq, slices)

    def decision_function(self, X, *, slices=0):
        """f(x) for every row of X.  ``slices`` > 0 forces how many work-groups share a query tile's support vectors (a test hook: the
        result does not depend on it)."""
        if not hasattr(self, "_sv"):
            raise RuntimeError("svm: not fitted")
        Xq, was_numpy = _dense.to_device_matrix(X, self.device, "svm", allow_row_stride=True)
        out = self._decision(Xq, slices)
        return out.cpu().numpy() if was_numpy else out

    def predict(self, X):
        """Class labels as a numpy array of ``classes_``' dtype (labels need not be numbers, so they stay on the host)."""
        if not hasattr(self, "_sv"):
            raise RuntimeError("svm: not fitted")
        Xq, _ = _dense.to_device_matrix(X, self.device, "svm", allow_row_stride=True)
        return self.classes_[(self._decision(Xq) > 0).cpu().numpy().astype(np.intp)]


def grid_search_cv(X, y, param_grid, cv: int = 5, device="cuda", *, tol=1e-3, max_iter=-1):
    """The reference's ``GridSearchCV(SVC(), param_grid, cv=5, scoring='f1')`` (model_opt_maccs.py:124-180) over ``C``, ``kernel`` and ``gamma``.

    Same conventions as ``neighbors.grid_search_cv``: sorted keys, ``itertools.product`` order, scikit-learn's ``StratifiedKFold(cv)``,
    ``f1_score`` of ``classes_[1]``, the first maximum wins; ``param_grid`` is a dict or, as for scikit-learn, a list of dicts.
    The linear matrix does not depend on the fold: it is formed once over all rows and a fold's problems index into it.  An RBF matrix depends on the fold through the mean it is centred on and through ``gamma="scale"``: one per
    fold and distinct gamma, over the fold's training rows, exactly as a single ``fit`` forms it.  All problems of a fold -- every C of
    every kernel -- are solved in one batch, so every grid point equals a single ``SVC(...).fit`` on that fold bit for bit.
    Returns (best_params, mean F1 per point, the classifier refitted on all rows with best_params)."""
    from itertools import product
    from sklearn.metrics import f1_score
    from sklearn.model_selection import StratifiedKFold
    points = []
    for sub in ([param_grid] if isinstance(param_grid, dict) else list(param_grid)):      # a list of grids: one after the other, as ParameterGrid
        unknown = set(sub) - {"C", "kernel", "gamma"}
        if unknown:
            raise ValueError(f"svm.grid_search_cv: unsupported grid keys {sorted(unknown)}")
        keys = sorted(sub)
        points += [dict(zip(keys, vals)) for vals in product(*(sub[k] for k in keys))]
    if not points:
        raise ValueError("svm.grid_search_cv: the grid is empty")
    full = [(pt.get("C", 1.0), pt.get("kernel", "rbf"), pt.get("gamma", "scale")) for pt in points]
    for C, kernel, gamma in full:
        _check_params(C, kernel, gamma, tol, max_iter, "svm.grid_search_cv")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"svm.grid_search_cv: device {device!r}: the solver runs on the GPU (no CPU fallback)")
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    y = np.asarray(y)
    classes, ys_all = _binary_labels(y, X.shape[0], "svm.grid_search_cv")
    pos = classes[1]
    folds = list(StratifiedKFold(n_splits=cv).split(X, y))
    f1 = np.zeros((len(points), len(folds)))
    with torch.cuda.device(dev):
        X_d = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        K_lin = kernel_matrix(X_d, "linear")[0] if any(k == "linear" for _, k, _ in full) else None
        for fi, (tr, te) in enumerate(folds):
            Xtr, Xte, ys = X_d[torch.from_numpy(tr).to(dev)], X_d[torch.from_numpy(te).to(dev)], ys_all[tr]
            y_d = torch.from_numpy(ys).to(dev)
            rows = torch.from_numpy(tr.astype(np.int32)).to(dev)
            mats, problems, owner = {}, [], {}
            gammas = {gamma: _resolve_gamma(gamma, Xtr) for _, kernel, gamma in full if kernel == "rbf"}      # one reduction per distinct gamma
            for C, kernel, gamma in full:
                g = gammas[gamma] if kernel == "rbf" else 0.0
                key = (float(C), kernel, g)
                if key in owner:
                    continue
                if kernel == "rbf" and g not in mats:
                    mats[g] = kernel_matrix(Xtr, "rbf", g)
                owner[key] = len(problems)
                problems.append(_Problem(K_lin, y_d, C, tol, rows) if kernel == "linear" else _Problem(mats[g][0], y_d, C, tol))
            solved = _solve(problems, max_iter)
            preds = {}
            for pi, (C, kernel, gamma) in enumerate(full):
                g = gammas[gamma] if kernel == "rbf" else 0.0
                key = (float(C), kernel, g)
                if key not in preds:
                    q = owner[key]
                    clf = SVC(C, kernel, g if kernel == "rbf" else "scale", tol, max_iter, device=dev)
                    mean, norms = (mats[g][1], mats[g][2]) if kernel == "rbf" else (None, None)
                    clf._adopt(Xtr, classes, ys, g, mean, norms, problems[q], *solved[q])
                    preds[key] = clf.predict(Xte)
                f1[pi, fi] = f1_score(y[te], preds[key], pos_label=pos)
            del mats, problems
    scores = [float(v) for v in f1.mean(axis=1)]
    best = int(np.argmax(scores))
    C, kernel, gamma = full[best]
    fitted = SVC(C, kernel, gamma, tol, max_iter, device=dev).fit(X, y)
    return points[best], scores, fitted


# ---- Platt-scaled probabilities ----------------------------------------------------------------------------------------------------------
PLATT_STATUS = {0: "converged", 1: "the line search failed", 2: "stopped at 100 iterations"}      # BBBP_PLATT_*


def platt_folds(n, cv, random_state):
    """libsvm's unstratified folds with numpy's generator: fold i holds out ``perm[i * n // cv : (i + 1) * n // cv]`` of
    ``perm = RandomState(random_state).permutation(n)``.  A list of ``cv`` index arrays that partition ``range(n)``."""
    perm = np.random.RandomState(random_state).permutation(n)
    return [perm[i * n // cv:(i + 1) * n // cv] for i in range(cv)]


def _check_folds(folds, n):
    """``folds`` as a list of int64 held-out index arrays that partition ``range(n)``."""
    try:
        held = [np.asarray(f) for f in folds]
    except TypeError:
        raise ValueError("PlattSVC: folds must be a list of held-out index arrays") from None
    if not held or any(f.ndim != 1 or (f.size and f.dtype.kind not in "iu") for f in held):
        raise ValueError("PlattSVC: folds must be a non-empty list of 1-D integer index arrays")
    held = [f.astype(np.int64) for f in held]
    if not np.array_equal(np.sort(np.concatenate(held)), np.arange(n)):
        raise ValueError(f"PlattSVC: folds must partition range({n}): every row held out exactly once")
    return held


def _platt_fit(decs, ys):
    """``bbbp_svm_platt_fit`` of the problems (decs[q], ys[q]), float64 device vectors of equal length >= 1: one launch (per 64 problems),
    one host read.  Returns (ab [P, 2] float64, info [P, 2] int32) as numpy arrays."""
    dev = decs[0].device
    ab = torch.empty((len(decs), 2), dtype=torch.float64, device=dev)
    info = torch.empty((len(decs), 2), dtype=torch.int32, device=dev)
    _platt_launch(decs, ys, ab, info)
    return ab.cpu().numpy(), info.cpu().numpy()


def _platt_launch(decs, ys, ab, info):
    """The launch of ``_platt_fit`` alone: problem q writes ab[q] and info[q] (device, [P, 2] float64 / int32)."""
    arr = (_lib.SvmPlattProblem * len(decs))(*[_lib.SvmPlattProblem(d.data_ptr(), y.data_ptr(), d.numel(), ab.data_ptr() + 16 * q, info.data_ptr() + 8 * q)
                                              for q, (d, y) in enumerate(zip(decs, ys))])
    _lib.check(_lib.lib().bbbp_svm_platt_fit(_dense.stream(), arr, len(decs)), "bbbp_svm_platt_fit")


def _oof_launch(K, parts, oof):
    """``bbbp_svm_oof_decision``: for every (solved fold ``_Problem`` over K, its held-out rows as an int32 device vector) of ``parts`` the
    held-out decision values in libsvm's sign, written to ``oof`` [n] by data row.  One launch (per 32 folds), no host read."""
    n = K.shape[0]
    arr = (_lib.SvmOofDesc * len(parts))(*[_lib.SvmOofDesc(K.data_ptr(), K.stride(0), n, pr.rows.data_ptr(), pr.y.data_ptr(), pr.alpha.data_ptr(),
                                                          pr.rho.data_ptr(), pr.n, te_d.data_ptr(), te_d.numel(), oof.data_ptr())
                                          for pr, te_d in parts])
    _lib.check(_lib.lib().bbbp_svm_oof_decision(_dense.stream(), arr, len(parts)), "bbbp_svm_oof_decision")


def _platt_problems(K, y_d, ys, held, C, tol, oof):
    """libsvm's fold problems over the shared matrix: for each non-empty held-out index array of ``held`` either a ``_Problem`` on the other
    rows (a row list into K) or, where those rows have one class or are none, libsvm's constant written to ``oof`` at once.  Returns the
    (problem, held-out rows as an int32 device vector) pairs."""
    n, dev, parts = len(ys), K.device, []
    for te in held:
        if len(te) == 0:
            continue
        keep = np.ones(n, dtype=bool)
        keep[te] = False
        tr = np.flatnonzero(keep)
        te_d = torch.from_numpy(te).to(dev)
        ytr = ys[tr]
        if len(tr) == 0 or (ytr > 0).all() or (ytr < 0).all():
            oof.index_fill_(0, te_d, 0.0 if len(tr) == 0 else float(ytr[0]))
            continue
        tr_d = torch.from_numpy(tr).to(dev)
        parts.append((_Problem(K, y_d.index_select(0, tr_d), C, tol, tr_d.to(torch.int32)), te_d.to(torch.int32)))
    return parts


def _platt_vector(v, dev, what):
    if isinstance(v, torch.Tensor):
        if not v.is_cuda:
            raise RuntimeError(f"svm.platt_scale: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {v.device} (no CPU fallback)")
        v = v.detach()
    else:
        v = np.asarray(v)
        if v.dtype.kind not in "fiub":
            raise ValueError(f"svm.platt_scale: {what} must hold real numbers, got dtype {v.dtype}")
        v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    if v.dim() != 1 or v.numel() < 1:
        raise ValueError(f"svm.platt_scale: {what} must be 1-D with at least one entry, got shape {tuple(v.shape)}")
    return v.to(device=dev, dtype=torch.float64).contiguous()


def platt_scale(dec, y_pm1, device="cuda"):
    """libsvm's ``sigmoid_train`` on the GPU (``bbbp_svm_platt_fit``): the (A, B) that minimise the cross-entropy of
    ``1 / (1 + exp(A dec + B))`` against the smoothed targets of the labels ``y_pm1`` (> 0 counts as the positive class), by Newton's
    method with backtracking as Lin, Lin and Weng state it.  ``dec`` and ``y_pm1`` are numpy arrays or CUDA tensors [n], or two lists of such
    for a batch that one launch solves, a work-group each; a problem's result does not depend on the batch.  Returns
    ``(A, B, n_iter, status)``: floats and ints for one problem, numpy arrays [P] for a list; status 0 = both gradient components below
    1e-5, 1 = the line search failed, 2 = 100 iterations."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"svm.platt_scale: device {device!r}: the fit runs on the GPU (no CPU fallback)")
    batch = isinstance(dec, (list, tuple)) and len(dec) > 0 and (isinstance(dec[0], torch.Tensor) or np.ndim(dec[0]) >= 1)
    decs, ys = (list(dec), list(y_pm1)) if batch else ([dec], [y_pm1])
    if len(decs) != len(ys):
        raise ValueError(f"svm.platt_scale: {len(decs)} decision vectors, {len(ys)} label vectors")
    with torch.cuda.device(dev):
        decs = [_platt_vector(d, dev, "dec") for d in decs]
        ys = [_platt_vector(y, dev, "y_pm1") for y in ys]
        for d, y in zip(decs, ys):
            if d.numel() != y.numel():
                raise ValueError(f"svm.platt_scale: dec has {d.numel()} entries, y_pm1 has {y.numel()}")
        if not bool(torch.stack([torch.isfinite(d).all() for d in decs]).all().item()):
            raise ValueError("svm.platt_scale: dec contains NaN or infinity")
        ab, info = _platt_fit(decs, ys)
    if batch:
        return ab[:, 0].copy(), ab[:, 1].copy(), info[:, 0].copy(), info[:, 1].copy()
    return float(ab[0, 0]), float(ab[0, 1]), int(info[0, 0]), int(info[0, 1])


class PlattSVC(SVC):
    """``PlattSVC(C=1.0, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, *, cv=5, random_state=0, device="cuda")``: scikit-learn's
    ``SVC(probability=True)`` for two classes.  Everything ``SVC`` has, fitted exactly as ``SVC`` fits it, plus ``predict_proba`` /
    ``predict_log_proba``, ``probA_`` and ``probB_`` ([1] each, libsvm's sign as scikit-learn stores them), ``platt_n_iter_``,
    ``platt_status_`` and ``oof_decision_`` ([n] float64 in libsvm's sign: positive towards ``classes_[0]``).

    ``fit(X, y, *, folds=None)`` follows libsvm: ``cv`` folds, each held-out row's decision value from the model trained on the other
    folds, a sigmoid fitted to those n values (``platt_scale``), and the model itself from all rows.  Here gamma is resolved once from all
    rows (as scikit-learn does before it calls libsvm), one kernel matrix is formed, and the fold problems -- row lists into it -- are
    solved in one batch with the all-rows problem.  A fold whose training part has one class gets libsvm's rule: its held-out values are
    +1 (only ``classes_[0]`` trained on), -1 (only ``classes_[1]``) or 0 (nothing).  ``folds``: a list of held-out index arrays that
    partition ``range(n)``, in place of the draw.  ``predict`` is the sign of the decision value, as scikit-learn's, and may disagree with
    the arg-max of ``predict_proba``.  A ``platt_status_`` other than 0 raises a ``ConvergenceWarning``.

    Two differences from scikit-learn:

    * the folds are libsvm's unstratified slices ``perm[i n // cv : (i + 1) n // cv]``, but the permutation is
      ``numpy.random.RandomState(random_state).permutation(n)``, not a draw from libsvm's own generator.  For one ``random_state``,
      ``probA_`` / ``probB_`` differ from scikit-learn's about as scikit-learn's own differ between two seeds (n = 200, d = 5, linear,
      scikit-learn 1.7.2: ``probA_`` from -0.954 to -0.842 over seeds 0 to 7); with the same folds they agree;
    * ``predict_proba`` is the exact sigmoid, as libsvm >= 3.3 returns for two classes.  scikit-learn's vendored libsvm sends two classes
      through ``multiclass_probability``, whose iteration stops at 0.005 / k: its values differ from the sigmoid of its own ``probA_`` /
      ``probB_`` by 2e-3 to 5e-3."""

    _params = ("C", "kernel", "gamma", "tol", "max_iter", "cv", "random_state", "device")

    def __init__(self, C=1.0, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, *, cv=5, random_state=0, device="cuda", **unsupported):
        if unsupported.get("class_weight") is not None:
            raise ValueError("PlattSVC: class_weight is not supported")
        unsupported.pop("class_weight", None)
        if unsupported:
            raise ValueError(f"PlattSVC: unsupported parameters {sorted(unsupported)}")
        _check_params(C, kernel, gamma, tol, max_iter, "PlattSVC")
        if isinstance(cv, bool) or not isinstance(cv, numbers.Integral) or cv < 2:
            raise ValueError(f"PlattSVC: cv must be an int of at least 2, got {cv!r}")
        if isinstance(random_state, bool) or not isinstance(random_state, numbers.Integral) or not (0 <= random_state < 2 ** 32):
            raise ValueError(f"PlattSVC: random_state must be an int in [0, 2^32), got {random_state!r}")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"PlattSVC: device {device!r}: the solver runs on the GPU (no CPU fallback)")
        # the values as given (get_params returns them, so that sklearn.base.clone round-trips)
        self.C, self.kernel, self.gamma, self.tol, self.max_iter = C, kernel, gamma, tol, max_iter
        self.cv, self.random_state, self.device = cv, random_state, device

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._params}

    def set_params(self, **params):
        unknown = set(params) - set(self._params)
        if unknown:
            raise ValueError(f"PlattSVC: unknown parameters {sorted(unknown)}")
        type(self)(**{**self.get_params(), **params})          # the constructor's checks
        for name, value in params.items():
            setattr(self, name, value)
        return self

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, *, folds=None):
        classes, ys = _binary_labels(y, None, "PlattSVC")
        n = len(ys)
        if folds is None:
            if self.cv > n:
                raise ValueError(f"PlattSVC: cv={self.cv} folds need at least as many rows, got {n}")
            held = platt_folds(n, int(self.cv), int(self.random_state))
        else:
            held = _check_folds(folds, n)
        dev = torch.device(self.device)
        X, _ = _dense.to_device_matrix(X, dev, "svm", allow_row_stride=True)
        if X.shape[0] != n:
            raise ValueError(f"PlattSVC: X has {X.shape[0]} rows, y has {n}")
        C, tol, max_iter = float(self.C), float(self.tol), int(self.max_iter)
        with torch.cuda.device(dev):
            g = _resolve_gamma(self.gamma, X)
            K, mean, norms = kernel_matrix(X, self.kernel, g)
            y_d = torch.from_numpy(ys).to(dev)
            oof = torch.empty(n, dtype=torch.float64, device=dev)
            parts = _platt_problems(K, y_d, ys, held, C, tol, oof)
            problems = [_Problem(K, y_d, C, tol)] + [pr for pr, _ in parts]      # the all-rows problem and the folds: one batch over one matrix
            solved = _solve(problems, max_iter)
            if parts:
                _oof_launch(K, parts, oof)
            ab, info = _platt_fit([oof], [y_d])
            # what the fold problems ended at, on the host (the device state, and with it the matrix, is released): per fold the
            # training rows, the held-out rows, alpha and rho
            self._folds = [(pr.rows.cpu().numpy(), te_d.cpu().numpy(), pr.alpha.cpu().numpy(), float(pr.rho.item())) for pr, te_d in parts]
            self._adopt(X, classes, ys, g, mean, norms, problems[0], *solved[0])
        from sklearn.exceptions import ConvergenceWarning
        if not all(done for _, done in solved[1:]):
            warnings.warn(f"PlattSVC: a fold's solver stopped after max_iter={self.max_iter} iterations before reaching tol={self.tol}", ConvergenceWarning)
        self.probA_, self.probB_ = np.array([ab[0, 0]]), np.array([ab[0, 1]])
        self.platt_n_iter_, self.platt_status_ = int(info[0, 0]), int(info[0, 1])
        self.oof_decision_ = oof.cpu().numpy()
        if self.platt_status_ != 0:
            warnings.warn(f"PlattSVC: the sigmoid fit ended without meeting its gradient criterion ({PLATT_STATUS[self.platt_status_]} after "
                          f"{self.platt_n_iter_} iterations)", ConvergenceWarning)
        return self

    # ---- probabilities ----------------------------------------------------------------------------------------------
    def _proba(self, X):
        if not hasattr(self, "_sv"):
            raise RuntimeError("svm: not fitted")
        dev = torch.device(self.device)
        Xq, was_numpy = _dense.to_device_matrix(X, dev, "svm", allow_row_stride=True)
        f = self._decision(Xq).neg()                                  # libsvm's sign: positive towards classes_[0]
        m = f.numel()
        with torch.cuda.device(dev):
            proba = torch.empty((m, 2), dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().bbbp_svm_platt_proba(_dense.stream(), f.data_ptr() if m else None, m, float(self.probA_[0]), float(self.probB_[0]),
                                                       proba.data_ptr() if m else None), "bbbp_svm_platt_proba")
        return proba, was_numpy

    def predict_proba(self, X):
        """[m, 2] float64 in ``classes_`` order (numpy in, numpy out; CUDA in, CUDA out): column 0 is libsvm's ``sigmoid_predict`` of minus
        the decision value, clipped to [1e-7, 1 - 1e-7]; column 1 is one minus it."""
        proba, was_numpy = self._proba(X)
        return proba.cpu().numpy() if was_numpy else proba

    def predict_log_proba(self, X):
        proba, was_numpy = self._proba(X)
        return np.log(proba.cpu().numpy()) if was_numpy else proba.log()


# ---- epsilon-support-vector regression ---------------------------------------------------------------------------------------------------
def _check_epsilon(epsilon, who):
    if isinstance(epsilon, bool) or not isinstance(epsilon, numbers.Real) or not (0.0 <= float(epsilon) < float("inf")):
        raise ValueError(f"{who}: epsilon must be a non-negative finite number, got {epsilon!r}")


def _targets(y, n, who="SVR"):
    """y as a float64 numpy vector: real, 1-D, finite, ``n`` long (None: any length)."""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{who}: y must be 1-D, got shape {y.shape}")
    if y.dtype.kind not in "fiub":
        raise ValueError(f"{who}: y must hold real numbers, got dtype {y.dtype}")
    y = np.ascontiguousarray(y, dtype=np.float64)
    if not np.isfinite(y).all():
        raise ValueError(f"{who}: y contains NaN or infinity")
    if n is not None and len(y) != n:
        raise ValueError(f"{who}: X has {n} rows, y has {len(y)}")
    return y


class _SvrProblem:
    """One epsilon-SVR dual problem on the device: state, outputs and the descriptor ``bbbp_svr_smo`` takes.  The solver's first launch
    sets alpha and the gradient itself: the host initialises the two flags only."""

    def __init__(self, K, t_d, C, epsilon, tol, rows=None):
        dev = K.device
        n = t_d.numel()
        self.K, self.t, self.rows, self.n, self.C, self.epsilon = K, t_d, rows, n, float(C), float(epsilon)
        self.alpha = torch.empty(2 * n, dtype=torch.float64, device=dev)
        self.grad = torch.empty(2 * n, dtype=torch.float64, device=dev)
        self.diag = torch.empty(n, dtype=torch.float64, device=dev)
        self.rho = torch.empty(1, dtype=torch.float64, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)       # n_iter, done
        self.desc = _lib.SvrProblem(K.data_ptr(), K.stride(0), None if rows is None else rows.data_ptr(), t_d.data_ptr(), self.alpha.data_ptr(),
                                    self.grad.data_ptr(), self.diag.data_ptr(), self.rho.data_ptr(), self.flags.data_ptr(),
                                    self.flags.data_ptr() + 4, n, float(C), float(epsilon), float(tol))


def _solve_svr(problems, max_iter=-1, iters_per_launch=None):
    return _solve(problems, max_iter, iters_per_launch, entry="bbbp_svr_smo")


class SVR:
    """``SVR(kernel="rbf", C=1.0, epsilon=0.1, gamma="scale", tol=1e-3, max_iter=-1, *, device="cuda", shrinking=False)``: scikit-learn's
    names.

    ``fit`` takes a CUDA tensor or a numpy array, float32 or float64, [n, d], and real targets [n].  ``predict`` returns float64 [m]: a
    numpy array for numpy input, a CUDA tensor for a CUDA tensor; ``predict_device`` always a CUDA tensor.  ``support_`` lists the rows
    with alpha - alpha* != 0 in ascending order; ``dual_coef_`` [1, n_SV] holds those differences, ``intercept_`` [1] is -rho.
    ``shrinking`` is accepted and ignored.  ``get_params`` / ``set_params`` make the class clone under ``sklearn.base.clone``, so it serves
    as a base learner of ``ensemble.StackingRegressor``."""

    _params = ("kernel", "C", "epsilon", "gamma", "tol", "max_iter", "device", "shrinking")

    def __init__(self, kernel="rbf", C=1.0, epsilon=0.1, gamma="scale", tol=1e-3, max_iter=-1, *, device="cuda", shrinking=False, **unsupported):
        if unsupported:
            raise ValueError(f"SVR: unsupported parameters {sorted(unsupported)}")
        _check_params(C, kernel, gamma, tol, max_iter, "SVR")
        _check_epsilon(epsilon, "SVR")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"SVR: device {device!r}: the solver runs on the GPU (no CPU fallback)")
        self.kernel, self.C, self.epsilon, self.gamma, self.tol, self.max_iter = kernel, C, epsilon, gamma, tol, max_iter
        self.device, self.shrinking = device, shrinking

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._params}

    def set_params(self, **params):
        unknown = set(params) - set(self._params)
        if unknown:
            raise ValueError(f"SVR: unknown parameters {sorted(unknown)}")
        type(self)(**{**self.get_params(), **params})          # the constructor's checks
        for name, value in params.items():
            setattr(self, name, value)
        return self

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("SVR: sample_weight is not supported")
        t = _targets(y, None)
        dev = torch.device(self.device)
        X, _ = _dense.to_device_matrix(X, dev, "svm", allow_row_stride=True)
        if X.shape[0] != len(t):
            raise ValueError(f"SVR: X has {X.shape[0]} rows, y has {len(t)}")
        with torch.cuda.device(dev):
            g = _resolve_gamma(self.gamma, X)
            K, mean, norms = kernel_matrix(X, self.kernel, g)
            pr = _SvrProblem(K, torch.from_numpy(t).to(dev), self.C, self.epsilon, self.tol)
            (n_iter, done), = _solve_svr([pr], int(self.max_iter))
            self._adopt(X, g, mean, norms, pr, n_iter, done)
        return self

    def _adopt(self, X, g, mean, norms, pr, n_iter, done):
        """Fitted attributes from a solved problem over the rows X (``pr``'s own row order)."""
        if not done:
            from sklearn.exceptions import ConvergenceWarning
            warnings.warn(f"SVR: solver stopped after max_iter={self.max_iter} iterations before reaching tol={self.tol}", ConvergenceWarning)
        dev = torch.device(self.device)
        n = pr.n
        alpha = pr.alpha.cpu().numpy()
        coef = alpha[:n] - alpha[n:]
        sup = np.flatnonzero(coef != 0.0)
        self._gamma, self.n_iter_ = g, n_iter
        self.support_ = sup.astype(np.int32)
        self.n_support_ = np.array([len(sup)], dtype=np.int32)
        self.dual_coef_ = coef[sup][None, :]
        self.intercept_ = np.array([-float(pr.rho.item())])
        self.alpha_ = alpha
        sup_d = torch.from_numpy(sup).to(dev)
        self._sv = X.index_select(0, sup_d)
        self._coef_d = torch.from_numpy(np.ascontiguousarray(self.dual_coef_[0])).to(dev)
        self._mean_d = mean
        self._sv_norms = None if norms is None else norms.index_select(0, sup_d)
        self.support_vectors_ = self._sv.cpu().numpy()
        self.n_features_in_ = X.shape[1]
        self.fit_status_ = 0 if done else 1

    # ---- predict ----------------------------------------------------------------------------------------------------
    def _decision(self, Xq, slices=0):
        return _decision(self, torch.device(self.device), Xq, slices)

    def predict_device(self, X, *, slices=0):
        """f(x) for every row of X as a float64 CUDA tensor.  ``slices``: ``SVC.decision_function``'s test hook."""
        if not hasattr(self, "_sv"):
            raise RuntimeError("svm: not fitted")
        Xq, _ = _dense.to_device_matrix(X, torch.device(self.device), "svm", allow_row_stride=True)
        return self._decision(Xq, slices)

    def predict(self, X):
        if not hasattr(self, "_sv"):
            raise RuntimeError("svm: not fitted")
        Xq, was_numpy = _dense.to_device_matrix(X, torch.device(self.device), "svm", allow_row_stride=True)
        out = self._decision(Xq)
        return out.cpu().numpy() if was_numpy else out


def _svr_point(params, who):
    """(kernel, C, epsilon, gamma, tol, max_iter) of a parameter dict, checked."""
    unknown = set(params) - {"kernel", "C", "epsilon", "gamma", "tol", "max_iter", "shrinking"}
    if unknown:
        raise ValueError(f"{who}: unsupported parameters {sorted(unknown)}")
    kernel, C, epsilon, gamma = params.get("kernel", "rbf"), params.get("C", 1.0), params.get("epsilon", 0.1), params.get("gamma", "scale")
    tol, max_iter = params.get("tol", 1e-3), params.get("max_iter", -1)
    _check_params(C, kernel, gamma, tol, max_iter, who)
    _check_epsilon(epsilon, who)
    return kernel, C, epsilon, gamma, tol, max_iter


def _host_matrix(X):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"svm: expected a 2-D [n, d] input, got shape {X.shape}")
    return np.ascontiguousarray(X if X.dtype in (np.float32, np.float64) else X.astype(np.float64))


def _fold_problems(X_d, t_all, tr, points, K_lin, dev):
    """The problems of ``points`` = (kernel, C, epsilon, gamma, tol, max_iter) over the training rows ``tr`` of X_d: the points that share a
    matrix -- the fold's RBF matrix of one gamma, or the shared linear matrix ``K_lin`` through the fold's row list -- stand side by side
    over it, and equal points share one problem.  Returns (problems, finish): ``finish(solved)`` takes their ``_solve_svr`` results and
    returns one fitted ``SVR`` per point, each equal to a single fit on those rows bit for bit."""
    tr_d = torch.from_numpy(np.asarray(tr, dtype=np.int64)).to(dev)
    Xtr = X_d.index_select(0, tr_d)
    t_d = torch.from_numpy(np.ascontiguousarray(t_all[tr])).to(dev)
    rows = tr_d.to(torch.int32) if any(p[0] == "linear" for p in points) else None
    gammas = {gamma: _resolve_gamma(gamma, Xtr) for gamma in {p[3] for p in points}}
    key = lambda kernel, C, epsilon, gamma, tol: (kernel, float(C), float(epsilon), gammas[gamma] if kernel == "rbf" else 0.0, float(tol))  # noqa: E731
    mats, problems, owner = {}, [], {}
    for kernel, C, epsilon, gamma, tol, _ in points:
        k = key(kernel, C, epsilon, gamma, tol)
        if k in owner:
            continue
        if kernel == "rbf" and k[3] not in mats:
            mats[k[3]] = kernel_matrix(Xtr, "rbf", k[3])
        owner[k] = len(problems)
        problems.append(_SvrProblem(K_lin, t_d, C, epsilon, tol, rows) if kernel == "linear" else _SvrProblem(mats[k[3]][0], t_d, C, epsilon, tol))

    def finish(solved):
        models = []
        for kernel, C, epsilon, gamma, tol, max_iter in points:
            q = owner[key(kernel, C, epsilon, gamma, tol)]
            m = SVR(kernel, C, epsilon, gamma, tol, max_iter, device=dev)
            _, mean, norms = mats[gammas[gamma]] if kernel == "rbf" else (None, None, None)
            m._adopt(Xtr, gammas[gamma], mean, norms, problems[q], *solved[q])
            models.append(m)
        return models
    return problems, finish


def fit_svr_folds(X, y, folds, device="cuda", **params):
    """The fold loop of the reference's regression stack (multi_input_data_regression_opt_transformer_cnn_opt_more.py:133-149) for its
    ``SVR``: one model per fold, all folds solved in one batch.  ``folds``: training-row index arrays, or (train, test) pairs as
    ``KFold.split`` yields them.  An RBF matrix depends on the fold (its mean and ``gamma="scale"``): one per fold; the linear matrix is
    formed once over all rows and a fold addresses it through its row list.  ``params``: ``SVR``'s.  Every returned model equals
    ``SVR(**params).fit(X[train], y[train])`` bit for bit."""
    point = _svr_point(params, "svm.fit_svr_folds")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"svm.fit_svr_folds: device {device!r}: the solver runs on the GPU (no CPU fallback)")
    X = _host_matrix(X)
    t = _targets(y, X.shape[0], "svm.fit_svr_folds")
    trains = [np.asarray(f[0] if isinstance(f, (tuple, list)) and len(f) == 2 and np.ndim(f[0]) == 1 else f, dtype=np.int64) for f in folds]
    if not trains:
        raise ValueError("svm.fit_svr_folds: no folds")
    for tr in trains:
        if tr.ndim != 1 or len(tr) == 0 or tr.min() < 0 or tr.max() >= X.shape[0]:
            raise ValueError(f"svm.fit_svr_folds: a fold's training rows must be a non-empty 1-D list of indices below {X.shape[0]}")
    with torch.cuda.device(dev):
        X_d = torch.from_numpy(X).to(dev)
        K_lin = kernel_matrix(X_d, "linear")[0] if point[0] == "linear" else None
        parts = [_fold_problems(X_d, t, tr, [point], K_lin, dev) for tr in trains]
        solved = _solve_svr([pr for problems, _ in parts for pr in problems], int(point[5]))      # one problem per fold, all in one batch
        return [finish([s])[0] for (_, finish), s in zip(parts, solved)]


def grid_search_cv_svr(X, y, param_grid, cv: int = 5, device="cuda", *, tol=1e-3, max_iter=-1):
    """``GridSearchCV(SVR(), param_grid, cv=cv)`` over ``C``, ``epsilon``, ``kernel`` and ``gamma``: scikit-learn's default for a regressor,
    unshuffled ``KFold(cv)`` and R^2 scoring, sorted keys, ``itertools.product`` order, the first maximum wins; ``param_grid`` is a dict
    or a list of dicts.  All points of a fold that share a matrix are solved side by side over it (``_fold_problems``), so every point equals
    a single ``SVR(...).fit`` on that fold bit for bit.  Returns (best_params, mean R^2 per point, the model refitted on all rows with
    best_params)."""
    from itertools import product
    from sklearn.metrics import r2_score
    from sklearn.model_selection import KFold
    points = []
    for sub in ([param_grid] if isinstance(param_grid, dict) else list(param_grid)):
        unknown = set(sub) - {"C", "epsilon", "kernel", "gamma"}
        if unknown:
            raise ValueError(f"svm.grid_search_cv_svr: unsupported grid keys {sorted(unknown)}")
        keys = sorted(sub)
        points += [dict(zip(keys, vals)) for vals in product(*(sub[k] for k in keys))]
    if not points:
        raise ValueError("svm.grid_search_cv_svr: the grid is empty")
    full = [_svr_point({**pt, "tol": tol, "max_iter": max_iter}, "svm.grid_search_cv_svr") for pt in points]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"svm.grid_search_cv_svr: device {device!r}: the solver runs on the GPU (no CPU fallback)")
    X = _host_matrix(X)
    t = _targets(y, X.shape[0], "svm.grid_search_cv_svr")
    folds = list(KFold(n_splits=cv).split(X))
    r2 = np.zeros((len(points), len(folds)))
    with torch.cuda.device(dev):
        X_d = torch.from_numpy(X).to(dev)
        K_lin = kernel_matrix(X_d, "linear")[0] if any(p[0] == "linear" for p in full) else None
        for fi, (tr, te) in enumerate(folds):
            Xte = X_d.index_select(0, torch.from_numpy(te).to(dev))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                   # a capped fit warns once more below, in the refit, if it is the chosen one
                problems, finish = _fold_problems(X_d, t, tr, full, K_lin, dev)
                models = finish(_solve_svr(problems, int(max_iter)))
            for pi, m in enumerate(models):
                r2[pi, fi] = r2_score(t[te], m.predict_device(Xte).cpu().numpy())
            del models, problems, finish
    scores = [float(v) for v in r2.mean(axis=1)]
    best = int(np.argmax(scores))
    kernel, C, epsilon, gamma, tol, max_iter = full[best]
    fitted = SVR(kernel, C, epsilon, gamma, tol, max_iter, device=device).fit(X, t)
    return points[best], scores, fitted
