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

Out of scope: ``probability=True`` (Platt scaling's internal cross-validation draws from libsvm's own generator), more than two classes,
``class_weight``, kernels other than linear and RBF, shrinking (accepted and ignored: the optimum is the same), a kernel matrix larger than
free device memory, more than one GPU.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import numbers
import warnings

import numpy as np
import torch

from . import _dense, _lib

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


class SVC:
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
            raise ValueError("SVC: probability=True is not supported (Platt scaling's internal cross-validation draws from libsvm's own generator)")
        if class_weight is not None:
            raise ValueError("SVC: class_weight is not supported")
        _check_params(C, kernel, gamma, tol, max_iter)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SVC: device {device!r}: the solver runs on the GPU (no CPU fallback)")
        self.C, self.kernel, self.gamma, self.tol, self.max_iter = float(C), kernel, gamma, float(tol), int(max_iter)

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
