"""``xgboost.XGBRegressor`` for the GPU: XGBoost's ``hist`` trees for the squared error, fitted by ``csrc/xgb.hip``.

Every logBB script of the reference stacks ``XGBRegressor(n_estimators=300, learning_rate=0.01, max_depth=30, tree_method="hist")`` on
``hstack([fingerprints, images])`` (``Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:186-189``): about 1 058 rows,
49 319 columns of few distinct values each, trees that grow until rows are alone.  The model the reference ships
(``Models/xgb_model_maccs.pkl``, XGBoost 2.0.0) says what it fits: ``grow_quantile_histmaker`` with ``max_bin=256``, ``reg:squarederror``,
``lambda=1``, ``gamma=0``, ``min_child_weight=1``, ``boost_from_average``.  The fitted model is a ``boosters.XGBTrees``: the predict kernel,
``ensemble.screen(boosters=...)`` and ``ensemble.StackingRegressor`` take it as it is.

The algorithm -- XGBoost 2.0's ``hist`` updater for ``reg:squarederror``, restated so that no sum has an order; ``tests/xgb_numpy.py``
restates it in numpy and the GPU fit equals that bit for bit:

*Quantisation.*  Features are float32.  Per feature, with the sorted column ``s_0 <= ... <= s_{n-1}``: if the column has at most
``max_bin`` distinct values, the cuts are all distinct values above the minimum, and a split's ``split_condition`` is then a value of the
column, the smallest on the right in the whole column, as XGBoost's hist does; otherwise the cuts are the distinct values among
``s[floor(j n / max_bin)]``, ``j = 1 .. max_bin - 1``, that exceed ``s_0``.  THE ONE DELIBERATE DEVIATION: that second rule is this
module's, not XGBoost's weighted quantile sketch; columns of more than ``max_bin`` distinct values get other cuts than XGBoost gives them.
A cut of -0.0 is stored as +0.0.  ``bin(x)`` is the number of cuts ``<= x``; ``2 <= max_bin <= 256``, so a bin is one byte.  Columns without a cut are constant (most of
the white image border) and are dropped before anything is uploaded; the kernels see the live columns, reported indices are the original ones.

*Gradients.*  ``base_score`` is ``float32(mean(y))`` unless given.  Margins are float32, ``g_i = margin_i - float32(y_i)`` in float32,
``h_i = 1``.  Per tree ``gmax = max |g_i|``, ``k = 47 - ilogb(gmax)`` (``k = 0`` when ``gmax == 0``: the tree is then one leaf of weight
0, stored as -0.0) and ``q_i = llrint((double)g_i 2^k)``, an exact product.  With ``n <= 8 192`` rows ``|sum q| <= 2^61``: a node's
``Q = sum q_i`` is an exact 64-bit integer whatever the order, ``G = ldexp((double)Q, -k)`` is one rounding, ``H = (double)m`` its row count.

*Split score*, in float64, every operation rounded on its own: ``term(G, H) = G G / (H + lambda)``, ``gain = (term(G_L, H_L) + term(G_R,
H_R)) - term(G, H)``.  A candidate is a boundary between two bins of a live feature with ``m_L >= max(1, min_child_weight)`` and ``m_R``
likewise.  The best candidate maximises the gain; among equal gains the lowest feature index wins (XGBoost's ``SplitEntry::NeedReplace``
has the same rule), then the lowest bin.  A node splits iff the best ``gain > 1e-6`` (XGBoost's ``kRtEps``), ``gain >= gamma`` and its
depth is ``< max_depth``.  ``w = -G / (H + lambda)``; a leaf's value is ``float32((double)float32(learning_rate) w)``; after a tree
``margin_i = margin_i + value[leaf(i)]`` in float32.

*Node ids and statistics.*  Ids are XGBoost's: the root is 0, nodes are expanded level by level in ascending id, each split appends its
left and right child as the next two ids (the shipped model's trees are numbered so).  Every node records, float32 as in XGBoost's model
schema, ``sum_hessian = m``, ``loss_changes`` = the gain (0 in a leaf) and ``base_weights`` = ``w`` in a split node, the scaled leaf
value in a leaf, which is how the shipped model stores them.  ``default_left`` is 0 everywhere, as in the shipped model.

PARITY UNPINNED: the xgboost package is installed neither where this is built nor where it runs.  Fits and the loading of
``get_model_json`` by XGBoost itself have never been compared with the package, only with the statistics of the model it shipped
(``tests/golden/xgb_maccs_stats.npz``), with scikit-learn's histogram booster on problems where every value has its own bin, and with the
numpy restatement.

Refused, each by name: objectives other than ``reg:squarederror``, ``subsample`` / ``colsample_*`` below 1, ``reg_alpha != 0``,
``max_delta_step``, ``grow_policy="lossguide"`` / ``max_leaves``, ``tree_method`` other than ``"hist"`` / ``"auto"``, ``sample_weight``,
``eval_set`` / early stopping, monotone or interaction constraints, categorical features, missing values (NaN) or infinity in ``X`` or
``y``, ``max_depth`` outside 1..1024, more than 8 192 rows, more than 65 536 live features, more than 10 000 trees, more than one GPU.
There is no CPU path.
"""
from __future__ import annotations

import json
import numbers

import numpy as np
import torch

from . import _dense, _lib, _tree_host, boosters
from ._tree_host import is_int as _is_int

MAX_ROWS, MAX_LIVE_FEATURES, MAX_DEPTH, MAX_TREES = 8192, 65536, 1024, 10000          # BBBP_XGB_FIT_MAX_*
_WHO = "XGBRegressor"
_PARAMS = ("n_estimators", "max_depth", "learning_rate", "reg_lambda", "gamma", "min_child_weight", "max_bin", "base_score", "tree_method", "random_state",
           "n_jobs", "device")
_ALIASES = {"eta": "learning_rate", "min_split_loss": "gamma", "lambda": "reg_lambda"}
# XGBoost's further parameters pass with None or the value that leaves the algorithm above unchanged; anything else is refused by name
_NEUTRAL = dict(objective="reg:squarederror", booster="gbtree", subsample=1.0, colsample_bytree=1.0, colsample_bylevel=1.0, colsample_bynode=1.0,
                reg_alpha=0.0, alpha=0.0, max_delta_step=0.0, grow_policy="depthwise", max_leaves=0, monotone_constraints=None,
                interaction_constraints=None, enable_categorical=False, feature_types=None, max_cat_to_onehot=None, max_cat_threshold=None,
                early_stopping_rounds=None, eval_metric=None, num_parallel_tree=1, scale_pos_weight=1.0, sampling_method="uniform",
                importance_type=None, multi_strategy=None, callbacks=None)
_IGNORED = ("verbosity", "validate_parameters")


def _number(v, name, lo, lo_open=False):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not np.isfinite(v) or v < lo or (lo_open and v == lo):
        raise ValueError(f"{_WHO}: {name} must be a finite number {'>' if lo_open else '>='} {lo}, got {v!r}")


def _check_params(n_estimators, max_depth, learning_rate, reg_lambda, gamma, min_child_weight, max_bin, base_score, tree_method):
    if not _is_int(n_estimators) or n_estimators < 1:
        raise ValueError(f"{_WHO}: n_estimators must be an int >= 1, got {n_estimators!r}")
    if n_estimators > MAX_TREES:
        raise NotImplementedError(f"{_WHO}: n_estimators = {n_estimators}: more than {MAX_TREES} trees are not supported")
    if not _is_int(max_depth) or not 1 <= max_depth <= MAX_DEPTH:
        raise NotImplementedError(f"{_WHO}: max_depth must be an int in 1..{MAX_DEPTH} (0 / None, XGBoost's unlimited depth, is not supported), got {max_depth!r}")
    _number(learning_rate, "learning_rate", 0.0, lo_open=True)
    if not np.isfinite(np.float32(learning_rate)) or np.float32(learning_rate) == 0:
        raise ValueError(f"{_WHO}: learning_rate {learning_rate!r} is not a positive finite float32")
    _number(reg_lambda, "reg_lambda", 0.0)
    _number(gamma, "gamma", 0.0)
    _number(min_child_weight, "min_child_weight", 0.0)
    if not _is_int(max_bin) or not 2 <= max_bin <= 256:
        raise NotImplementedError(f"{_WHO}: max_bin must be an int in 2..256 (a bin is one byte), got {max_bin!r}")
    if base_score is not None:
        _number(base_score, "base_score", -np.inf)
        if not np.isfinite(np.float32(base_score)):
            raise ValueError(f"{_WHO}: base_score {base_score!r} is not a finite float32")
    if tree_method not in ("hist", "auto", None):
        raise NotImplementedError(f"{_WHO}: tree_method={tree_method!r} is not supported (only 'hist' and 'auto')")


def _refuse(other):
    for name, value in other.items():
        if name in _IGNORED:
            continue
        if name not in _NEUTRAL:
            raise ValueError(f"{_WHO}: unknown parameter {name}")
        neutral = _NEUTRAL[name]
        if value is None or value is neutral or (isinstance(value, (numbers.Real, str)) and not isinstance(neutral, type(None)) and value == neutral):
            continue
        raise NotImplementedError(f"{_WHO}: {name}={value!r} is not supported (only {neutral!r})")


def _cuda_device(device, who=_WHO):
    if isinstance(device, (list, tuple)):
        raise NotImplementedError(f"{who}: device={device!r}: more than one GPU is not supported")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU path)")
    return dev


# ---- quantisation -----------------------------------------------------------------------------------------------------------------------
def cut_matrix(XT, max_bin):
    """The cuts of every row of ``XT`` [d, n] (one feature per row, float32, finite) as [d, max_bin - 1] float32, ascending and padded
    with +infinity: all distinct values above the minimum for a feature of at most ``max_bin`` distinct values, else the distinct values
    among ``s[floor(j n / max_bin)]`` that exceed the minimum; a cut of -0.0 is stored as +0.0.  Plain torch on ``XT``'s device: sorting is
    plumbing."""
    d, n = XT.shape
    C = max_bin - 1
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=XT.device)
    S = torch.sort(XT, dim=1).values + 0.0              # -0.0 + 0.0 = +0.0: which of the two equal zeros a sort keeps is not defined
    new = S[:, 1:] != S[:, :-1]
    cuts = torch.where(new, S[:, 1:], inf).sort(dim=1).values[:, :C]
    if cuts.shape[1] < C:
        cuts = torch.cat([cuts, inf.expand(d, C - cuts.shape[1])], dim=1)
    cuts = cuts.contiguous()
    many = (new.sum(dim=1) + 1) > max_bin
    if bool(many.any()):
        Sm = S[many]
        picks = Sm[:, torch.tensor([(j * n) // max_bin for j in range(1, max_bin)], device=XT.device)]
        keep = picks > Sm[:, :1]
        keep[:, 1:] &= picks[:, 1:] != picks[:, :-1]
        cuts[many] = torch.where(keep, picks, inf).sort(dim=1).values
    return cuts


class _Upload:
    """One matrix: checked, then on the device its columns that are not constant over all rows, float32, one feature per row, with their
    original indices.  For a numpy input the check and the dropping of constant columns happen on the host and touch no GPU."""

    def __init__(self, X):
        self.on_device = isinstance(X, torch.Tensor)
        if self.on_device and not X.is_cuda:
            raise RuntimeError(f"{_WHO}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU path)")
        if not self.on_device:
            X = np.asarray(X)
        if X.ndim != 2 or X.shape[0] < 2 or X.shape[1] < 1:
            raise ValueError(f"{_WHO}: expected a 2-D [n, d] input of at least two rows and one feature, got shape {tuple(X.shape)}")
        if self.on_device:
            X32 = X.to(torch.float32)
            finite = bool(torch.isfinite(X32).all())
        else:
            with np.errstate(over="ignore"):
                X32 = np.asarray(X, dtype=np.float32)
            finite = bool(np.isfinite(X32).all())
        if not finite:
            raise ValueError(f"{_WHO}: X contains NaN (missing values are not supported in training), infinity or a value too large for float32")
        self.n, self.d = X.shape
        if self.on_device:
            self.cols = (X32.min(dim=0).values != X32.max(dim=0).values).nonzero().flatten().cpu().numpy().astype(np.int64)
        else:
            self.cols = np.flatnonzero(X32.min(axis=0) != X32.max(axis=0)).astype(np.int64)
        self.X32, self.XT = X32, None

    def upload(self, dev):
        if self.XT is None:
            if self.on_device:
                self.XT = self.X32.to(dev)[:, torch.from_numpy(self.cols).to(dev)].t().contiguous()
            else:
                self.XT = torch.from_numpy(np.ascontiguousarray(self.X32[:, self.cols].T)).to(dev)
            self.X32 = None
        return self


class _Bins:
    """The byte matrix of one problem's rows: cuts from those rows alone, their live features, ``bins`` [d_live, n] by ``bbbp_xgb_bin``."""

    def __init__(self, up, rows, max_bin, dev):
        XT = up.XT if rows is None else up.XT[:, torch.from_numpy(rows).to(dev)]
        self.n = XT.shape[1]
        C = max_bin - 1
        if XT.shape[0]:
            cuts = cut_matrix(XT, max_bin)
            live = torch.isfinite(cuts[:, 0])
            XT, cuts = XT[live].contiguous(), cuts[live].contiguous()
            self.cols = up.cols[live.cpu().numpy()]
        if XT.shape[0] == 0:                   # every column constant: one dead feature, so that the kernels have a matrix; it has no boundary
            self.cols = np.zeros(1, np.int64)
            self.cuts = torch.full((1, C), float("inf"), dtype=torch.float32, device=dev)
            self.bins = torch.zeros((1, self.n), dtype=torch.uint8, device=dev)
            self.d = 1
            return
        self.d = XT.shape[0]
        if self.d > MAX_LIVE_FEATURES:
            raise NotImplementedError(f"{_WHO}: {self.d} live features, more than {MAX_LIVE_FEATURES} are not supported (BBBP_XGB_FIT_MAX_D)")
        self.cuts = cuts
        self.bins = torch.empty((self.d, self.n), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().bbbp_xgb_bin(_dense.stream(), XT.data_ptr(), self.n, self.d, cuts.data_ptr(), C, self.bins.data_ptr()), "bbbp_xgb_bin")


class _Problem:
    """One model to fit: its outputs, its work area and the descriptor ``bbbp_xgb_fit`` takes.  Nothing needs initialising."""

    def __init__(self, reg, bins, y, n_features, dev):
        L = _lib.lib()
        n, d, T = bins.n, bins.d, int(reg.n_estimators)
        nbytes, self.cap = L.bbbp_xgb_fit_work_bytes(n, d), L.bbbp_xgb_fit_tree_capacity(n, int(reg.max_depth))
        if not nbytes or not self.cap:
            raise ValueError("xgb: " + L.bbbp_last_error().decode("utf-8", "replace"))
        self.bins, self.n_features, self.T = bins, n_features, T
        self.base_score = np.float32(np.mean(y)) if reg.base_score is None else np.float32(reg.base_score)
        with np.errstate(over="ignore"):
            y32 = y.astype(np.float32)
        if not np.isfinite(y32).all() or not np.isfinite(self.base_score):
            raise ValueError(f"{_WHO}: y holds a value too large for float32")
        self.y = torch.from_numpy(y32).to(dev)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
        f32 = lambda k: torch.empty(k, dtype=torch.float32, device=dev)  # noqa: E731
        self.left, self.right, self.feature = i32(T * self.cap), i32(T * self.cap), i32(T * self.cap)
        self.cond, self.base_weight, self.loss_change, self.sum_hessian = f32(T * self.cap), f32(T * self.cap), f32(T * self.cap), f32(T * self.cap)
        self.tree_nodes, self.margin = i32(T), f32(n)
        min_child_rows = int(min(max(1, np.ceil(float(reg.min_child_weight))), MAX_ROWS + 1))
        self.desc = _lib.XgbProblem(bins.bins.data_ptr(), bins.cuts.data_ptr(), self.y.data_ptr(), n, d, bins.cuts.shape[1], T, int(reg.max_depth),
                                    min_child_rows, float(reg.reg_lambda), float(reg.gamma), float(np.float32(reg.learning_rate)), float(self.base_score),
                                    self.work.data_ptr(), self.left.data_ptr(), self.right.data_ptr(), self.feature.data_ptr(), self.cond.data_ptr(),
                                    self.base_weight.data_ptr(), self.loss_change.data_ptr(), self.sum_hessian.data_ptr(), self.tree_nodes.data_ptr(),
                                    self.margin.data_ptr())

    def trees(self):
        """The fitted trees as flat host arrays in ``boosters.XGBTrees``' convention, with the recorded statistics; the one host read of a fit."""
        counts = self.tree_nodes.cpu().numpy().astype(np.int64)
        if (counts < 1).any():
            raise RuntimeError(f"xgb: the fit kernels reported an index outside its array in tree {int(np.argmax(counts < 1))} "
                               "(a defect of csrc/xgb.hip, not of the data); no model is returned")
        root = np.concatenate([[0], np.cumsum(counts)])
        keep = (np.arange(self.cap)[None, :] < counts[:, None]).ravel()
        pick = lambda a: a.cpu().numpy()[keep]  # noqa: E731
        left, right = _tree_host.rebase_children(pick(self.left), pick(self.right), np.repeat(root[:-1], counts))
        feature = pick(self.feature)
        feature = np.where(left >= 0, self.bins.cols[feature], 0).astype(np.int32)          # the original column of a live feature
        return _with_parents(dict(left=left, right=right, feature=feature, cond=pick(self.cond), default_left=np.zeros(len(left), np.uint8),
                                  root=root.astype(np.int32), base_weights=pick(self.base_weight), loss_changes=pick(self.loss_change),
                                  sum_hessian=pick(self.sum_hessian)))


def _with_parents(trees):
    parents = np.full(len(trees["left"]), -1, np.int32)
    inner = np.flatnonzero(trees["left"] >= 0)
    parents[trees["left"][inner]] = inner
    parents[trees["right"][inner]] = inner
    return {**trees, "parents": parents}


def _run(problems, dev):
    arr = (_lib.XgbProblem * len(problems))(*[p.desc for p in problems])
    on_device = _tree_host.upload(arr, dev)
    alive = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().bbbp_xgb_fit(_dense.stream(), arr, on_device.data_ptr(), len(problems), alive.data_ptr()), "bbbp_xgb_fit")
    return on_device, alive                           # the fit has synchronised the stream; kept alive by the caller all the same


class XGBRegressor:
    """``XGBRegressor(n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, max_bin=256,
    base_score=None, tree_method="hist", random_state=None, device="cuda")``: XGBoost's names; the aliases ``eta``, ``min_split_loss`` and
    ``lambda`` are accepted, ``random_state`` and ``n_jobs`` are accepted and unused (nothing is random: the tie rule is fixed).

    ``fit(X, y)`` takes a numpy array or a CUDA tensor [n, d], float32 or float64 (cast to float32), ``2 <= n <= 8 192``, and finite targets.
    It sets ``booster_`` (a ``boosters.XGBTrees`` of the fitted arrays; ``predict`` is its ``predict``), ``trees_`` (the flat host arrays
    ``left``, ``right``, ``feature``, ``cond``, ``default_left``, ``root`` of ``XGBTrees`` and ``base_weights``, ``loss_changes``,
    ``sum_hessian``, ``parents`` -- absolute indices, -1 at a root), ``base_score_``, ``n_features_in_`` and ``train_margin_`` (float32: the
    training rows' margins as the fit summed them).  ``get_model_json`` / ``save_model`` write XGBoost's published JSON schema.
    ``get_params`` / ``set_params`` make ``sklearn.base.clone`` and ``ensemble.StackingRegressor`` work.  The module docstring states the
    algorithm, the quantile-cut deviation, the unpinned parity with the xgboost package and everything that is refused."""

    def __init__(self, n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, max_bin=256, base_score=None,
                 tree_method="hist", random_state=None, n_jobs=None, device="cuda", **other):
        given = dict(learning_rate=learning_rate, gamma=gamma, reg_lambda=reg_lambda)
        for alias, name in _ALIASES.items():
            if alias in other:
                given[name] = other.pop(alias)
        _refuse(other)
        learning_rate, gamma, reg_lambda = given["learning_rate"], given["gamma"], given["reg_lambda"]
        _check_params(n_estimators, max_depth, learning_rate, reg_lambda, gamma, min_child_weight, max_bin, base_score, tree_method)
        if isinstance(device, (list, tuple)):
            raise NotImplementedError(f"{_WHO}: device={device!r}: more than one GPU is not supported")
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.n_estimators, self.max_depth, self.learning_rate, self.reg_lambda, self.gamma = n_estimators, max_depth, learning_rate, reg_lambda, gamma
        self.min_child_weight, self.max_bin, self.base_score, self.tree_method = min_child_weight, max_bin, base_score, tree_method
        self.random_state, self.n_jobs, self.device = random_state, n_jobs, device

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in _PARAMS}

    def set_params(self, **params):
        params = {_ALIASES.get(k, k): v for k, v in params.items()}
        unknown = set(params) - set(_PARAMS)
        if unknown:
            raise ValueError(f"{_WHO}: unknown parameters {sorted(unknown)}")
        type(self)(**{**self.get_params(), **params})
        for name, value in params.items():
            setattr(self, name, value)
        return self

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None, eval_set=None, **other):
        if sample_weight is not None:
            raise NotImplementedError(f"{_WHO}: sample_weight is not supported")
        if eval_set is not None or other.get("early_stopping_rounds") is not None:
            raise NotImplementedError(f"{_WHO}: eval_set and early stopping are not supported")
        if set(other) - {"early_stopping_rounds", "verbose"}:
            raise NotImplementedError(f"{_WHO}: fit arguments {sorted(set(other) - {'early_stopping_rounds', 'verbose'})} are not supported")
        _fit([self], [(X, y)])
        return self

    def _adopt(self, trees, base_score, n_features, train_margin=None):
        self.trees_, self.base_score_, self.n_features_in_, self.train_margin_ = trees, np.float32(base_score), int(n_features), train_margin
        self.booster_ = boosters.XGBTrees(trees["left"], trees["right"], trees["feature"], trees["cond"], trees["default_left"], trees["root"],
                                          int(n_features), float(base_score), device=self.device)
        return self

    @classmethod
    def from_trees(cls, trees, base_score, n_features, device="cuda", **params):
        """A regressor around fitted arrays (``trees_``' keys; ``parents`` is derived when absent): for prediction and the JSON export.
        ``device="cpu"`` gives a model that exports and validates but cannot predict."""
        self = cls(device=device, **params)
        trees = {k: np.asarray(v) for k, v in trees.items()}
        return self._adopt(trees if "parents" in trees else _with_parents(trees), base_score, n_features)

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _fitted(self):
        if not hasattr(self, "booster_"):
            raise RuntimeError(f"{_WHO}: not fitted")
        return self.booster_

    def predict(self, X):
        """float32 [m]: ``base_score_`` plus the trees' leaf values (``bbbp_gbt_predict``); numpy for numpy queries, a CUDA tensor for a CUDA tensor."""
        out = self._fitted().predict_device(X)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict_device(self, X):
        return self._fitted().predict_device(X)

    # ---- export -----------------------------------------------------------------------------------------------------
    def get_model_json(self):
        """The model as a JSON document in XGBoost's published schema (``learner.gradient_booster.model.trees[*]`` with every array the
        shipped model carries, ``learner_model_param``, ``objective``); ``boosters.XGBTrees.from_raw`` reads it back to the same arrays.
        That XGBoost itself loads it is UNPINNED: the package is absent (see the module docstring)."""
        self._fitted()
        t, nf = self.trees_, str(self.n_features_in_)
        root = t["root"].astype(np.int64)
        trees = []
        for i in range(len(root) - 1):
            lo, hi = int(root[i]), int(root[i + 1])
            local = lambda a: [int(c) - lo if c >= 0 else -1 for c in a[lo:hi]]  # noqa: E731
            f32 = lambda a: [float(x) for x in np.asarray(a[lo:hi], np.float32)]  # noqa: E731
            trees.append({"base_weights": f32(t["base_weights"]), "categories": [], "categories_nodes": [], "categories_segments": [],
                          "categories_sizes": [], "default_left": [int(x) for x in t["default_left"][lo:hi]], "id": i,
                          "left_children": local(t["left"]), "loss_changes": f32(t["loss_changes"]),
                          "parents": [int(c) - lo if c >= 0 else 2147483647 for c in t["parents"][lo:hi]], "right_children": local(t["right"]),
                          "split_conditions": f32(t["cond"]), "split_indices": [int(x) for x in t["feature"][lo:hi]], "split_type": [0] * (hi - lo),
                          "sum_hessian": f32(t["sum_hessian"]),
                          "tree_param": {"num_deleted": "0", "num_feature": nf, "num_nodes": str(hi - lo), "size_leaf_vector": "1"}})
        T = len(trees)
        doc = {"learner": {"attributes": {}, "feature_names": [], "feature_types": [],
                           "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1", "num_trees": str(T)},
                                                          "iteration_indptr": list(range(T + 1)), "tree_info": [0] * T, "trees": trees},
                                                "name": "gbtree"},
                           "learner_model_param": {"base_score": f"{float(self.base_score_):.8E}", "boost_from_average": "1", "num_class": "0",
                                                   "num_feature": nf, "num_target": "1"},
                           "objective": {"name": "reg:squarederror", "reg_loss_param": {"scale_pos_weight": "1"}}},
               "version": [2, 0, 0]}
        return json.dumps(doc)

    def save_model(self, path):
        with open(path, "w") as f:
            f.write(self.get_model_json())


def _fit(regressors, problems):
    """Fit ``regressors[i]`` on ``problems[i] = (X, y)`` or ``(X, y, rows)`` in one ``bbbp_xgb_fit`` batch.  Problems over one matrix object
    share its upload; they share a bin matrix too when their rows and ``max_bin`` are the same, which is when their cuts are equal for
    certain.  Cuts are per problem, from the problem's own rows: a fold fitted in a batch equals the fold fitted alone."""
    devices = {str(_cuda_device(reg.device)) for reg in regressors}
    if len(devices) != 1:
        raise NotImplementedError(f"{_WHO}: the regressors of one batch name the devices {sorted(devices)}: more than one GPU is not supported")
    dev = _cuda_device(regressors[0].device)
    checked, uploads = [], {}
    for prob in problems:
        if len(prob) not in (2, 3):
            raise ValueError(f"{_WHO}: a problem is (X, y) or (X, y, rows), got {len(prob)} items")
        X, y, rows = prob[0], prob[1], (prob[2] if len(prob) == 3 else None)
        n_all = X.shape[0] if hasattr(X, "shape") and len(X.shape) == 2 else None
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.ndim != 1 or n_all is None or (len(rows) and (rows.min() < 0 or rows.max() >= n_all)):
                raise ValueError(f"{_WHO}: rows must be a 1-D array of row indices of X")
        n = len(rows) if rows is not None else n_all
        if n is not None and n > MAX_ROWS:
            raise NotImplementedError(f"{_WHO}: n = {n} rows, more than {MAX_ROWS} are not supported (BBBP_XGB_FIT_MAX_N)")
        if n is not None and n < 2:
            raise ValueError(f"{_WHO}: at least two rows are needed, got {n}")
        y_all = _tree_host.targets_1d(y, n_all, _WHO, "more than one output column is not supported")
        if id(X) not in uploads:
            uploads[id(X)] = _Upload(X)
        if rows is None and len(uploads[id(X)].cols) > MAX_LIVE_FEATURES:
            raise NotImplementedError(f"{_WHO}: {len(uploads[id(X)].cols)} live features, more than {MAX_LIVE_FEATURES} are not supported (BBBP_XGB_FIT_MAX_D)")
        checked.append((X, y_all if rows is None else y_all[rows], rows))
    with torch.cuda.device(dev):
        binned, fits = {}, []
        for reg, (X, y, rows) in zip(regressors, checked):
            up = uploads[id(X)].upload(dev)
            key = (id(X), None if rows is None else rows.tobytes(), int(reg.max_bin))
            if key not in binned:
                binned[key] = _Bins(up, rows, int(reg.max_bin), dev)
            fits.append(_Problem(reg, binned[key], y, up.d, dev))
        keep = _run(fits, dev)
        for reg, fit in zip(regressors, fits):
            reg._adopt(fit.trees(), fit.base_score, fit.n_features, fit.margin.cpu().numpy())
        del keep


def fit_regressors(problems, **params):
    """``[XGBRegressor(**params).fit(X[rows], y[rows]) for X, y, rows in problems]`` with every problem in one batch (``(X, y)`` means all
    rows): the reference's five folds and the refit are one call.  Each regressor equals its single ``fit`` bit for bit."""
    problems = list(problems)
    if not problems:
        raise ValueError("xgb.fit_regressors: no problems")
    regressors = [XGBRegressor(**params) for _ in problems]
    _fit(regressors, problems)
    return regressors
