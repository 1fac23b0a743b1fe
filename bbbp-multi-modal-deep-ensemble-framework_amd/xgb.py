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

*Curves and the best iteration, after the fit.*  ``eval_set`` stays refused inside ``fit``: the fit is deterministic and no validation row
influences a tree, so ``eval_curves(eval_set, period=1)`` computes XGBoost's ``evals_result()`` (``{"validation_k": {"rmse": [...]}}``)
afterwards, from one walk of the trees per eval set (``boosters.XGBTrees.staged_predict_device``) and one ``metrics.squared_error_sums``
launch for all stages; ``staged_predict``, ``predict(X, iteration_range=(begin, end))``, ``boosters.best_iteration`` and ``shrink(tree_end)``
complete it (the reference's ``Models/multi_input_data_regression_opt_transformer_cnn_20250113.py:291-312``).  No training stops early: a
fit of T trees is a prefix of a longer one, so cutting the full fit gives the same model.  RMSE takes ``y`` as float64; XGBoost's float32
labels and its stage convention for periods above 1 are unpinned.

``XGBClassifier``: the same trees under ``binary:logistic``, fitted by ``csrc/xgbc.hip``.  The reference's newest classification script stacks
and votes with ``XGBClassifier(use_label_encoder=False, eval_metric="logloss", learning_rate=0.02, n_estimators=500, max_depth=7,
colsample_bytree=0.8, subsample=0.8, reg_lambda=3, tree_method="hist", device="cuda")`` (``Models/model_opt_20250130.py:445-456``) and searches
it with ``RandomizedSearchCV`` (``:533-561``; here ``randomized_search_cv``).  ``tests/xgbc_numpy.py`` restates what follows in numpy and the GPU
fit equals that bit for bit.  Everything not mentioned is the regressor's rule, unchanged: quantisation and cuts, the gain in float64 with
every operation rounded on its own, the tie rule, ``kRtEps``, node ids, float32 leaf values, margins added in float32.

*Labels.*  Exactly two classes: ``classes_ = np.unique(y)`` and ``t = (y == classes_[1])``; anything else is refused by name.

*Initial margin.*  With ``base_score=None``, ``m0 = float32(4 (mean(t) - 0.5))``, the product formed in float64 on the host: the one Newton
step from margin 0 (``g = 1/2 - mean(t)``, ``h = 1/4``) that XGBoost 2.0 takes for its intercept, as far as can be told without the package --
UNPINNED like the rest of the parity; ``base_score_ = sigmoid32(m0)``, a probability.  A given ``base_score`` must lie strictly inside
(0, 1); then ``m0 = float32(log(p / (1 - p)))``, formed in float64 on the host, and ``base_score_ = float32(p)``.

*sigmoid32(x)* of a float32 margin, from IEEE operations only, so that numpy and the device agree bit for bit (``csrc/xgbc.hip`` is compiled
with ``-ffp-contract=off``): ``z = (double)x``, ``a = max(-|z|, -87.0)`` (the clamp keeps p a normal float32); ``k = rint(a INV_LN2)``,
``r = (a - k LN2_HI) - k LN2_LO``; ``P = sum_{j=0..13} c_j r^j`` by Horner from ``c_13`` down with ``c_j = 1.0 / (double)(j!)``;
``e = ldexp(P, (int)k)``; ``s = 1 / (1 + e)`` if ``z >= 0`` else ``e / (1 + e)``; ``p = (float)s``.  The constants are fdlibm's:
``LN2_HI = 0x1.62e42fee00000p-1``, ``LN2_LO = 0x1.a39ef35793c76p-33``, ``INV_LN2 = 0x1.71547652b82fep+0``.  On the float32 margins tested
(``tests/test_xgbc_cpu.py``) it equals the float32 rounding of a long-double sigmoid and is monotone.  XGBoost itself uses a float32 ``expf``,
whose last bit can differ from this.

*Gradients per tree.*  ``p_i = sigmoid32(margin_i)``, ``g_i = p_i - float32(t_i)`` and ``h_i = p_i (1 - p_i)`` in float32, the subtraction
and the product each rounded on its own.  A row that the tree's draw left out (below) has ``q_i = r_i = 0``; it stays in the row list and
gets its leaf's value like any other row, as in XGBoost.  For sampled rows ``gmax``, ``k`` and ``q_i`` are the regressor's, ``gmax`` taken over
the sampled rows only, and ``r_i = max(1, llrint(ldexp((double)h_i, 48)))``: ``h <= 1/4`` gives ``r_i <= 2^46``, so with ``n <= 8 192``
``R = sum r_i <= 2^59`` is an exact integer in any order and ``H = ldexp((double)R, -48)`` is one rounding, like ``G``.

*Candidates and stop rule.*  A boundary is a candidate iff ``m_L >= 1``, ``m_R >= 1``, ``R_L >= 1``, ``R_R >= 1``, ``H_L >= min_child_weight``
and ``H_R >= min_child_weight`` (float64 comparisons; rows are not counted up to a ceiling any more).  ``gain``, ``w = -G / (H + lambda)``,
``gamma``, ``kRtEps`` and ``max_depth`` are as before.  A node with ``R = 0`` (every row unsampled) is a leaf of weight 0, stored as -0.0 like
the regressor's zero leaf.  A child is searched iff the tree may go deeper and the child has at least two rows.  Recorded ``sum_hessian =
(float)H``.

*Sampling*, this module's own counter-based rule, A DELIBERATE DEVIATION from XGBoost's ``mt19937``: ``seed = random_state`` (``None``: 0,
XGBoost's default); ``mix(x)``: ``x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31`` modulo 2^64;
``u(stream, tree, i) = mix(mix(mix(seed + 0x9E3779B97F4A7C15 (stream + 1)) + tree) + i)``.  Rows are stream 0 and ``i`` is the row's
position within the problem, so a fold fitted in a batch equals the fold fitted alone; a row is sampled iff ``(u >> 32) < floor(subsample
2^32)`` (at least 1), on the device in the tree-start code; ``subsample = 1`` samples nothing out.  Columns are stream 1 and ``i`` is the
original column index: per tree the ``max(1, floor(colsample_bytree d_live))`` live columns with the smallest ``(u, i)`` are eligible,
computed on the host for all trees at once and uploaded as a bit mask.  XGBoost draws from all columns, constant ones included; this draws
from the live ones.  The draw for tree ``t`` does not depend on ``n_estimators``: a model of T trees is the prefix of a longer one even
with sampling, which ``randomized_search_cv`` relies on.

*Accepted*: ``n_estimators``, ``max_depth``, ``learning_rate`` / ``eta``, ``reg_lambda`` / ``lambda``, ``gamma`` / ``min_split_loss``,
``min_child_weight``, ``max_bin``, ``base_score``, ``subsample`` and ``colsample_bytree`` in (0, 1], ``tree_method``, ``random_state``,
``n_jobs``, ``device``; ``objective`` only as ``None`` or ``"binary:logistic"``, ``eval_metric`` only as ``None`` or ``"logloss"``;
``use_label_encoder`` is ignored.  Refused by name: ``scale_pos_weight != 1``, ``colsample_bylevel`` / ``colsample_bynode`` below 1, and
everything else the regressor refuses.
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


def _number(v, name, lo, lo_open=False, who=_WHO):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not np.isfinite(v) or v < lo or (lo_open and v == lo):
        raise ValueError(f"{who}: {name} must be a finite number {'>' if lo_open else '>='} {lo}, got {v!r}")


def _check_params(n_estimators, max_depth, learning_rate, reg_lambda, gamma, min_child_weight, max_bin, base_score, tree_method, who=_WHO):
    if not _is_int(n_estimators) or n_estimators < 1:
        raise ValueError(f"{who}: n_estimators must be an int >= 1, got {n_estimators!r}")
    if n_estimators > MAX_TREES:
        raise NotImplementedError(f"{who}: n_estimators = {n_estimators}: more than {MAX_TREES} trees are not supported")
    if not _is_int(max_depth) or not 1 <= max_depth <= MAX_DEPTH:
        raise NotImplementedError(f"{who}: max_depth must be an int in 1..{MAX_DEPTH} (0 / None, XGBoost's unlimited depth, is not supported), got {max_depth!r}")
    _number(learning_rate, "learning_rate", 0.0, lo_open=True, who=who)
    if not np.isfinite(np.float32(learning_rate)) or np.float32(learning_rate) == 0:
        raise ValueError(f"{who}: learning_rate {learning_rate!r} is not a positive finite float32")
    _number(reg_lambda, "reg_lambda", 0.0, who=who)
    _number(gamma, "gamma", 0.0, who=who)
    _number(min_child_weight, "min_child_weight", 0.0, who=who)
    if not _is_int(max_bin) or not 2 <= max_bin <= 256:
        raise NotImplementedError(f"{who}: max_bin must be an int in 2..256 (a bin is one byte), got {max_bin!r}")
    if base_score is not None:
        _number(base_score, "base_score", -np.inf, who=who)
        if not np.isfinite(np.float32(base_score)):
            raise ValueError(f"{who}: base_score {base_score!r} is not a finite float32")
    if tree_method not in ("hist", "auto", None):
        raise NotImplementedError(f"{who}: tree_method={tree_method!r} is not supported (only 'hist' and 'auto')")


def _refuse(other, neutrals=_NEUTRAL, ignored=_IGNORED, who=_WHO):
    for name, value in other.items():
        if name in ignored:
            continue
        if name not in neutrals:
            raise ValueError(f"{who}: unknown parameter {name}")
        neutral = neutrals[name]
        if value is None or value is neutral or (isinstance(value, (numbers.Real, str)) and not isinstance(neutral, type(None)) and value == neutral):
            continue
        raise NotImplementedError(f"{who}: {name}={value!r} is not supported (only {neutral!r})")


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

    def __init__(self, X, who=_WHO):
        self.on_device = isinstance(X, torch.Tensor)
        if self.on_device and not X.is_cuda:
            raise RuntimeError(f"{who}: expected a CUDA (HIP) tensor or a numpy array, got a tensor on {X.device} (no CPU path)")
        if not self.on_device:
            X = np.asarray(X)
        if X.ndim != 2 or X.shape[0] < 2 or X.shape[1] < 1:
            raise ValueError(f"{who}: expected a 2-D [n, d] input of at least two rows and one feature, got shape {tuple(X.shape)}")
        if self.on_device:
            X32 = X.to(torch.float32)
            finite = bool(torch.isfinite(X32).all())
        else:
            with np.errstate(over="ignore"):
                X32 = np.asarray(X, dtype=np.float32)
            finite = bool(np.isfinite(X32).all())
        if not finite:
            raise ValueError(f"{who}: X contains NaN (missing values are not supported in training), infinity or a value too large for float32")
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

    def __init__(self, up, rows, max_bin, dev, who=_WHO):
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
            raise NotImplementedError(f"{who}: {self.d} live features, more than {MAX_LIVE_FEATURES} are not supported (BBBP_XGB_FIT_MAX_D)")
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

    def predict(self, X, iteration_range=None):
        """float32 [m]: ``base_score_`` plus the trees' leaf values (``bbbp_gbt_predict``); numpy for numpy queries, a CUDA tensor for a CUDA tensor.
        ``iteration_range=(begin, end)`` is XGBoost's: the trees ``[begin, end)`` only, ``end = 0`` meaning all of them (one stage of
        ``bbbp_gbt_staged_predict``); ``None`` and ``(0, 0)`` are the whole model."""
        booster = self._fitted()
        if iteration_range is None or tuple(iteration_range) == (0, 0):
            out = booster.predict_device(X)
        else:
            if len(iteration_range) != 2 or not all(_is_int(v) for v in iteration_range):
                raise ValueError(f"{_WHO}: iteration_range must be two ints (begin, end), got {iteration_range!r}")
            begin, end = iteration_range
            end = booster.n_trees if end == 0 else end
            boosters._check_tree_range(f"{_WHO}.predict", booster.n_trees, begin, end)
            out = booster.staged_predict_device(X, begin, end, period=end - begin)[0]
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict_device(self, X):
        return self._fitted().predict_device(X)

    def staged_predict(self, X, period=1):
        """float32 ``[K, m]``: row ``k`` is the prediction of the first ``min((k + 1) period, T)`` trees, all from one walk of the trees
        (``boosters.XGBTrees.staged_predict_device``); the last row is ``predict(X)`` bit for bit.  numpy for numpy queries, a CUDA tensor
        for a CUDA tensor."""
        out = self._fitted().staged_predict_device(X, period=period)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def eval_curves(self, eval_set, period=1):
        """``{"validation_0": {"rmse": [...]}, "validation_1": ...}``, the layout of XGBoost's ``evals_result()``, for a list of ``(X, y)``
        pairs: the RMSE of every stage of ``staged_predict(X, period)`` against ``y``.  What ``fit(..., eval_set=...)`` records in XGBoost,
        computed after the fit: the fit is deterministic and no validation row influences a tree.  Per pair the staged matrix stays on the
        device and ``metrics.squared_error_sums`` scores its ``K`` rows in one launch (``y`` as float64 -- XGBoost's float32 labels are not
        reproduced); ``sqrt(sse / n)`` is formed on the host.  A non-finite ``y`` or prediction raises ``ValueError``.  The result is kept
        in ``evals_result_``."""
        booster = self._fitted()
        result = {f"validation_{i}": {"rmse": boosters.rmse_curve(booster.staged_predict_device(X, period=period), y)}
                  for i, (X, y) in enumerate(boosters.eval_pairs(eval_set, _WHO))}
        self.evals_result_ = result
        return result

    def evals_result(self):
        """What the last ``eval_curves`` call returned."""
        if not hasattr(self, "evals_result_"):
            raise RuntimeError(f"{_WHO}: no evaluation results: call eval_curves(eval_set) first (fit takes no eval_set)")
        return self.evals_result_

    def shrink(self, tree_end):
        """Keep the trees ``[0, tree_end)`` in place: ``trees_`` and ``booster_`` are rebuilt, ``train_margin_`` becomes ``None``, the
        constructor parameters stay (``n_estimators`` included, so a clone fits the full count again).  The result is the model a fit of
        ``tree_end`` trees gives: a shorter fit is a prefix of a longer one.  Returns ``self``."""
        self._fitted()
        t = self.trees_
        boosters._check_tree_range(f"{_WHO}.shrink", len(t["root"]) - 1, 0, tree_end)
        nodes = int(t["root"][tree_end])
        trees = {k: (np.asarray(v)[:tree_end + 1] if k == "root" else np.asarray(v)[:nodes]).copy() for k, v in t.items()}
        return self._adopt(trees, self.base_score_, self.n_features_in_)

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


# ---- classification: XGBClassifier under binary:logistic ------------------------------------------------------------------------------------
_CWHO = "XGBClassifier"
_CLASSIFIER_PARAMS = _PARAMS[:8] + ("subsample", "colsample_bytree") + _PARAMS[8:]
_CLASSIFIER_NEUTRAL = {**{k: v for k, v in _NEUTRAL.items() if k not in ("subsample", "colsample_bytree")}, "objective": "binary:logistic",
                       "eval_metric": "logloss"}
_CLASSIFIER_IGNORED = _IGNORED + ("use_label_encoder",)
LN2_HI, LN2_LO, INV_LN2 = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33"), float.fromhex("0x1.71547652b82fep+0")
_EXP_COEFFS = tuple(1.0 / float(np.prod(np.arange(1, j + 1, dtype=np.float64))) for j in range(14))         # 1 / j!
_GOLDEN, _ROW_STREAM, _COLUMN_STREAM = 0x9E3779B97F4A7C15, 0, 1


def sigmoid32(x):
    """``sigmoid32`` of the module docstring on the host: float32 probabilities of float32 margins, the bits ``csrc/xgbc.hip`` gives."""
    z = np.asarray(x, np.float32).astype(np.float64)
    a = np.maximum(-np.abs(z), -87.0)
    k = np.rint(a * INV_LN2)
    r = (a - k * LN2_HI) - k * LN2_LO
    P = np.full_like(r, _EXP_COEFFS[13])
    for j in range(12, -1, -1):
        P = P * r + _EXP_COEFFS[j]
    e = np.ldexp(P, k.astype(np.int32))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(np.float32)


def _mix(x):
    x = np.array(x, dtype=np.uint64, ndmin=1)                # uint64 arrays wrap modulo 2^64
    x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def sample_hash(seed, stream, tree, i):
    """``u(stream, tree, i)`` of the module docstring as uint64, broadcast over ``tree`` and ``i``."""
    s = np.full(1, (int(seed) + _GOLDEN * (int(stream) + 1)) % 2 ** 64, np.uint64)
    return _mix(_mix(_mix(s) + np.asarray(tree, np.uint64)) + np.asarray(i, np.uint64))


def _subsample_threshold(subsample):
    return 0 if subsample >= 1.0 else max(1, int(np.floor(float(subsample) * 2.0 ** 32)))


def row_sample(seed, tree, n, subsample):
    """bool [n]: the rows tree ``tree`` uses (the host's copy of the draw the tree-start code makes on the device)."""
    thr = _subsample_threshold(subsample)
    if thr == 0:
        return np.ones(n, bool)
    return (sample_hash(seed, _ROW_STREAM, tree, np.arange(n)) >> np.uint64(32)) < np.uint64(thr)


def column_masks(seed, n_trees, cols, colsample_bytree):
    """bool [n_trees, len(cols)]: per tree the ``max(1, floor(colsample_bytree d_live))`` live columns with the smallest ``(u, original index)``."""
    cols = np.asarray(cols, np.int64)
    masks = np.ones((n_trees, len(cols)), bool)
    if colsample_bytree >= 1.0:
        return masks
    keep = max(1, int(np.floor(float(colsample_bytree) * len(cols))))
    u = sample_hash(seed, _COLUMN_STREAM, np.arange(n_trees)[:, None], cols[None, :])
    masks[:] = False
    np.put_along_axis(masks, np.argsort(u, axis=1, kind="stable")[:, :keep], True, axis=1)      # cols ascend: stable is (u, index)
    return masks


def _pack_masks(masks):
    """bool [T, d] as uint32 [T, ceil(d / 32)], feature f in bit f % 32 of word f / 32."""
    T, d = masks.shape
    words = (d + 31) // 32
    padded = np.zeros((T, words * 32), np.uint8)
    padded[:, :d] = masks
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").reshape(T, words)


def _initial_margin(t, base_score):
    """(m0, base_score_) as float32: one Newton step from margin 0, or the logit of the given probability."""
    if base_score is None:
        m0 = np.float32(4.0 * (float(np.mean(np.asarray(t, np.float64))) - 0.5))
        return m0, np.float32(sigmoid32(m0)[()])
    p = float(base_score)
    return np.float32(np.log(p / (1.0 - p))), np.float32(p)


def _check_classifier_params(p, who=_CWHO):
    _check_params(p["n_estimators"], p["max_depth"], p["learning_rate"], p["reg_lambda"], p["gamma"], p["min_child_weight"], p["max_bin"], None,
                  p["tree_method"], who=who)
    if p["base_score"] is not None:
        _number(p["base_score"], "base_score", 0.0, lo_open=True, who=who)
        if not p["base_score"] < 1 or not np.isfinite(np.float32(np.log(float(p["base_score"]) / (1.0 - float(p["base_score"]))))):
            raise ValueError(f"{who}: base_score must be a probability strictly inside (0, 1), got {p['base_score']!r}")
    for name in ("subsample", "colsample_bytree"):
        _number(p[name], name, 0.0, lo_open=True, who=who)
        if p[name] > 1:
            raise ValueError(f"{who}: {name} must lie in (0, 1], got {p[name]!r}")
    rs = p["random_state"]
    if rs is not None and (not _is_int(rs) or not 0 <= rs < 2 ** 64):
        raise NotImplementedError(f"{who}: random_state must be None or an int in 0..2^64-1 (generator objects are not supported), got {rs!r}")


def _binary_labels(y, n_rows, who=_CWHO):
    """(classes_, t): ``np.unique(y)`` of exactly two classes and the targets 0 / 1 as float32 [n_rows]."""
    y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
    if y.ndim == 2 and y.shape[1] == 1:
        y = y[:, 0]
    if y.ndim != 1 or (n_rows is not None and len(y) != n_rows):
        raise ValueError(f"{who}: y must hold one label per row of X, got shape {tuple(y.shape)} for {n_rows} rows")
    if y.dtype.kind == "f" and not np.isfinite(y).all():
        raise ValueError(f"{who}: y contains NaN or infinity")
    classes = np.unique(y)
    if len(classes) != 2:
        raise ValueError(f"{who}: y must hold exactly two classes (objective binary:logistic), got {len(classes)}: {classes[:5]!r}")
    return classes, (y == classes[1]).astype(np.float32)


class _ClassifierProblem(_Problem):
    """One classifier to fit: outputs, work area, the tree's column masks and the descriptor ``bbbp_xgbc_fit`` takes."""

    def __init__(self, clf, bins, classes, t, n_features, dev):
        L = _lib.lib()
        n, d, T = bins.n, bins.d, int(clf.n_estimators)
        nbytes, self.cap = L.bbbp_xgbc_fit_work_bytes(n, d), L.bbbp_xgbc_fit_tree_capacity(n, int(clf.max_depth))
        if not nbytes or not self.cap:
            raise ValueError("xgb: " + L.bbbp_last_error().decode("utf-8", "replace"))
        self.bins, self.n_features, self.T, self.classes = bins, n_features, T, classes
        self.base_margin, self.base_score = _initial_margin(t, clf.base_score)
        seed = 0 if clf.random_state is None else int(clf.random_state)
        self.y = torch.from_numpy(t).to(dev)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
        f32 = lambda k: torch.empty(k, dtype=torch.float32, device=dev)  # noqa: E731
        self.left, self.right, self.feature = i32(T * self.cap), i32(T * self.cap), i32(T * self.cap)
        self.cond, self.base_weight, self.loss_change, self.sum_hessian = f32(T * self.cap), f32(T * self.cap), f32(T * self.cap), f32(T * self.cap)
        self.tree_nodes, self.margin = i32(T), f32(n)
        self.col_mask, stride = None, 0
        if clf.colsample_bytree < 1:
            packed = _pack_masks(column_masks(seed, T, bins.cols, clf.colsample_bytree))
            stride = packed.shape[1]
            self.col_mask = torch.empty((T, stride), dtype=torch.int32, device=dev)
            self.col_mask.copy_(torch.from_numpy(packed.view(np.int32)))
        self.desc = _lib.XgbcProblem(bins.bins.data_ptr(), bins.cuts.data_ptr(), self.y.data_ptr(), n, d, bins.cuts.shape[1], T, int(clf.max_depth),
                                     _subsample_threshold(clf.subsample), float(clf.reg_lambda), float(clf.gamma), float(clf.min_child_weight),
                                     float(np.float32(clf.learning_rate)), float(self.base_margin), seed,
                                     self.col_mask.data_ptr() if self.col_mask is not None else None, stride,
                                     self.work.data_ptr(), self.left.data_ptr(), self.right.data_ptr(), self.feature.data_ptr(), self.cond.data_ptr(),
                                     self.base_weight.data_ptr(), self.loss_change.data_ptr(), self.sum_hessian.data_ptr(), self.tree_nodes.data_ptr(),
                                     self.margin.data_ptr())


def _run_classifiers(problems, dev):
    arr = (_lib.XgbcProblem * len(problems))(*[p.desc for p in problems])
    on_device = _tree_host.upload(arr, dev)
    alive = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().bbbp_xgbc_fit(_dense.stream(), arr, on_device.data_ptr(), len(problems), alive.data_ptr()), "bbbp_xgbc_fit")
    return on_device, alive


def _proba_of_margin(margin):
    """float32 [m, 2] on the margins' device: ``bbbp_xgbc_proba``."""
    margin = margin.contiguous()
    out = torch.empty((margin.shape[0], 2), dtype=torch.float32, device=margin.device)
    with torch.cuda.device(margin.device):
        _lib.check(_lib.lib().bbbp_xgbc_proba(_dense.stream(), margin.data_ptr(), margin.shape[0], out.data_ptr()), "bbbp_xgbc_proba")
    return out


class XGBClassifier:
    """``XGBClassifier(n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, max_bin=256,
    base_score=None, subsample=1.0, colsample_bytree=1.0, tree_method="hist", random_state=None, device="cuda")``: XGBoost's names for two
    classes under ``binary:logistic``; the aliases ``eta``, ``min_split_loss`` and ``lambda`` are accepted, ``objective="binary:logistic"``,
    ``eval_metric="logloss"`` and ``use_label_encoder`` pass, ``n_jobs`` is unused.  The reference's ``XGBClassifier(use_label_encoder=False,
    eval_metric="logloss", learning_rate=0.02, n_estimators=500, max_depth=7, colsample_bytree=0.8, subsample=0.8, reg_lambda=3,
    tree_method="hist", device="cuda")`` (Models/model_opt_20250130.py:445-456) builds as written.

    ``fit(X, y)`` takes a numpy array or a CUDA tensor [n, d] (cast to float32), ``2 <= n <= 8 192``, and labels of exactly two classes.  It
    sets ``classes_`` (``np.unique(y)``), ``booster_`` (a ``boosters.XGBTrees`` whose offset is the initial margin), ``trees_`` (the
    regressor's keys), ``base_score_`` (a probability), ``n_features_in_`` and ``train_margin_``.  ``decision_function`` returns float32
    margins, ``predict_proba`` float32 [m, 2] (``bbbp_xgbc_proba``), ``predict`` is ``classes_[p1 > 0.5]``: numpy for numpy queries, CUDA
    tensors for CUDA queries (``predict`` then returns the indices into ``classes_``' order as the labels when those are numbers, numpy
    otherwise).  ``get_model_json`` / ``save_model`` write XGBoost's JSON schema with the objective ``binary:logistic`` and ``base_score`` as the
    probability; ``from_model_json`` reads it back.  The module docstring states the algorithm, the draws and everything that is refused."""

    def __init__(self, n_estimators=100, max_depth=6, learning_rate=0.3, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, max_bin=256, base_score=None,
                 subsample=1.0, colsample_bytree=1.0, tree_method="hist", random_state=None, n_jobs=None, device="cuda", **other):
        given = dict(learning_rate=learning_rate, gamma=gamma, reg_lambda=reg_lambda)
        for alias, name in _ALIASES.items():
            if alias in other:
                given[name] = other.pop(alias)
        _refuse(other, _CLASSIFIER_NEUTRAL, _CLASSIFIER_IGNORED, _CWHO)
        # None is XGBoost's "use the default" for these two
        subsample, colsample_bytree = (1.0 if subsample is None else subsample), (1.0 if colsample_bytree is None else colsample_bytree)
        params = dict(n_estimators=n_estimators, max_depth=max_depth, min_child_weight=min_child_weight, max_bin=max_bin, base_score=base_score,
                      subsample=subsample, colsample_bytree=colsample_bytree, tree_method=tree_method, random_state=random_state, n_jobs=n_jobs,
                      device=device, **given)
        _check_classifier_params(params)
        if isinstance(device, (list, tuple)):
            raise NotImplementedError(f"{_CWHO}: device={device!r}: more than one GPU is not supported")
        for name in _CLASSIFIER_PARAMS:                       # kept as they were given: sklearn.base.clone compares them by identity
            setattr(self, name, params[name])

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in _CLASSIFIER_PARAMS}

    def set_params(self, **params):
        params = {_ALIASES.get(k, k): v for k, v in params.items()}
        unknown = set(params) - set(_CLASSIFIER_PARAMS)
        if unknown:
            raise ValueError(f"{_CWHO}: unknown parameters {sorted(unknown)}")
        type(self)(**{**self.get_params(), **params})
        for name, value in params.items():
            setattr(self, name, value)
        return self

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, sample_weight=None, eval_set=None, **other):
        if sample_weight is not None:
            raise NotImplementedError(f"{_CWHO}: sample_weight is not supported")
        if eval_set is not None or other.get("early_stopping_rounds") is not None:
            raise NotImplementedError(f"{_CWHO}: eval_set and early stopping are not supported")
        if set(other) - {"early_stopping_rounds", "verbose"}:
            raise NotImplementedError(f"{_CWHO}: fit arguments {sorted(set(other) - {'early_stopping_rounds', 'verbose'})} are not supported")
        _fit_classifiers([self], [(X, y)])
        return self

    def _adopt(self, classes, trees, base_margin, base_score, n_features, train_margin=None):
        self.classes_, self.trees_, self.base_margin_, self.base_score_ = np.asarray(classes), trees, np.float32(base_margin), np.float32(base_score)
        self.n_features_in_, self.train_margin_ = int(n_features), train_margin
        self.booster_ = boosters.XGBTrees(trees["left"], trees["right"], trees["feature"], trees["cond"], trees["default_left"], trees["root"],
                                          int(n_features), float(base_margin), device=self.device)
        return self

    @classmethod
    def from_trees(cls, trees, base_score, n_features, classes=(0, 1), device="cuda", **params):
        """A classifier around fitted arrays (``trees_``' keys; ``parents`` is derived when absent) and the probability ``base_score``, whose
        logit is the initial margin, as XGBoost takes it from a model file: for prediction and the JSON export.  ``device="cpu"`` gives a
        model that exports and validates but cannot predict."""
        self = cls(device=device, **params)
        trees = {k: np.asarray(v) for k, v in trees.items()}
        if not 0 < float(base_score) < 1:
            raise ValueError(f"{_CWHO}: base_score must be a probability strictly inside (0, 1), got {base_score!r}")
        m0, p = _initial_margin(None, np.float32(base_score))
        return self._adopt(classes, trees if "parents" in trees else _with_parents(trees), m0, p, n_features)

    @classmethod
    def from_model_json(cls, doc, classes=(0, 1), device="cuda", **params):
        """A classifier from ``get_model_json``'s document (a string, bytes or the parsed dict): the same arrays, statistics included."""
        if isinstance(doc, (bytes, bytearray)):
            doc = doc.decode("utf-8")
        if isinstance(doc, str):
            doc = json.loads(doc)
        learner = doc["learner"]
        if learner.get("objective", {}).get("name") != "binary:logistic":
            raise ValueError(f"{_CWHO}: the document's objective is {learner.get('objective', {}).get('name')!r}, not 'binary:logistic'")
        left, right, feature, cond, dleft, root, n_features, base = boosters.XGBTrees.flatten(
            {"learner": {**learner, "objective": {"name": "reg:squarederror"}}})        # the tree arrays are read as the regressor's are
        stats = {k: np.concatenate([np.asarray(t[k], np.float32) for t in learner["gradient_booster"]["model"]["trees"]])
                 for k in ("base_weights", "loss_changes", "sum_hessian")}
        trees = dict(left=left.astype(np.int32), right=right.astype(np.int32), feature=feature.astype(np.int32), cond=cond.astype(np.float32),
                     default_left=dleft.astype(np.uint8), root=root.astype(np.int32), **stats)
        return cls.from_trees(trees, base, n_features, classes=classes, device=device, n_estimators=len(root) - 1, **params)

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _fitted(self):
        if not hasattr(self, "booster_"):
            raise RuntimeError(f"{_CWHO}: not fitted")
        return self.booster_

    def decision_function(self, X):
        """float32 [m]: the margins, the initial margin plus the trees' leaf values (``bbbp_gbt_predict``)."""
        out = self._fitted().predict_device(X)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict_proba(self, X):
        """float32 [m, 2]: ``(1 - p1, p1)`` with ``p1 = sigmoid32(margin)``."""
        out = _proba_of_margin(self._fitted().predict_device(X))
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict(self, X):
        """``classes_[p1 > 0.5]``: numpy for numpy queries; for a CUDA tensor a CUDA tensor of the labels when they are numbers."""
        p1 = _proba_of_margin(self._fitted().predict_device(X))[:, 1] > 0.5
        if isinstance(X, torch.Tensor) and self.classes_.dtype.kind in "biuf":
            return torch.from_numpy(self.classes_).to(p1.device)[p1.long()]
        return self.classes_[p1.cpu().numpy().astype(np.intp)]

    # ---- export -----------------------------------------------------------------------------------------------------
    def get_model_json(self):
        """The model in XGBoost's published JSON schema, as the regressor writes it, with the objective ``binary:logistic``, ``base_score``
        the probability ``base_score_`` and ``num_class`` "0".  That XGBoost itself loads it is UNPINNED (see the module docstring)."""
        self._fitted()
        doc = json.loads(XGBRegressor.get_model_json(self))
        doc["learner"]["objective"] = {"name": "binary:logistic", "reg_loss_param": {"scale_pos_weight": "1"}}
        return json.dumps(doc)

    def save_model(self, path):
        with open(path, "w") as f:
            f.write(self.get_model_json())


def _fit_classifiers(classifiers, problems):
    """Fit ``classifiers[i]`` on ``problems[i] = (X, y)`` or ``(X, y, rows)`` in one ``bbbp_xgbc_fit`` batch.  Problems over one matrix object
    share its upload, and a bin matrix too when their rows and ``max_bin`` are the same.  Cuts, classes, the initial margin and the draws
    (a row's position within the problem, a column's original index) are the problem's own: a fold fitted in a batch equals the fold
    fitted alone bit for bit."""
    devices = {str(_cuda_device(clf.device, _CWHO)) for clf in classifiers}
    if len(devices) != 1:
        raise NotImplementedError(f"{_CWHO}: the classifiers of one batch name the devices {sorted(devices)}: more than one GPU is not supported")
    dev = _cuda_device(classifiers[0].device, _CWHO)
    checked, uploads = [], {}
    for prob in problems:
        if len(prob) not in (2, 3):
            raise ValueError(f"{_CWHO}: a problem is (X, y) or (X, y, rows), got {len(prob)} items")
        X, y, rows = prob[0], prob[1], (prob[2] if len(prob) == 3 else None)
        n_all = X.shape[0] if hasattr(X, "shape") and len(X.shape) == 2 else None
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.ndim != 1 or n_all is None or (len(rows) and (rows.min() < 0 or rows.max() >= n_all)):
                raise ValueError(f"{_CWHO}: rows must be a 1-D array of row indices of X")
        n = len(rows) if rows is not None else n_all
        if n is not None and n > MAX_ROWS:
            raise NotImplementedError(f"{_CWHO}: n = {n} rows, more than {MAX_ROWS} are not supported (BBBP_XGB_FIT_MAX_N)")
        if n is not None and n < 2:
            raise ValueError(f"{_CWHO}: at least two rows are needed, got {n}")
        y_all = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
        if y_all.ndim == 2 and y_all.shape[1] == 1:
            y_all = y_all[:, 0]
        if y_all.ndim != 1 or (n_all is not None and len(y_all) != n_all):
            raise ValueError(f"{_CWHO}: y must hold one label per row of X, got shape {tuple(y_all.shape)} for {n_all} rows")
        if id(X) not in uploads:
            uploads[id(X)] = _Upload(X, _CWHO)
        if rows is None and len(uploads[id(X)].cols) > MAX_LIVE_FEATURES:
            raise NotImplementedError(f"{_CWHO}: {len(uploads[id(X)].cols)} live features, more than {MAX_LIVE_FEATURES} are not supported (BBBP_XGB_FIT_MAX_D)")
        checked.append((X, *_binary_labels(y_all if rows is None else y_all[rows], n), rows))
    with torch.cuda.device(dev):
        binned, fits = {}, []
        for clf, (X, classes, t, rows) in zip(classifiers, checked):
            up = uploads[id(X)].upload(dev)
            key = (id(X), None if rows is None else rows.tobytes(), int(clf.max_bin))
            if key not in binned:
                binned[key] = _Bins(up, rows, int(clf.max_bin), dev, _CWHO)
            fits.append(_ClassifierProblem(clf, binned[key], classes, t, up.d, dev))
        keep = _run_classifiers(fits, dev)
        for clf, fit in zip(classifiers, fits):
            clf._adopt(fit.classes, fit.trees(), fit.base_margin, fit.base_score, fit.n_features, fit.margin.cpu().numpy())
        del keep


def fit_classifiers(problems, **params):
    """``[XGBClassifier(**params).fit(X[rows], y[rows]) for X, y, rows in problems]`` with every problem in one batch (``(X, y)`` means all
    rows): five folds and the refit are one call.  Each classifier equals its single ``fit`` bit for bit."""
    problems = list(problems)
    if not problems:
        raise ValueError("xgb.fit_classifiers: no problems")
    classifiers = [XGBClassifier(**params) for _ in problems]
    _fit_classifiers(classifiers, problems)
    return classifiers


# ---- the reference's randomized search ------------------------------------------------------------------------------------------------------
_SEARCH_KEYS = ("n_estimators", "learning_rate", "max_depth", "subsample", "colsample_bytree", "reg_lambda", "gamma", "min_child_weight", "max_bin",
                "base_score")


def _prefix_margins(clf, Xq, lengths):
    """{T: float32 margins of ``clf``'s first T trees on the device rows ``Xq``}: the fold's test margins from tree prefixes.  A prefix is a
    model of its own (``boosters.XGBTrees`` over the first T trees), so each equals the margins of the shorter fit bit for bit."""
    t, out = clf.trees_, {}
    for T in lengths:
        hi = int(t["root"][T])
        short = boosters.XGBTrees(t["left"][:hi], t["right"][:hi], t["feature"][:hi], t["cond"][:hi], t["default_left"][:hi], t["root"][:T + 1],
                                  clf.n_features_in_, float(clf.base_margin_), device=clf.device)
        out[T] = short.predict_device(Xq)
    return out


def randomized_search_cv(X, y, param_distributions, n_iter=50, cv=5, scoring=("accuracy", "precision"), refit="accuracy", random_state=None, device="cuda",
                         **fixed):
    """The reference's ``RandomizedSearchCV(XGBClassifier(...), param_grid, n_iter=50, cv=StratifiedKFold(5), scoring={accuracy, precision},
    refit="accuracy")`` (Models/model_opt_20250130.py:533-561) over ``n_estimators``, ``learning_rate``, ``max_depth``, ``subsample``,
    ``colsample_bytree``, ``reg_lambda``, ``gamma`` and ``min_child_weight``; ``fixed`` holds the estimator's other parameters.

    The points are scikit-learn's ``ParameterSampler(param_distributions, n_iter, random_state=random_state)``, the folds
    ``StratifiedKFold(cv)`` without shuffling.  The draw for tree ``t`` does not depend on ``n_estimators``, so a model of T trees is the
    prefix of a longer one even with sampling: every fold fits one chain per distinct setting of everything but ``n_estimators`` to the
    longest length asked of it, all chains of all folds in one ``bbbp_xgbc_fit`` batch, and the shorter models are scored from tree
    prefixes of the fold's test margins.  Scores come through ``bbbp_amd.metrics`` with ``classes_[1]`` as the positive class (an
    undefined precision counts 0, scikit-learn's default).  Returns (best_params, {name: mean score per point}, the classifier refitted on
    all rows with best_params); the first maximum of ``refit`` wins."""
    from sklearn.model_selection import ParameterSampler, StratifiedKFold
    from . import metrics
    who = "xgb.randomized_search_cv"
    score_keys = {"accuracy": "Accuracy", "precision": "Precision", "recall": "Recall", "f1": "F1 Score"}
    scoring = (scoring,) if isinstance(scoring, str) else tuple(scoring)
    unknown = [s for s in scoring if s not in score_keys]
    if unknown or not scoring:
        raise NotImplementedError(f"{who}: scoring {unknown!r} is not supported (only {sorted(score_keys)})")
    if refit not in scoring:
        raise ValueError(f"{who}: refit={refit!r} is not one of the scores {scoring!r}")
    dev = _cuda_device(device, who)
    strangers = set(param_distributions) - set(_SEARCH_KEYS)
    if strangers:
        raise NotImplementedError(f"{who}: the parameters {sorted(strangers)} cannot be searched (only {list(_SEARCH_KEYS)})")
    points = list(ParameterSampler(param_distributions, n_iter=n_iter, random_state=random_state))
    models = [XGBClassifier(**{**fixed, **pt, "device": dev}) for pt in points]            # every point is checked before anything is fitted
    X = np.asarray(X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else X)
    y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
    classes, _ = _binary_labels(y, X.shape[0] if X.ndim == 2 else None, who)
    folds = list(StratifiedKFold(n_splits=cv).split(np.zeros((len(y), 1)), y))
    rest_of = lambda m: tuple((k, v) for k, v in m.get_params().items() if k not in ("n_estimators", "device"))  # noqa: E731
    longest = {}
    for m in models:
        longest[rest_of(m)] = max(longest.get(rest_of(m), 0), int(m.n_estimators))
    chains, problems = {}, []
    for fi, (tr, _) in enumerate(folds):
        for rest, T in longest.items():
            chains[(fi, rest)] = XGBClassifier(n_estimators=T, device=dev, **dict(rest))
            problems.append((X, y, tr))
    _fit_classifiers(list(chains.values()), problems)
    table = {s: np.zeros((len(points), len(folds))) for s in scoring}
    with torch.cuda.device(dev):
        for fi, (_, te) in enumerate(folds):
            Xq = torch.from_numpy(np.ascontiguousarray(X[te], dtype=np.float32)).to(dev)
            for rest in longest:
                chain = chains[(fi, rest)]
                members = [pi for pi, m in enumerate(models) if rest_of(m) == rest]
                margins = _prefix_margins(chain, Xq, sorted({int(models[pi].n_estimators) for pi in members}))
                preds = np.stack([chain.classes_[(_proba_of_margin(margins[int(models[pi].n_estimators)])[:, 1] > 0.5).cpu().numpy().astype(np.intp)]
                                  for pi in members])
                got = metrics.classification_scores(y[te], preds, pos_label=classes[1], zero_division=0, device=dev)
                for s in scoring:
                    table[s][members, fi] = got[score_keys[s]][:, 0]
    means = {s: [float(v) for v in table[s].mean(axis=1)] for s in scoring}
    best = int(np.argmax(means[refit]))
    fitted = XGBClassifier(**{**fixed, **points[best], "device": dev}).fit(X, y)
    return points[best], means, fitted
