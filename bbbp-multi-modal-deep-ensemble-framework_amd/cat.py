"""``catboost.CatBoostRegressor`` for the GPU: boosted oblivious (symmetric) trees for RMSE, fitted by ``csrc/cat.hip``.

Every logBB script of the reference stacks ``CatBoostRegressor(iterations=300, learning_rate=0.01, depth=10, verbose=0, random_state=42)``
on ``hstack([fingerprints, images])`` (``Models/multi_input_data_regression_opt_transformer_cnn_20250108.py:192-195``): about 1 058 rows,
49 319 columns, and once more on the [N, 4] out-of-fold matrix inside ``StackingRegressor``.  The fitted model is a
``boosters.CatBoostTrees``: ``bbbp_oblivious_predict``, ``ensemble.screen(boosters=...)`` and ``ensemble.StackingRegressor`` take it as it is.

PARITY UNPINNED: the catboost package is installed neither where this is built nor where it runs, and the reference ships no fitted
CatBoost model.  Fits and the loading of ``get_model_json`` by CatBoost itself have never been compared with the package, only with the
numpy restatement (``tests/cat_numpy.py``), which the GPU fit equals bit for bit: alone, in any batch and from run to run.

THE DEVIATIONS from the package, by name:

1. *The deterministic form only.*  This class is ``boosting_type="Plain"``, ``bootstrap_type="No"``, ``random_strength=0``; those may be
   passed with these values or ``None``.  The package's own defaults (``bootstrap_type="MVS"``, ``random_strength=1``) and everything else
   that is not built are refused by name with ``ValueError``: losses other than ``RMSE``, ``boosting_type="Ordered"``, any bootstrap or
   ``subsample``, ``rsm`` below 1, ``grow_policy`` other than ``SymmetricTree``, ``min_data_in_leaf != 1``, ``leaf_estimation_iterations !=
   1``, ``score_function`` other than ``None`` / ``"Cosine"``, categorical or text features, ``sample_weight``, ``eval_set`` / early stopping,
   NaN or infinity in ``X`` or ``y``, ``depth`` outside 1..16, more than 8 192 rows, more than 65 536 live features, more than 10 000 trees,
   more than one GPU.  The seed is accepted and has no effect: nothing is random.  There is no CPU path.
2. *Borders.*  ``xgb.cut_matrix`` with ``max_bin = border_count + 1``: a column of at most ``max_bin`` distinct values gets every distinct
   value above its minimum as a cut, other columns get evenly spaced order statistics -- not CatBoost's ``GreedyLogSum``.
3. *The gradient grid.*  A gradient is rounded once to a per-tree grid (below), so that sums are exact integers.
4. *The score* is ``num^2 / den``, which orders candidates as CatBoost's Cosine ``num / sqrt(den)`` does, without a square root.
5. *learning_rate=None* means CatBoost's documented 0.03; the package picks a value from the data.

The algorithm -- CatBoost's Plain boosting of symmetric trees for RMSE, made deterministic so that no sum has an order:

*Quantisation.*  Features are float32; ``1 <= border_count <= 255`` (default 254), so a bin is one byte (``xgb._Upload``, ``xgb._Bins``,
``bbbp_xgb_bin``).  ``bin(x)`` is the number of the column's cuts ``<= x``.  Columns without a cut are constant and are dropped before the
upload; reported indices are the original ones.  If no column has a cut, ``fit`` raises ``ValueError`` ("all features are constant").

*Border rule.*  Candidate ``(f, c)`` sends a row right iff ``bin(x_f) > c``, that is ``x_f >= cut_c``.  The predict kernel tests ``x >
border`` in float32: with ``a`` the largest value of the training column below ``cut_c``, ``border = float32(0.5 ((double)a +
(double)cut_c))``, and ``border = a`` if that is ``>= cut_c`` (adjacent floats).  Then ``x > border`` iff ``bin(x) > c`` for every value
of the training column.

*State.*  ``bias = np.mean(y)`` in float64, formed on the host (``boost_from_average``).  Per row ``s_i`` is the float64 sum of the leaf
values so far, from 0.0, added in tree order; the approximation is ``a_i = s_i + bias``, one rounding: the order of ``obl_sum_kernel``,
so ``predict(X_train)`` equals ``train_approx_`` bit for bit.

*Gradients per tree.*  ``g_i = y_i - a_i`` in float64, ``gmax = max |g_i|``, ``k = 47 - ilogb(gmax)`` (``k = 0`` when ``gmax == 0``) and
``q_i = llrint(ldexp(g_i, k))``.  With ``n <= 8 192`` a part's ``Q = sum q_i`` is an exact 64-bit integer in any order; ``S =
ldexp((double)Q, -k)``; ``m`` is the part's row count.

*Levels.*  A tree has ``depth`` levels; level l has up to ``2^l`` parts.  The row list is partitioned in place and stably: a part's left
rows (``bin <= c``) come first, then its right rows, so parts stand in the order of the leaf index read with level 0 as the most
significant bit.  That is the summation order.

*Score of a candidate*, float64, every operation rounded on its own (``-ffp-contract=off``): ``num = den = 0``; over the parts in that
order, in a part left then right, a side with ``m_s == 0`` is skipped, otherwise ``alpha = S_s / (m_s + lambda)``, ``num += alpha S_s``,
``den += (alpha alpha) m_s``; ``score = den > 0 ? (num num) / den : 0``; ``lambda = l2_leaf_reg``.

*Choosing the split.*  The level's split is the unused candidate of highest score; among equal scores the lowest original feature index
wins, then the lowest cut.  A ``(feature, cut)`` pair already used in this tree is no candidate.  There is no minimum gain: the tree takes
its ``depth`` levels, and is shallower only when no unused candidate is left.

*Leaves.*  Leaf j (CatBoost's convention: bit i is the outcome of split i) has the value ``learning_rate (S_j / (m_j + lambda))``, two
roundings; an empty leaf has 0.0.  Then ``s_i += v[leaf(i)]``; ``leaf_weights`` records ``m_j``.

*Model.*  A ``boosters.CatBoostTrees`` with ``scale = 1``, ``bias``, no NaN treatment, float32 borders and float64 leaf values.
"""
from __future__ import annotations

import json
import numbers

import numpy as np
import torch

from . import _dense, _estimator, _lib, _tree_host, boosters, xgb
from ._tree_host import is_int as _is_int

MAX_ROWS, MAX_LIVE_FEATURES, MAX_DEPTH, MAX_TREES = 8192, 65536, 16, 10000          # BBBP_CAT_FIT_MAX_*
DEFAULT_LEARNING_RATE = 0.03
_WHO = "CatBoostRegressor"
_ALIASES = {"random_state": "random_seed", "n_estimators": "iterations", "max_depth": "depth", "reg_lambda": "l2_leaf_reg"}
_DEFAULTS = dict(iterations=1000, depth=6, l2_leaf_reg=3.0, random_seed=None)
# CatBoost's further parameters pass with None or a value that leaves the algorithm of the module docstring unchanged; anything else is
# refused by name
_NEUTRAL = dict(loss_function=("RMSE",), objective=("RMSE",), eval_metric=("RMSE",), boosting_type=("Plain",), bootstrap_type=("No",),
                random_strength=(0,), subsample=(), bagging_temperature=(), sampling_frequency=(), sampling_unit=(), mvs_reg=(), rsm=(1,),
                colsample_bylevel=(1,), grow_policy=("SymmetricTree",), min_data_in_leaf=(1,), min_child_samples=(1,), max_leaves=(),
                leaf_estimation_iterations=(1,), leaf_estimation_method=("Newton", "Gradient"), leaf_estimation_backtracking=("No",),
                score_function=("Cosine",), cat_features=(), text_features=(), embedding_features=(), one_hot_max_size=(), early_stopping_rounds=(),
                od_type=(), od_wait=(), od_pval=(), use_best_model=(False,), boost_from_average=(True,), nan_mode=("Forbidden",),
                feature_border_type=(), monotone_constraints=(), feature_weights=(), penalties_coefficient=(), langevin=(False,),
                diffusion_temperature=(), posterior_sampling=(False,), model_shrink_rate=(0,), model_shrink_mode=(), has_time=(False,),
                fold_permutation_block=(), approx_on_full_history=(), devices=())
_IGNORED = ("thread_count", "logging_level", "silent", "metric_period", "allow_writing_files", "train_dir", "name", "save_snapshot", "snapshot_file",
            "snapshot_interval", "used_ram_limit", "gpu_ram_part", "task_type", "custom_metric", "model_size_reg")


def _same(value, ok):
    if isinstance(ok, bool) or isinstance(value, (bool, np.bool_)):
        return isinstance(ok, bool) and bool(value) is ok
    if isinstance(ok, numbers.Real):
        return isinstance(value, numbers.Real) and value == ok
    return isinstance(value, str) and value == ok


def _refuse(other, who=_WHO):
    for name, value in other.items():
        if name in _IGNORED:
            continue
        if name not in _NEUTRAL:
            raise ValueError(f"{who}: unknown parameter {name}")
        if value is None or any(_same(value, ok) for ok in _NEUTRAL[name]):
            continue
        only = " or ".join(repr(ok) for ok in _NEUTRAL[name] + (None,))
        raise ValueError(f"{who}: {name}={value!r} is not supported (only {only}): this class is the deterministic Plain form")


def _check_params(iterations, learning_rate, depth, l2_leaf_reg, border_count, random_seed, who=_WHO):
    if not _is_int(iterations) or iterations < 1:
        raise ValueError(f"{who}: iterations must be an int >= 1, got {iterations!r}")
    if iterations > MAX_TREES:
        raise ValueError(f"{who}: iterations = {iterations}: more than {MAX_TREES} trees are not supported (BBBP_CAT_FIT_MAX_TREES)")
    if not _is_int(depth) or not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"{who}: depth must be an int in 1..{MAX_DEPTH}, got {depth!r}")
    if (iterations << depth) >= 2 ** 31:
        raise ValueError(f"{who}: {iterations} trees of {1 << depth} leaves exceed 32-bit leaf indices")
    if learning_rate is not None:
        xgb._number(learning_rate, "learning_rate", 0.0, lo_open=True, who=who)
    xgb._number(l2_leaf_reg, "l2_leaf_reg", 0.0, who=who)
    if not _is_int(border_count) or not 1 <= border_count <= 255:
        raise ValueError(f"{who}: border_count must be an int in 1..255 (a bin is one byte), got {border_count!r}")
    if random_seed is not None and not _is_int(random_seed):
        raise ValueError(f"{who}: random_seed must be None or an int, got {random_seed!r}")


def _cuda_device(device, who=_WHO):
    if isinstance(device, (list, tuple)):
        raise ValueError(f"{who}: device={device!r}: more than one GPU is not supported")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: device {device!r}: trees are fitted on the GPU (no CPU path)")
    return dev


def borders_of(XT, cuts):
    """float32 [U]: the border of every pair (training column ``XT[u]`` [U, n], its cut ``cuts[u]``) by the module docstring's rule.  Plain
    torch on the columns' device: a maximum is plumbing."""
    neg = torch.tensor(float("-inf"), dtype=torch.float32, device=XT.device)
    a = torch.where(XT < cuts[:, None], XT, neg).max(dim=1).values + 0.0
    mid = (0.5 * (a.double() + cuts.double())).float()
    return torch.where(mid >= cuts, a, mid)


class _Problem:
    """One model to fit: its outputs, its work area and the descriptor ``bbbp_cat_fit`` takes.  Nothing needs initialising."""

    def __init__(self, reg, up, rows, bins, n_cuts, y, dev):
        L = _lib.lib()
        n, d, T, D = bins.n, bins.d, int(reg.iterations), int(reg.depth)
        nbytes = L.bbbp_cat_fit_work_bytes(n, d, D)
        if not nbytes:
            raise ValueError("cat: " + L.bbbp_last_error().decode("utf-8", "replace"))
        self.up, self.rows, self.bins, self.n_cuts, self.T, self.D = up, rows, bins, n_cuts, T, D
        self.bias = float(np.mean(y))
        self.learning_rate = DEFAULT_LEARNING_RATE if reg.learning_rate is None else float(reg.learning_rate)
        self.y = torch.from_numpy(np.ascontiguousarray(y, np.float64)).to(dev)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.split_feature = torch.empty(T * D, dtype=torch.int32, device=dev)
        self.split_bin = torch.empty(T * D, dtype=torch.int32, device=dev)
        self.leaf_values = torch.empty(T << D, dtype=torch.float64, device=dev)
        self.leaf_weights = torch.empty(T << D, dtype=torch.int32, device=dev)
        self.tree_depth = torch.empty(T, dtype=torch.int32, device=dev)
        self.approx = torch.empty(n, dtype=torch.float64, device=dev)
        self.desc = _lib.CatProblem(bins.bins.data_ptr(), n_cuts.data_ptr(), self.y.data_ptr(), n, d, T, D, float(reg.l2_leaf_reg), self.learning_rate,
                                    self.bias, self.work.data_ptr(), self.split_feature.data_ptr(), self.split_bin.data_ptr(),
                                    self.leaf_values.data_ptr(), self.leaf_weights.data_ptr(), self.tree_depth.data_ptr(), self.approx.data_ptr())

    def trees(self, dev):
        """The fitted trees as flat host arrays in ``boosters.CatBoostTrees``' convention, with ``split_bin`` and ``leaf_weights``."""
        T, D = self.T, self.D
        levels = self.tree_depth.cpu().numpy().astype(np.int64)
        if (levels < 0).any() or (levels > D).any():
            raise RuntimeError(f"cat: the fit kernels reported an index outside its array in tree {int(np.argmax((levels < 0) | (levels > D)))} "
                               "(a defect of csrc/cat.hip, not of the data); no model is returned")
        keep_split = (np.arange(D)[None, :] < levels[:, None]).ravel()
        keep_leaf = (np.arange(1 << D)[None, :] < (1 << levels)[:, None]).ravel()
        f_live = self.split_feature.cpu().numpy()[keep_split].astype(np.int64)
        c = self.split_bin.cpu().numpy()[keep_split].astype(np.int64)
        if len(f_live) and (f_live.min() < 0 or f_live.max() >= self.bins.d or c.min() < 0 or c.max() >= self.bins.cuts.shape[1]):
            raise RuntimeError("cat: the fit kernels recorded a split outside the bin matrix (a defect of csrc/cat.hip); no model is returned")
        # the borders of the pairs the model uses, from the problem's own training columns
        pairs, inverse = np.unique(f_live * 256 + c, return_inverse=True)
        uf, uc = torch.from_numpy(pairs // 256).to(dev), torch.from_numpy(pairs % 256).to(dev)
        at = torch.from_numpy(np.searchsorted(self.up.cols, self.bins.cols[pairs // 256])).to(dev)
        XT = self.up.XT[at]
        if self.rows is not None:
            XT = XT[:, torch.from_numpy(self.rows).to(dev)]
        border = borders_of(XT, self.bins.cuts[uf, uc]).cpu().numpy()[inverse.ravel()]
        first_leaf = np.concatenate([[0], np.cumsum(1 << levels)])
        return dict(split_feature=self.bins.cols[f_live].astype(np.int32), split_border=border.astype(np.float32), split_bin=c.astype(np.int32),
                    tree_first_split=np.concatenate([[0], np.cumsum(levels)]).astype(np.int32), tree_first_leaf=first_leaf[:-1].astype(np.int64),
                    leaf_values=self.leaf_values.cpu().numpy()[keep_leaf], leaf_weights=self.leaf_weights.cpu().numpy()[keep_leaf])


def _run(problems, dev):
    arr = (_lib.CatProblem * len(problems))(*[p.desc for p in problems])
    on_device = _tree_host.upload(arr, dev)
    _lib.check(_lib.lib().bbbp_cat_fit(_dense.stream(), arr, on_device.data_ptr(), len(problems)), "bbbp_cat_fit")
    return on_device                                  # the fit has synchronised the stream; kept alive by the caller all the same


class CatBoostRegressor(_estimator.Params):
    """``CatBoostRegressor(iterations=1000, learning_rate=None, depth=6, l2_leaf_reg=3.0, border_count=254, random_seed=None, verbose=None,
    device="cuda")``: CatBoost's names; ``random_state``, ``n_estimators``, ``max_depth`` and ``reg_lambda`` are aliases of ``random_seed``,
    ``iterations``, ``depth`` and ``l2_leaf_reg``.  ``learning_rate=None`` is 0.03; the seed and ``verbose`` are accepted and unused (nothing
    is random).  The reference's ``CatBoostRegressor(iterations=300, learning_rate=0.01, depth=10, verbose=0, random_state=42)`` builds as
    written.  The class is CatBoost's deterministic Plain form; everything else is refused by name with ``ValueError`` (the module docstring
    lists it, with the algorithm, the deviations and the unpinned parity with the catboost package).

    ``fit(X, y)`` takes a numpy array or a CUDA tensor [n, d], float32 or float64 (cast to float32; a row-strided view in place),
    ``2 <= n <= 8 192``, and finite targets.  It sets ``model_`` (a ``boosters.CatBoostTrees``; ``predict`` is its ``predict``), ``trees_``
    (the flat host arrays ``split_feature``, ``split_border``, ``split_bin``, ``tree_first_split``, ``tree_first_leaf``, ``leaf_values``,
    ``leaf_weights``), ``bias_``, ``tree_count_``, ``n_features_in_`` and ``train_approx_`` (float64: the training rows' approximations as the
    fit summed them; ``predict(X_train)`` equals it bit for bit).  ``get_model_json`` / ``save_model`` write CatBoost's JSON export schema.
    ``get_params`` / ``set_params`` make ``sklearn.base.clone`` and ``ensemble.StackingRegressor`` work."""

    _params = ("iterations", "learning_rate", "depth", "l2_leaf_reg", "border_count", "random_seed", "verbose", "device")

    def __init__(self, iterations=1000, learning_rate=None, depth=6, l2_leaf_reg=3.0, border_count=254, random_seed=None, verbose=None, device="cuda",
                 **other):
        given = dict(iterations=iterations, depth=depth, l2_leaf_reg=l2_leaf_reg, random_seed=random_seed)
        for alias, name in _ALIASES.items():
            if alias in other:
                value = other.pop(alias)
                if given[name] is not _DEFAULTS[name] and given[name] != _DEFAULTS[name]:
                    raise ValueError(f"{_WHO}: {alias} is an alias of {name}: only one of them may be given")
                given[name] = value
        _refuse(other)
        border_count = 254 if border_count is None else border_count
        _check_params(given["iterations"], learning_rate, given["depth"], given["l2_leaf_reg"], border_count, given["random_seed"])
        if isinstance(device, (list, tuple)):
            raise ValueError(f"{_WHO}: device={device!r}: more than one GPU is not supported")
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.iterations, self.depth, self.l2_leaf_reg, self.random_seed = given["iterations"], given["depth"], given["l2_leaf_reg"], given["random_seed"]
        self.learning_rate, self.border_count, self.verbose, self.device = learning_rate, border_count, verbose, device

    def set_params(self, **params):
        return super().set_params(**{_ALIASES.get(k, k): v for k, v in params.items()})

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, cat_features=None, text_features=None, embedding_features=None, sample_weight=None, eval_set=None, early_stopping_rounds=None,
            use_best_model=None, **other):
        if cat_features is not None or text_features is not None or embedding_features is not None:
            raise ValueError(f"{_WHO}: categorical, text and embedding features are not supported (float features only)")
        if sample_weight is not None:
            raise ValueError(f"{_WHO}: sample_weight is not supported")
        if eval_set is not None or early_stopping_rounds is not None or use_best_model:
            raise ValueError(f"{_WHO}: eval_set and early stopping are not supported")
        rest = set(other) - {"verbose", "verbose_eval", "silent", "logging_level", "plot", "metric_period"}
        if rest:
            raise ValueError(f"{_WHO}: fit arguments {sorted(rest)} are not supported")
        _fit([self], [(X, y)])
        return self

    def _adopt(self, trees, bias, n_features, train_approx=None):
        self.trees_, self.bias_, self.n_features_in_, self.train_approx_ = trees, float(bias), int(n_features), train_approx
        self.tree_count_ = len(trees["tree_first_split"]) - 1
        self.model_ = boosters.CatBoostTrees(trees["split_feature"], trees["split_border"], np.zeros(int(n_features), np.uint8), trees["tree_first_split"],
                                             trees["tree_first_leaf"], trees["leaf_values"], int(n_features), 1.0, float(bias), device=self.device)
        return self

    @classmethod
    def from_trees(cls, trees, bias, n_features, device="cuda", **params):
        """A regressor around fitted arrays (``trees_``' keys): for prediction and the JSON export.  ``device="cpu"`` gives a model that
        exports and validates but cannot predict."""
        self = cls(device=device, **params)
        return self._adopt({k: np.asarray(v) for k, v in trees.items()}, bias, n_features)

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _fitted(self):
        if not hasattr(self, "model_"):
            raise RuntimeError(f"{_WHO}: not fitted")
        return self.model_

    def predict(self, X):
        """float64 [m]: ``bias_`` behind the sum of the trees' leaf values (``bbbp_oblivious_predict``); numpy for numpy queries, a CUDA
        tensor for a CUDA tensor."""
        out = self._fitted().predict_device(X)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict_device(self, X):
        return self._fitted().predict_device(X)

    # ---- export -----------------------------------------------------------------------------------------------------
    def get_model_json(self):
        """The model as a JSON document in the schema of CatBoost's ``save_model(format="json")``: ``oblivious_trees`` with ``splits``
        (``float_feature_index``, ``border``, ``split_type``), ``leaf_values`` and ``leaf_weights``, ``features_info.float_features`` and
        ``scale_and_bias``; ``boosters.CatBoostTrees.from_json`` reads it back to the same arrays.  That CatBoost itself loads it is
        UNPINNED: the package is absent (see the module docstring)."""
        self._fitted()
        t = self.trees_
        fs, fl = t["tree_first_split"].astype(np.int64), np.concatenate([t["tree_first_leaf"], [len(t["leaf_values"])]]).astype(np.int64)
        used = {}                                         # feature -> its borders in use, ascending
        for f, b in zip(t["split_feature"], t["split_border"]):
            used.setdefault(int(f), set()).add(float(b))
        used = {f: sorted(b) for f, b in used.items()}
        first_index, acc = {}, 0                          # split_index: the position in the features' borders laid end to end
        for f in sorted(used):
            first_index[f] = acc
            acc += len(used[f])
        trees = []
        for i in range(self.tree_count_):
            splits = [{"float_feature_index": int(f), "border": float(b), "split_type": "FloatFeature",
                       "split_index": first_index[int(f)] + used[int(f)].index(float(b))}
                      for f, b in zip(t["split_feature"][fs[i]:fs[i + 1]], t["split_border"][fs[i]:fs[i + 1]])]
            trees.append({"splits": splits, "leaf_values": [float(x) for x in t["leaf_values"][fl[i]:fl[i + 1]]],
                          "leaf_weights": [int(x) for x in t["leaf_weights"][fl[i]:fl[i + 1]]]})
        feats = [{"feature_index": f, "flat_feature_index": f, "has_nans": False, "nan_value_treatment": "AsIs", "borders": used.get(f, [])}
                 for f in range(self.n_features_in_)]
        lr = DEFAULT_LEARNING_RATE if self.learning_rate is None else float(self.learning_rate)
        doc = {"features_info": {"float_features": feats},
               "model_info": {"params": {"boosting_options": {"boosting_type": "Plain", "iterations": int(self.iterations), "learning_rate": lr},
                                         "loss_function": {"type": "RMSE"},
                                         "tree_learner_options": {"depth": int(self.depth), "l2_leaf_reg": float(self.l2_leaf_reg)}}},
               "oblivious_trees": trees, "scale_and_bias": [1.0, [float(self.bias_)]]}
        return json.dumps(doc)

    def save_model(self, path, format="json"):
        if format != "json":
            raise ValueError(f"{_WHO}: save_model writes format='json' only, got {format!r}")
        with open(path, "w") as f:
            f.write(self.get_model_json())


def _fit(regressors, problems):
    """Fit ``regressors[i]`` on ``problems[i] = (X, y)`` or ``(X, y, rows)`` in one ``bbbp_cat_fit`` batch.  Problems over one matrix object
    share its upload; they share a bin matrix too when their rows and ``border_count`` are the same.  Cuts are per problem, from the
    problem's own rows: a fold fitted in a batch equals the fold fitted alone."""
    devices = {str(_cuda_device(reg.device)) for reg in regressors}
    if len(devices) != 1:
        raise ValueError(f"{_WHO}: the regressors of one batch name the devices {sorted(devices)}: more than one GPU is not supported")
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
            raise ValueError(f"{_WHO}: n = {n} rows, more than {MAX_ROWS} are not supported (BBBP_CAT_FIT_MAX_N)")
        if n is not None and n < 2:
            raise ValueError(f"{_WHO}: at least two rows are needed, got {n}")
        try:
            y_all = _tree_host.targets_1d(y, n_all, _WHO, "more than one output column is not supported")
        except NotImplementedError as e:
            raise ValueError(str(e)) from None
        if id(X) not in uploads:
            uploads[id(X)] = xgb._Upload(X, who=_WHO)
        up = uploads[id(X)]
        if len(up.cols) == 0:
            raise ValueError(f"{_WHO}: all features are constant")
        if rows is None and len(up.cols) > MAX_LIVE_FEATURES:
            raise ValueError(f"{_WHO}: {len(up.cols)} live features, more than {MAX_LIVE_FEATURES} are not supported (BBBP_CAT_FIT_MAX_D)")
        checked.append((X, y_all if rows is None else y_all[rows], rows))
    with torch.cuda.device(dev):
        binned, fits = {}, []
        for reg, (X, y, rows) in zip(regressors, checked):
            up = uploads[id(X)].upload(dev)
            key = (id(X), None if rows is None else rows.tobytes(), int(reg.border_count))
            if key not in binned:
                try:
                    bins = xgb._Bins(up, rows, int(reg.border_count) + 1, dev, who=_WHO)
                except NotImplementedError as e:
                    raise ValueError(str(e)) from None
                n_cuts = torch.isfinite(bins.cuts).sum(dim=1).to(torch.int32).contiguous()
                if int(n_cuts.min()) < 1:                 # xgb._Bins' dead feature: no column of these rows has a cut
                    raise ValueError(f"{_WHO}: all features are constant")
                binned[key] = (bins, n_cuts)
            fits.append(_Problem(reg, up, rows, *binned[key], y, dev))
        keep = _run(fits, dev)
        for reg, fit in zip(regressors, fits):
            reg._adopt(fit.trees(dev), fit.bias, fit.up.d, fit.approx.cpu().numpy())
        del keep


def fit_regressors(problems, **params):
    """``[CatBoostRegressor(**params).fit(X[rows], y[rows]) for X, y, rows in problems]`` with every problem in one batch (``(X, y)`` means all
    rows): the reference's five folds and the refit are one call.  Each regressor equals its single ``fit`` bit for bit."""
    problems = list(problems)
    if not problems:
        raise ValueError("cat.fit_regressors: no problems")
    regressors = [CatBoostRegressor(**params) for _ in problems]
    _fit(regressors, problems)
    return regressors
