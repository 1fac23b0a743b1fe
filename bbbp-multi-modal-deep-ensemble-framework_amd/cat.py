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

*Curves, the best iteration and ``use_best_model``, after the fit.*  ``eval_set`` / ``use_best_model`` stay refused inside ``fit``: the fit is
deterministic and no validation row influences a tree, so the reference's ``fit(X, y, eval_set=(X_test, y_test), use_best_model=True)``
(``Models/multi_input_data_regression_opt_transformer_cnn_20250113.py:337-369``) is ``fit(X, y)``, ``eval_curves((X_test, y_test),
learn=(X, y))`` -- which sets ``evals_result_`` (``{"learn": {"RMSE": [...]}, "validation": {"RMSE": [...]}}``) and ``best_iteration_`` -- and
``shrink(get_best_iteration() + 1)``.  ``staged_predict``, ``eval_metrics`` and ``predict(X, ntree_start, ntree_end)`` carry CatBoost's
names; all of them come from one walk of the trees (``boosters.CatBoostTrees.staged_predict_device``), a curve from one
``metrics.squared_error_sums`` launch for all its stages.  No training stops early: a fit of T trees is a prefix of a longer one, so
cutting the full fit gives the same model.  RMSE only.  Unpinned: CatBoost's stage convention for ``eval_period > 1`` and which eval set
it takes the best iteration from (``best_on``, the last by default).


``catboost.CatBoostClassifier`` for two classes under Logloss, fitted by ``csrc/catc.hip``
==========================================================================================

Every classification script of the reference ends in a table of ten learners, one of them ``CatBoostClassifier(iterations=500,
learning_rate=0.03, depth=10, l2_leaf_reg=5, bagging_temperature=0.5, loss_function="Logloss", verbose=0, random_seed=42)``
(``Models/model_opt_20250130.py:413-457``), searched with ``RandomizedSearchCV`` over ``iterations``, ``learning_rate``, ``depth``,
``l2_leaf_reg`` and ``border_count`` (``:547-561``) and a member of the stack's soft ``VotingClassifier`` (``:596-642``).

PARITY UNPINNED, as for the regressor: the catboost package is absent where this is built and where it runs.  Fits and the loading of
``get_model_json`` by CatBoost itself have never been compared with the package, only with the numpy restatement
(``tests/catc_numpy.py``), which the GPU fit equals bit for bit: alone, in any batch and from run to run.

THE DEVIATIONS from the package: the regressor's five stand (the deterministic form, the borders, the gradient grid -- here ``2^-28`` of
``gmax`` --, the score ``num^2 / den``, ``learning_rate=None`` meaning 0.03), and

6. *bootstrap_type=None* means ``"Bayesian"`` with the given temperature when ``bagging_temperature`` is given, otherwise ``"No"``.
   ``bootstrap_type="Bayesian"`` with ``bagging_temperature=None`` means temperature 1.0.  The package's default is ``"MVS"`` for this loss.
7. *The weights* are drawn per tree from our hash (``xgb.sample_hash``), in fixed point, not from the package's generator; and
   ``bagging_temperature`` must lie in [0, 1].
8. *random_strength=None* means 0; the package's default is 1.
9. *leaf_estimation_iterations* must be ``None`` or 1, with method ``Newton``: one Newton step per leaf.  The package's default count for
   Logloss is believed to be larger; that could not be checked, the package being absent.
10. *The bias rule* below (``boost_from_average``).

Refused by name with ``ValueError``: everything the regressor refuses, ``class_weights``, ``auto_class_weights``, ``scale_pos_weight``
other than 1, bootstrap types other than ``"No"`` / ``"Bayesian"`` (MVS, Bernoulli, Poisson), ``subsample``, ``bagging_temperature`` outside
[0, 1], ``random_strength > 0``, more than one leaf-estimation iteration, more or fewer than two classes (``MultiClass``), NaN.

The algorithm is the regressor's -- quantisation, border rule, levels, the choice of a split and the model are word for word the text
above -- with these differences:

*Labels and bias.*  Exactly two classes; ``classes_ = np.unique(y)`` may hold labels of any dtype and ``t_i`` in {0.0, 1.0} is the row's
index in ``classes_``.  With P rows of class 1 and N of class 0, ``boost_from_average=None`` or ``True`` gives ``bias = np.log(np.float64(P)
/ np.float64(N))``, formed on the host, and ``False`` gives ``bias = 0.0``.  A fit whose rows lack a class is refused with ``ValueError``.

*State.*  ``s_i`` and ``a_i = s_i + bias`` as in the regressor: float64, summed in tree order, the bias last, so
``predict(X_train, prediction_type="RawFormulaVal")`` equals ``train_approx_`` bit for bit.

*The sigmoid.*  ``p_i = sigmoid64(a_i)`` is ``csrc/xgbc.hip``'s ``sigmoid32`` without its final rounding to float32: ``a = max(-|z|,
-700.0)`` (the clamp keeps ``p`` a normal float64), ``k = rint(a / ln2)``, ``r = (a - k LN2_HI) - k LN2_LO``, the Taylor polynomial of degree
13 in ``r`` by Horner's rule in float64, ``e = ldexp(P, k)``, and ``1 / (1 + e)`` for ``z >= 0``, otherwise ``e / (1 + e)``.  IEEE operations
only, in a file compiled with ``-ffp-contract=off``: numpy gives the same bits.  Against x86 long double the numpy form is within 2.4 ulp
over +-700, monotone, finite and normal (``tests/test_catc_cpu.py`` asserts 4 ulp).

*Per tree.*  ``g_i = t_i - p_i`` and ``h_i = p_i (1 - p_i)`` in float64, each operation rounded on its own; ``gmax = max |g_i|``, ``k = 27 -
ilogb(gmax)`` (``k = 0`` when ``gmax == 0``), ``q_i = llrint(ldexp(g_i, k))``, so ``|q_i| <= 2^28``, and ``r_i = max(1, llrint(ldexp(h_i,
48)))``, so ``r_i <= 2^46``.

*Bootstrap weights.*  The Bayesian bootstrap, drawn once per tree, on the host (``log`` and ``pow`` are not IEEE-exact on the device).
With the stream tag 2 (``xgb`` holds 0 and 1): ``u = ((sample_hash(seed, 2, tree, i) >> 11) + 1) 2^-53`` in (0, 1], ``i`` the row's
position in the problem; ``w = np.power(-np.log(u), bagging_temperature)``; ``w_i = max(1, llrint(w 2^16))`` as uint32.  With the
temperature in [0, 1], ``w_i <= 2 407 583 < 2^22``.  One table ``[iterations, n]`` is built per (seed, temperature) and batch, uploaded
once and shared by the problems of the batch that use it, its row stride their largest ``n``.  ``random_seed=None`` means 0.
``bootstrap_type="No"`` passes no table and every ``w_i`` is ``2^16``; ``bagging_temperature=0`` gives a table of ``2^16`` (``0 ** 0 == 1``
in numpy): the two give the same model bit for bit.  The draw for tree ``t`` does not depend on ``iterations``: a model of T trees is
the prefix of a longer one.

*Structure search.*  The regressor's, with weighted gradients and weight sums for gradients and counts.  A row carries ``qw_i = q_i
w_i``, an exact int64 product, ``|qw_i| < 2^50``.  A part carries ``QW = sum qw_i``, ``MW = sum w_i`` and its row count; with ``n <= 8 192``,
``|QW| < 2^63`` and ``MW < 2^35``: exact integers in any order.  ``S = ldexp((double)QW, -(k + 16))`` and ``M = ldexp((double)MW, -16)``.  A
side of a part is empty iff it holds no row, which is ``MW == 0`` (``w_i >= 1``); an empty side is skipped, otherwise ``alpha = S / (M +
lambda)``, ``num += alpha S``, ``den += (alpha alpha) M``.  The order of the parts and sides, ``score = den > 0 ? (num num) / den : 0``, the
tie rule, no pair used twice in a tree and no minimum gain are the regressor's.

*Leaves.*  One Newton step over all rows of the leaf, unweighted (the bootstrap shapes the structure only): ``Qg = sum q_i`` and ``R = sum
r_i`` over the leaf's rows, exact integers (``R <= 2^59``); ``G = ldexp((double)Qg, -k)``, ``H = ldexp((double)R, -48)``, ``value =
learning_rate (G / (H + lambda))``; an empty leaf has 0.0; ``leaf_weights`` records the row count.

*Output.*  ``predict_proba`` is float64 ``(1 - p1, p1)`` with ``p1 = sigmoid64(raw)``, the subtraction in float64; the class is
``classes_[raw > 0]``.
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


def _refuse(other, who=_WHO, neutral=_NEUTRAL):
    for name, value in other.items():
        if name in _IGNORED:
            continue
        if name not in neutral:
            raise ValueError(f"{who}: unknown parameter {name}")
        if value is None or any(_same(value, ok) for ok in neutral[name]):
            continue
        only = " or ".join(repr(ok) for ok in neutral[name] + (None,))
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

    source = "csrc/cat.hip"

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
                               f"(a defect of {self.source}, not of the data); no model is returned")
        keep_split = (np.arange(D)[None, :] < levels[:, None]).ravel()
        keep_leaf = (np.arange(1 << D)[None, :] < (1 << levels)[:, None]).ravel()
        f_live = self.split_feature.cpu().numpy()[keep_split].astype(np.int64)
        c = self.split_bin.cpu().numpy()[keep_split].astype(np.int64)
        if len(f_live) and (f_live.min() < 0 or f_live.max() >= self.bins.d or c.min() < 0 or c.max() >= self.bins.cuts.shape[1]):
            raise RuntimeError(f"cat: the fit kernels recorded a split outside the bin matrix (a defect of {self.source}); no model is returned")
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

    def predict(self, X, ntree_start=0, ntree_end=0):
        """float64 [m]: ``bias_`` behind the sum of the trees' leaf values (``bbbp_oblivious_predict``); numpy for numpy queries, a CUDA
        tensor for a CUDA tensor.  ``ntree_start`` / ``ntree_end`` are CatBoost's: the trees ``[ntree_start, ntree_end)`` only, ``ntree_end
        = 0`` meaning all of them (one stage of ``bbbp_oblivious_staged_predict``)."""
        model = self._fitted()
        if _is_int(ntree_start) and _is_int(ntree_end) and ntree_start == 0 and ntree_end == 0:
            out = model.predict_device(X)
        else:
            out = model.staged_predict_device(X, ntree_start, ntree_end, period=model.n_trees)[0]
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict_device(self, X):
        return self._fitted().predict_device(X)

    def staged_predict(self, X, ntree_start=0, ntree_end=0, eval_period=1):
        """float64 ``[K, m]``: row ``k`` is the prediction of the trees ``[ntree_start, min(ntree_start + (k + 1) eval_period, ntree_end))``,
        all from one walk of the trees (``boosters.CatBoostTrees.staged_predict_device``); iterating over the result gives one stage per
        step, which is what CatBoost's generator yields.  numpy for numpy queries, a CUDA tensor for a CUDA tensor."""
        out = self._fitted().staged_predict_device(X, ntree_start, ntree_end, eval_period)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def eval_metrics(self, data, metrics=("RMSE",), ntree_start=0, ntree_end=0, eval_period=1):
        """``{"RMSE": [...]}`` for ``data = (X, y)``: the RMSE of every stage of ``staged_predict`` against ``y`` (``boosters.rmse_curve``:
        the staged matrix is scored on the device in one launch).  Any other metric is refused by name."""
        names = [metrics] if isinstance(metrics, str) else list(metrics)
        for name in names:
            if name != "RMSE":
                raise ValueError(f"{_WHO}: eval_metrics: the metric {name!r} is not supported (only 'RMSE')")
        if not names:
            raise ValueError(f"{_WHO}: eval_metrics: no metric is named")
        if not isinstance(data, (tuple, list)) or len(data) != 2:
            raise ValueError(f"{_WHO}: eval_metrics: data must be an (X, y) pair")
        X, y = data
        return {"RMSE": boosters.rmse_curve(self._fitted().staged_predict_device(X, ntree_start, ntree_end, eval_period), y)}

    def eval_curves(self, eval_set, learn=None, best_on=-1):
        """``{"learn": {"RMSE": [...]}, "validation": {"RMSE": [...]}}``, the layout of CatBoost's ``evals_result_``, with one value per
        iteration: what ``fit(..., eval_set=...)`` records in CatBoost, computed after the fit (the fit is deterministic and no validation
        row influences a tree).  ``eval_set`` is one ``(X, y)`` pair, keyed ``"validation"``, or a list of pairs, keyed ``"validation_0"``,
        ``"validation_1"``, ... when there are several; ``learn=(X, y)`` adds the ``"learn"`` curve.  Sets ``evals_result_`` and
        ``best_iteration_``: ``boosters.best_iteration`` of eval set number ``best_on`` (the last by default; which set CatBoost itself
        takes is unpinned).  ``shrink(get_best_iteration() + 1)`` then gives the model of ``use_best_model=True``."""
        model = self._fitted()
        pairs = boosters.eval_pairs(eval_set, _WHO, single=True)
        if not _is_int(best_on) or not -len(pairs) <= best_on < len(pairs):
            raise ValueError(f"{_WHO}: best_on={best_on!r} does not name one of the {len(pairs)} eval sets")
        result = {}
        if learn is not None:
            if not isinstance(learn, (tuple, list)) or len(learn) != 2:
                raise ValueError(f"{_WHO}: learn must be an (X, y) pair")
            X, y = learn
            result["learn"] = {"RMSE": boosters.rmse_curve(model.staged_predict_device(X), y)}
        for i, (X, y) in enumerate(pairs):
            result["validation" if len(pairs) == 1 else f"validation_{i}"] = {"RMSE": boosters.rmse_curve(model.staged_predict_device(X), y)}
        keys = [k for k in result if k != "learn"]
        self.evals_result_, self.best_iteration_ = result, boosters.best_iteration(result[keys[best_on]]["RMSE"])[0]
        return result

    def get_best_iteration(self):
        """``best_iteration_`` of the last ``eval_curves`` call (0-based, as CatBoost's)."""
        if not hasattr(self, "best_iteration_"):
            raise RuntimeError(f"{_WHO}: no best iteration: call eval_curves(eval_set) first (fit takes no eval_set)")
        return self.best_iteration_

    def shrink(self, ntree_end, ntree_start=0):
        """Keep the trees ``[ntree_start, ntree_end)`` in place (CatBoost's ``shrink``): ``trees_``, ``model_`` and ``tree_count_`` are
        rebuilt, ``train_approx_`` becomes ``None``, the constructor parameters stay.  With ``ntree_start = 0`` the result is the model a
        fit of ``ntree_end`` iterations gives: a shorter fit is a prefix of a longer one.  Returns ``self``."""
        self._fitted()
        t = self.trees_
        boosters._check_tree_range(f"{_WHO}.shrink", self.tree_count_, ntree_start, ntree_end)
        fs = np.asarray(t["tree_first_split"]).astype(np.int64)
        fl = np.concatenate([t["tree_first_leaf"], [len(t["leaf_values"])]]).astype(np.int64)
        s0, s1, l0, l1 = int(fs[ntree_start]), int(fs[ntree_end]), int(fl[ntree_start]), int(fl[ntree_end])
        trees = {k: np.asarray(t[k])[s0:s1].copy() for k in ("split_feature", "split_border", "split_bin") if k in t}
        trees.update({k: np.asarray(t[k])[l0:l1].copy() for k in ("leaf_values", "leaf_weights") if k in t})
        trees["tree_first_split"] = (fs[ntree_start:ntree_end + 1] - s0).astype(np.int32)
        trees["tree_first_leaf"] = fl[ntree_start:ntree_end] - l0
        return self._adopt({k: trees[k] for k in t}, self.bias_, self.n_features_in_)

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


# ---- the classifier: Logloss, two classes (the second part of the module docstring) -------------------------------------------------------
_CWHO = "CatBoostClassifier"
WEIGHT_STREAM = 2                                    # the bootstrap's stream tag of xgb.sample_hash; xgb's row and column draws hold 0 and 1
WEIGHT_BITS = 16                                     # fraction bits of a bootstrap weight
_BOOTSTRAPS = ("No", "Bayesian")
# as _NEUTRAL; the bootstrap and the bias are parameters of the constructor here
_CLASSIFIER_NEUTRAL = {**{k: v for k, v in _NEUTRAL.items() if k not in ("bootstrap_type", "bagging_temperature", "boost_from_average")},
                       "loss_function": ("Logloss",), "objective": ("Logloss",), "eval_metric": ("Logloss",), "leaf_estimation_method": ("Newton",),
                       "class_weights": (), "auto_class_weights": (), "scale_pos_weight": (1,), "class_names": (), "classes_count": (2,)}


def sigmoid64(x):
    """``sigmoid64`` of the module docstring on the host: float64 probabilities of float64 raw values, the bits ``csrc/catc.hip`` gives."""
    z = np.asarray(x, np.float64)
    a = np.maximum(-np.abs(z), -700.0)
    k = np.rint(a * xgb.INV_LN2)
    r = (a - k * xgb.LN2_HI) - k * xgb.LN2_LO
    P = np.full_like(r, xgb._EXP_COEFFS[13])
    for j in range(12, -1, -1):
        P = P * r + xgb._EXP_COEFFS[j]
    e = np.ldexp(P, k.astype(np.int32))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def weight_table(seed, temperature, iterations, n):
    """uint32 [iterations, n]: the Bayesian bootstrap's fixed-point weights of the module docstring, tree by row position.  Formed on the
    host: ``log`` and ``pow`` are not IEEE-exact on the device."""
    if not 0.0 <= float(temperature) <= 1.0:
        raise ValueError(f"{_CWHO}: bagging_temperature must lie in [0, 1], got {temperature!r}")
    h = xgb.sample_hash(0 if seed is None else seed, WEIGHT_STREAM, np.arange(int(iterations))[:, None], np.arange(int(n))[None, :])
    u = ((h >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    w = np.power(-np.log(u), np.float64(temperature))
    return np.maximum(1, np.rint(w * 2.0 ** WEIGHT_BITS).astype(np.int64)).astype(np.uint32)


def _binary_labels(y, n_rows, who=_CWHO):
    """(classes_, t): ``np.unique(y)`` of exactly two classes and the targets 0.0 / 1.0 as float64 [n_rows]."""
    y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
    if y.ndim == 2 and y.shape[1] == 1:
        y = y[:, 0]
    if y.ndim != 1 or (n_rows is not None and len(y) != n_rows):
        raise ValueError(f"{who}: y must hold one label per row of X, got shape {tuple(y.shape)} for {n_rows} rows")
    if y.dtype.kind == "f" and not np.isfinite(y).all():
        raise ValueError(f"{who}: y contains NaN or infinity")
    classes = np.unique(y)
    if len(classes) != 2:
        raise ValueError(f"{who}: y must hold exactly two classes (loss_function Logloss; MultiClass is not supported), got {len(classes)}: "
                         f"{classes[:5]!r}")
    return classes, (y == classes[1]).astype(np.float64)


def _proba_of_raw(raw):
    """float64 [m, 2] on the raw values' device: ``bbbp_catc_proba``."""
    raw = raw.contiguous()
    out = torch.empty((raw.shape[0], 2), dtype=torch.float64, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(_lib.lib().bbbp_catc_proba(_dense.stream(), raw.data_ptr(), raw.shape[0], out.data_ptr()), "bbbp_catc_proba")
    return out


class _ClassifierProblem(_Problem):
    """One classifier to fit: its outputs, its work area and the descriptor ``bbbp_catc_fit`` takes.  ``weights`` is the batch's table for
    the classifier's (seed, temperature), uint32 [>= iterations, stride] on the device, or None."""

    source = "csrc/catc.hip"

    def __init__(self, clf, up, rows, bins, n_cuts, classes, t, weights, dev):
        L = _lib.lib()
        n, d, T, D = bins.n, bins.d, int(clf.iterations), int(clf.depth)
        nbytes = L.bbbp_catc_fit_work_bytes(n, d, D)
        if not nbytes:
            raise ValueError("cat: " + L.bbbp_last_error().decode("utf-8", "replace"))
        self.up, self.rows, self.bins, self.n_cuts, self.T, self.D, self.classes, self.weights = up, rows, bins, n_cuts, T, D, classes, weights
        positives = float(t.sum())
        self.bias = 0.0 if clf.boost_from_average is False else float(np.log(np.float64(positives) / np.float64(len(t) - positives)))
        self.learning_rate = DEFAULT_LEARNING_RATE if clf.learning_rate is None else float(clf.learning_rate)
        self.y = torch.from_numpy(np.ascontiguousarray(t, np.float64)).to(dev)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.split_feature = torch.empty(T * D, dtype=torch.int32, device=dev)
        self.split_bin = torch.empty(T * D, dtype=torch.int32, device=dev)
        self.leaf_values = torch.empty(T << D, dtype=torch.float64, device=dev)
        self.leaf_weights = torch.empty(T << D, dtype=torch.int32, device=dev)
        self.tree_depth = torch.empty(T, dtype=torch.int32, device=dev)
        self.approx = torch.empty(n, dtype=torch.float64, device=dev)
        if weights is not None and (weights.shape[0] < T or weights.shape[1] < n):
            raise RuntimeError(f"cat: a weight table of shape {tuple(weights.shape)} for {T} trees of {n} rows")
        self.desc = _lib.CatcProblem(bins.bins.data_ptr(), n_cuts.data_ptr(), self.y.data_ptr(), weights.data_ptr() if weights is not None else None,
                                     weights.stride(0) if weights is not None else 0, n, d, T, D, float(clf.l2_leaf_reg), self.learning_rate, self.bias,
                                     self.work.data_ptr(), self.split_feature.data_ptr(), self.split_bin.data_ptr(), self.leaf_values.data_ptr(),
                                     self.leaf_weights.data_ptr(), self.tree_depth.data_ptr(), self.approx.data_ptr())


def _run_classifiers(problems, dev):
    arr = (_lib.CatcProblem * len(problems))(*[p.desc for p in problems])
    on_device = _tree_host.upload(arr, dev)
    _lib.check(_lib.lib().bbbp_catc_fit(_dense.stream(), arr, on_device.data_ptr(), len(problems)), "bbbp_catc_fit")
    return on_device                                  # the fit has synchronised the stream; kept alive by the caller all the same


class CatBoostClassifier(_estimator.Params):
    """``CatBoostClassifier(iterations=1000, learning_rate=None, depth=6, l2_leaf_reg=3.0, border_count=254, bagging_temperature=None,
    bootstrap_type=None, boost_from_average=None, random_seed=None, verbose=None, device="cuda")``: CatBoost's names for two classes under
    ``Logloss``; the regressor's aliases apply (``random_state``, ``n_estimators``, ``max_depth``, ``reg_lambda``), and ``loss_function`` /
    ``objective`` / ``eval_metric`` pass as ``"Logloss"``.  ``bootstrap_type`` is ``None``, ``"No"`` or ``"Bayesian"``: ``None`` means
    ``"Bayesian"`` when ``bagging_temperature`` is given and ``"No"`` otherwise, ``"Bayesian"`` without a temperature means 1.0; the
    temperature lies in [0, 1].  The reference's ``CatBoostClassifier(iterations=500, learning_rate=0.03, depth=10, l2_leaf_reg=5,
    bagging_temperature=0.5, loss_function="Logloss", verbose=0, random_seed=42)`` (Models/model_opt_20250130.py:413-457) builds as written.
    Everything else is refused by name with ``ValueError`` (the module docstring lists it, with the algorithm, the deviations and the
    unpinned parity with the catboost package).

    ``fit(X, y)`` takes what the regressor's takes, with finite features, and labels of any dtype in exactly two classes.  It sets
    ``classes_``, ``model_`` (a ``boosters.CatBoostTrees`` of raw values), ``trees_``, ``bias_``, ``tree_count_``, ``n_features_in_`` and
    ``train_approx_`` (float64: the training rows' raw values as the fit summed them; ``predict(X_train,
    prediction_type="RawFormulaVal")`` equals it bit for bit).  ``predict_proba`` / ``predict_log_proba`` are float64 [m, 2], ``predict`` takes
    ``prediction_type="Class" | "Probability" | "RawFormulaVal"``; numpy in gives numpy out, a CUDA tensor in a CUDA tensor, answered from
    the device.  ``get_model_json`` / ``save_model`` write CatBoost's JSON export schema; ``get_params`` / ``set_params`` make
    ``sklearn.base.clone`` and ``ensemble.StackingClassifier`` / ``VotingClassifier`` work."""

    _params = ("iterations", "learning_rate", "depth", "l2_leaf_reg", "border_count", "bagging_temperature", "bootstrap_type", "boost_from_average",
               "random_seed", "verbose", "device")

    def __init__(self, iterations=1000, learning_rate=None, depth=6, l2_leaf_reg=3.0, border_count=254, bagging_temperature=None, bootstrap_type=None,
                 boost_from_average=None, random_seed=None, verbose=None, device="cuda", **other):
        given = dict(iterations=iterations, depth=depth, l2_leaf_reg=l2_leaf_reg, random_seed=random_seed)
        for alias, name in _ALIASES.items():
            if alias in other:
                value = other.pop(alias)
                if given[name] is not _DEFAULTS[name] and given[name] != _DEFAULTS[name]:
                    raise ValueError(f"{_CWHO}: {alias} is an alias of {name}: only one of them may be given")
                given[name] = value
        _refuse(other, _CWHO, _CLASSIFIER_NEUTRAL)
        border_count = 254 if border_count is None else border_count
        _check_params(given["iterations"], learning_rate, given["depth"], given["l2_leaf_reg"], border_count, given["random_seed"], who=_CWHO)
        seed = given["random_seed"]
        if seed is not None and not 0 <= seed < 2 ** 64:
            raise ValueError(f"{_CWHO}: random_seed must be None or an int in 0..2^64-1, got {seed!r}")
        if bootstrap_type is not None and bootstrap_type not in _BOOTSTRAPS:
            raise ValueError(f"{_CWHO}: bootstrap_type={bootstrap_type!r} is not supported (only 'No', 'Bayesian' or None: MVS, Bernoulli and "
                             "Poisson sampling are not built)")
        if bagging_temperature is not None:
            xgb._number(bagging_temperature, "bagging_temperature", 0.0, who=_CWHO)
            if bagging_temperature > 1:
                raise ValueError(f"{_CWHO}: bagging_temperature must lie in [0, 1] (the weights are fixed point below 2^22), got {bagging_temperature!r}")
            if bootstrap_type == "No":
                raise ValueError(f"{_CWHO}: bagging_temperature={bagging_temperature!r} needs bootstrap_type='Bayesian' or None, got 'No'")
        if boost_from_average is not None and not isinstance(boost_from_average, (bool, np.bool_)):
            raise ValueError(f"{_CWHO}: boost_from_average must be None, True or False, got {boost_from_average!r}")
        if isinstance(device, (list, tuple)):
            raise ValueError(f"{_CWHO}: device={device!r}: more than one GPU is not supported")
        # the parameters are kept as they were given: sklearn.base.clone compares them by identity
        self.iterations, self.depth, self.l2_leaf_reg, self.random_seed = given["iterations"], given["depth"], given["l2_leaf_reg"], given["random_seed"]
        self.learning_rate, self.border_count, self.verbose, self.device = learning_rate, border_count, verbose, device
        self.bagging_temperature, self.bootstrap_type, self.boost_from_average = bagging_temperature, bootstrap_type, boost_from_average

    def set_params(self, **params):
        return super().set_params(**{_ALIASES.get(k, k): v for k, v in params.items()})

    def _temperature(self):
        """The Bayesian bootstrap's temperature, or None without a bootstrap."""
        if self.bagging_temperature is not None:
            return float(self.bagging_temperature)
        return 1.0 if self.bootstrap_type == "Bayesian" else None

    # ---- fit --------------------------------------------------------------------------------------------------------
    def fit(self, X, y, cat_features=None, text_features=None, embedding_features=None, sample_weight=None, eval_set=None, early_stopping_rounds=None,
            use_best_model=None, **other):
        if cat_features is not None or text_features is not None or embedding_features is not None:
            raise ValueError(f"{_CWHO}: categorical, text and embedding features are not supported (float features only)")
        if sample_weight is not None:
            raise ValueError(f"{_CWHO}: sample_weight is not supported")
        if eval_set is not None or early_stopping_rounds is not None or use_best_model:
            raise ValueError(f"{_CWHO}: eval_set and early stopping are not supported")
        rest = set(other) - {"verbose", "verbose_eval", "silent", "logging_level", "plot", "metric_period"}
        if rest:
            raise ValueError(f"{_CWHO}: fit arguments {sorted(rest)} are not supported")
        _fit_classifiers([self], [(X, y)])
        return self

    def _adopt(self, classes, trees, bias, n_features, train_approx=None):
        self.classes_ = np.asarray(classes)
        return CatBoostRegressor._adopt(self, trees, bias, n_features, train_approx)

    @classmethod
    def from_trees(cls, trees, bias, n_features, classes=(0, 1), device="cuda", **params):
        """A classifier around fitted arrays (``trees_``' keys): for prediction and the JSON export.  ``device="cpu"`` gives a model that
        exports and validates but cannot predict."""
        classes = np.asarray(classes)
        if classes.shape != (2,) or not np.array_equal(np.unique(classes), classes):
            raise ValueError(f"{_CWHO}: classes must be two distinct labels in ascending order, got {classes!r}")
        self = cls(device=device, **params)
        return self._adopt(classes, {k: np.asarray(v) for k, v in trees.items()}, bias, n_features)

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _fitted(self):
        if not hasattr(self, "model_"):
            raise RuntimeError(f"{_CWHO}: not fitted")
        return self.model_

    def predict_device(self, X):
        """float64 [m] on the device: the raw values, ``bias_`` behind the sum of the trees' leaf values (``bbbp_oblivious_predict``)."""
        return self._fitted().predict_device(X)

    def predict_proba(self, X):
        """float64 [m, 2]: ``(1 - p1, p1)`` with ``p1 = sigmoid64(raw)`` (``bbbp_catc_proba``)."""
        out = _proba_of_raw(self.predict_device(X))
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict_log_proba(self, X):
        """float64 [m, 2]: the logarithm of ``predict_proba``; a logarithm of finished probabilities is plumbing (torch's, on the device)."""
        out = torch.log(_proba_of_raw(self.predict_device(X)))
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def predict(self, X, prediction_type="Class"):
        """``classes_[raw > 0]``, the probabilities or the raw values: numpy for numpy queries; for a CUDA tensor a CUDA tensor (of the labels
        when they are numbers)."""
        if prediction_type == "Probability":
            return self.predict_proba(X)
        if prediction_type not in ("Class", "RawFormulaVal"):
            raise ValueError(f"{_CWHO}: prediction_type={prediction_type!r} is not supported (only 'Class', 'Probability' or 'RawFormulaVal')")
        raw = self.predict_device(X)
        if prediction_type == "RawFormulaVal":
            return raw if isinstance(X, torch.Tensor) else raw.cpu().numpy()
        positive = raw > 0
        if isinstance(X, torch.Tensor) and self.classes_.dtype.kind in "biuf":
            return torch.from_numpy(self.classes_).to(positive.device)[positive.long()]
        return self.classes_[positive.cpu().numpy().astype(np.intp)]

    # ---- export -----------------------------------------------------------------------------------------------------
    def get_model_json(self):
        """The regressor's document with ``loss_function.type = "Logloss"`` and ``model_info.class_params`` (``class_names``,
        ``class_to_label``, ``class_label_type``); ``boosters.CatBoostTrees.from_json`` reads it back to the same arrays, which give raw
        values.  That CatBoost itself loads it is UNPINNED: the package is absent (see the module docstring)."""
        doc = json.loads(CatBoostRegressor.get_model_json(self))
        doc["model_info"]["params"]["loss_function"] = {"type": "Logloss"}
        kind = self.classes_.dtype.kind
        doc["model_info"]["class_params"] = {"class_label_type": "Integer" if kind in "biu" else "Float" if kind == "f" else "String",
                                             "class_names": [c.item() if kind in "biuf" else str(c) for c in self.classes_], "class_to_label": [0, 1]}
        return json.dumps(doc)

    def save_model(self, path, format="json"):
        if format != "json":
            raise ValueError(f"{_CWHO}: save_model writes format='json' only, got {format!r}")
        with open(path, "w") as f:
            f.write(self.get_model_json())


def _fit_classifiers(classifiers, problems):
    """Fit ``classifiers[i]`` on ``problems[i] = (X, y)`` or ``(X, y, rows)`` in one ``bbbp_catc_fit`` batch.  Uploads and bin matrices are
    shared as ``_fit`` shares them; cuts, classes, the bias and the weights (by a row's position within the problem) are the problem's own:
    a fold fitted in a batch equals the fold fitted alone bit for bit.  One weight table per (seed, temperature) serves the batch."""
    devices = {str(_cuda_device(clf.device, _CWHO)) for clf in classifiers}
    if len(devices) != 1:
        raise ValueError(f"{_CWHO}: the classifiers of one batch name the devices {sorted(devices)}: more than one GPU is not supported")
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
            raise ValueError(f"{_CWHO}: n = {n} rows, more than {MAX_ROWS} are not supported (BBBP_CAT_FIT_MAX_N)")
        if n is not None and n < 2:
            raise ValueError(f"{_CWHO}: at least two rows are needed, got {n}")
        y_all = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
        if y_all.ndim == 2 and y_all.shape[1] == 1:
            y_all = y_all[:, 0]
        if y_all.ndim != 1 or (n_all is not None and len(y_all) != n_all):
            raise ValueError(f"{_CWHO}: y must hold one label per row of X, got shape {tuple(y_all.shape)} for {n_all} rows")
        classes, t = _binary_labels(y_all if rows is None else y_all[rows], n)
        if id(X) not in uploads:
            uploads[id(X)] = xgb._Upload(X, who=_CWHO)
        up = uploads[id(X)]
        if len(up.cols) == 0:
            raise ValueError(f"{_CWHO}: all features are constant")
        if rows is None and len(up.cols) > MAX_LIVE_FEATURES:
            raise ValueError(f"{_CWHO}: {len(up.cols)} live features, more than {MAX_LIVE_FEATURES} are not supported (BBBP_CAT_FIT_MAX_D)")
        checked.append((X, classes, t, rows))
    with torch.cuda.device(dev):
        binned, per_problem = {}, []
        for clf, (X, classes, t, rows) in zip(classifiers, checked):
            up = uploads[id(X)].upload(dev)
            key = (id(X), None if rows is None else rows.tobytes(), int(clf.border_count))
            if key not in binned:
                try:
                    bins = xgb._Bins(up, rows, int(clf.border_count) + 1, dev, who=_CWHO)
                except NotImplementedError as e:
                    raise ValueError(str(e)) from None
                n_cuts = torch.isfinite(bins.cuts).sum(dim=1).to(torch.int32).contiguous()
                if int(n_cuts.min()) < 1:                 # xgb._Bins' dead feature: no column of these rows has a cut
                    raise ValueError(f"{_CWHO}: all features are constant")
                binned[key] = (bins, n_cuts)
            per_problem.append((up, binned[key]))
        shapes = {}                                       # (seed, temperature) -> (most trees, most rows) among the problems that draw from it
        for clf, (_, (bins, _)) in zip(classifiers, per_problem):
            if clf._temperature() is not None:
                key = (0 if clf.random_seed is None else int(clf.random_seed), clf._temperature())
                T, n = shapes.get(key, (0, 0))
                shapes[key] = (max(T, int(clf.iterations)), max(n, bins.n))
        tables = {}
        for key, (T, n) in shapes.items():
            tables[key] = torch.empty((T, n), dtype=torch.int32, device=dev)
            tables[key].copy_(torch.from_numpy(weight_table(key[0], key[1], T, n).view(np.int32)))
        fits = []
        for clf, (X, classes, t, rows), (up, (bins, n_cuts)) in zip(classifiers, checked, per_problem):
            key = (0 if clf.random_seed is None else int(clf.random_seed), clf._temperature())
            fits.append(_ClassifierProblem(clf, up, rows, bins, n_cuts, classes, t, tables.get(key), dev))
        keep = _run_classifiers(fits, dev)
        for clf, fit in zip(classifiers, fits):
            clf._adopt(fit.classes, fit.trees(dev), fit.bias, fit.up.d, fit.approx.cpu().numpy())
        del keep


def fit_classifiers(problems, **params):
    """``[CatBoostClassifier(**params).fit(X[rows], y[rows]) for X, y, rows in problems]`` with every problem in one batch (``(X, y)`` means
    all rows): five folds and the refit are one call.  Each classifier equals its single ``fit`` bit for bit."""
    problems = list(problems)
    if not problems:
        raise ValueError("cat.fit_classifiers: no problems")
    classifiers = [CatBoostClassifier(**params) for _ in problems]
    _fit_classifiers(classifiers, problems)
    return classifiers


# ---- the reference's randomized search ------------------------------------------------------------------------------------------------------
_SEARCH_KEYS = ("iterations", "learning_rate", "depth", "l2_leaf_reg", "border_count", "bagging_temperature")


def _prefix_raw(clf, Xq, lengths):
    """{T: float64 raw values of ``clf``'s first T trees on the device rows ``Xq``}.  A prefix is a model of its own
    (``boosters.CatBoostTrees`` over the first T trees), so each equals the raw values of the shorter fit bit for bit."""
    t, out = clf.trees_, {}
    first_leaf = np.concatenate([t["tree_first_leaf"], [len(t["leaf_values"])]])
    for T in lengths:
        ns, nl = int(t["tree_first_split"][T]), int(first_leaf[T])
        short = boosters.CatBoostTrees(t["split_feature"][:ns], t["split_border"][:ns], np.zeros(clf.n_features_in_, np.uint8), t["tree_first_split"][:T + 1],
                                       t["tree_first_leaf"][:T], t["leaf_values"][:nl], clf.n_features_in_, 1.0, float(clf.bias_), device=clf.device)
        out[T] = short.predict_device(Xq)
    return out


def randomized_search_cv(X, y, param_distributions, n_iter=50, cv=5, scoring=("accuracy", "precision"), refit="accuracy", random_state=None, device="cuda",
                         **fixed):
    """The reference's ``RandomizedSearchCV(CatBoostClassifier(...), param_grid, n_iter=50, cv=StratifiedKFold(5), scoring={accuracy,
    precision}, refit="accuracy")`` (Models/model_opt_20250130.py:533-561) over ``iterations``, ``learning_rate``, ``depth``, ``l2_leaf_reg``,
    ``border_count`` and ``bagging_temperature``; ``fixed`` holds the estimator's other parameters.

    The points are scikit-learn's ``ParameterSampler(param_distributions, n_iter, random_state=random_state)``, the folds
    ``StratifiedKFold(cv)`` without shuffling.  The weights of tree ``t`` do not depend on ``iterations``, so a model of T trees is the prefix
    of a longer one: every fold fits one chain per distinct setting of everything but ``iterations`` to the longest length asked of it, all
    chains of all folds in one ``bbbp_catc_fit`` batch, and the shorter models are scored from tree prefixes of the fold's test rows.  Scores
    come through ``bbbp_amd.metrics`` with ``classes_[1]`` as the positive class (an undefined precision counts 0, scikit-learn's default).
    Returns (best_params, {name: mean score per point}, the classifier refitted on all rows with best_params); the first maximum of
    ``refit`` wins."""
    from sklearn.model_selection import ParameterSampler, StratifiedKFold
    from . import metrics
    who = "cat.randomized_search_cv"
    score_keys = {"accuracy": "Accuracy", "precision": "Precision", "recall": "Recall", "f1": "F1 Score"}
    scoring = (scoring,) if isinstance(scoring, str) else tuple(scoring)
    unknown = [s for s in scoring if s not in score_keys]
    if unknown or not scoring:
        raise ValueError(f"{who}: scoring {unknown!r} is not supported (only {sorted(score_keys)})")
    if refit not in scoring:
        raise ValueError(f"{who}: refit={refit!r} is not one of the scores {scoring!r}")
    dev = _cuda_device(device, who)
    strangers = set(param_distributions) - set(_SEARCH_KEYS)
    if strangers:
        raise ValueError(f"{who}: the parameters {sorted(strangers)} cannot be searched (only {list(_SEARCH_KEYS)})")
    points = list(ParameterSampler(param_distributions, n_iter=n_iter, random_state=random_state))
    models = [CatBoostClassifier(**{**fixed, **pt, "device": dev}) for pt in points]       # every point is checked before anything is fitted
    X = np.asarray(X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else X)
    y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
    classes, _ = _binary_labels(y, X.shape[0] if X.ndim == 2 else None, who)
    folds = list(StratifiedKFold(n_splits=cv).split(np.zeros((len(y), 1)), y))
    rest_of = lambda m: tuple((k, v) for k, v in m.get_params().items() if k not in ("iterations", "device"))  # noqa: E731
    longest = {}
    for m in models:
        longest[rest_of(m)] = max(longest.get(rest_of(m), 0), int(m.iterations))
    chains, problems = {}, []
    for fi, (tr, _) in enumerate(folds):
        for rest, T in longest.items():
            chains[(fi, rest)] = CatBoostClassifier(iterations=T, device=dev, **dict(rest))
            problems.append((X, y, tr))
    _fit_classifiers(list(chains.values()), problems)
    table = {s: np.zeros((len(points), len(folds))) for s in scoring}
    with torch.cuda.device(dev):
        for fi, (_, te) in enumerate(folds):
            Xq = torch.from_numpy(np.ascontiguousarray(X[te], dtype=np.float32)).to(dev)
            for rest in longest:
                chain = chains[(fi, rest)]
                members = [pi for pi, m in enumerate(models) if rest_of(m) == rest]
                raw = _prefix_raw(chain, Xq, sorted({int(models[pi].iterations) for pi in members}))
                preds = np.stack([chain.classes_[(raw[int(models[pi].iterations)] > 0).cpu().numpy().astype(np.intp)] for pi in members])
                got = metrics.classification_scores(y[te], preds, pos_label=classes[1], zero_division=0, device=dev)
                for s in scoring:
                    table[s][members, fi] = got[score_keys[s]][:, 0]
    means = {s: [float(v) for v in table[s].mean(axis=1)] for s in scoring}
    best = int(np.argmax(means[refit]))
    fitted = CatBoostClassifier(**{**fixed, **points[best], "device": dev}).fit(X, y)
    return points[best], means, fitted
