"""GPU: staged prediction of both boosted families (``bbbp_gbt_staged_predict`` / ``bbbp_oblivious_staged_predict``) and the regressor
API on top of it.  Everything is compared on bit patterns: a stage against the existing predict kernels run on the truncated model (the
contract), and the whole matrix against the numpy restatement of ``tests/staged_numpy.py``.

Synthetic models hold the tree shapes that take different paths (a chain of depth 40, single leaves, oblivious depths 0, 1 and 6) and
the queries about 10 % NaN (default children, NaN-as-true features).  Rows: 1, one below / at / above a work-group of 256, and 700 (three
work-groups, and seven chunks at 100 rows per call, where the output's leading dimension exceeds the chunk)."""
import functools

import numpy as np
import pytest
import torch

import cat_numpy as cn
import staged_numpy as S
from bbbp_amd import boosters, metrics

pytestmark = pytest.mark.gpu

D = 9
ROWS = (1, 255, 256, 257, 700)
FAMILIES = {"gbt": (S.random_gbt, S.xgb_trees, S.gbt_leaves, S.staged_gbt, torch.float32),
            "oblivious": (S.random_oblivious, S.cat_trees, S.oblivious_leaves, S.staged_oblivious, torch.float64)}


@functools.lru_cache(maxsize=None)
def synthetic(family, T):
    return FAMILIES[family][0](T, D, seed=100 + T)


@functools.lru_cache(maxsize=None)
def query(n):
    return S.queries(n, D, seed=n)


_truncated = {}


def truncated(full, family, T, start, end):
    """The truncated model, built and uploaded once per (family, T, start, end)."""
    key = (family, T, start, end)
    if key not in _truncated:
        _truncated[key] = full.truncated(start, end)
    return _truncated[key]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("T", [1, 2, 7, 40])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_stages_equal_the_truncated_models_predictions_and_the_restatement(dev, family, T, n):
    _, build, leaves_of, staged_of, dtype = FAMILIES[family]
    model, X = synthetic(family, T), query(n)
    full = build(model, dev)
    leaves = leaves_of(model, X)
    Xd = torch.from_numpy(X).to(dev)
    predicted = {}
    for start, end, period in S.triples(T):
        ends = boosters.stage_ends(T, start, end, period)
        want = staged_of(model, X, ends, start, leaves=leaves)
        for rows_per_call in (None, 100):
            kw = {} if rows_per_call is None else dict(rows_per_call=rows_per_call)
            got = full.staged_predict_device(Xd, start, end, period, **kw)
            assert got.dtype == dtype and got.shape == (len(ends), n) and got.is_contiguous() and got.device.type == "cuda"
            got = got.cpu().numpy()
            what = (family, T, n, start, end, period, rows_per_call)
            for k, e in enumerate(ends):                            # 1. the kernel against the existing kernel on the truncated model
                if (start, int(e)) not in predicted:
                    predicted[start, int(e)] = truncated(full, family, T, start, int(e)).predict_device(Xd).cpu().numpy()
                assert np.array_equal(S.bits(got[k]), S.bits(predicted[start, int(e)])), (what, k)
            assert np.array_equal(S.bits(got), S.bits(want)), what   # 2. the matrix against the numpy oracle
    assert np.array_equal(S.bits(full.staged_predict_device(X, period=T).cpu().numpy()[0]), S.bits(full.predict(X)))      # a numpy query


def test_no_rows_and_bad_arguments(dev):
    for family in FAMILIES:
        full = FAMILIES[family][1](synthetic(family, 7), dev)
        out = full.staged_predict_device(np.zeros((0, D), np.float32), period=3)
        assert out.shape == (3, 0) and out.dtype == FAMILIES[family][4]
        for bad in (dict(tree_start=7), dict(tree_end=8), dict(tree_start=3, tree_end=3), dict(period=0)):
            with pytest.raises(ValueError):
                full.staged_predict_device(query(1), **bad)
        with pytest.raises(ValueError, match="X must be"):
            full.staged_predict_device(np.zeros((3, D + 1), np.float32))


def test_a_model_without_any_split_predicts(dev):
    """Depth-0 trees only, which a truncation can be: the empty split arrays have no device address of their own, yet the model predicts
    ``scale * (the sum of its single leaves) + bias``, staged and whole."""
    from oracle import reference_cpu as oracle
    m = dict(S.random_oblivious(3, D, seed=5), split_feature=np.zeros(0, np.int32), split_border=np.zeros(0, np.float32),
             tree_first_split=np.zeros(4, np.int32), tree_first_leaf=np.arange(3, dtype=np.int64), leaf_values=np.asarray([0.25, -1.5, 3.0]))
    trees, X = S.cat_trees(m, dev), query(257)
    want = oracle.catboost_predict(*(m[k] for k in S.OBL_KEYS), m["scale"], m["bias"], X)
    assert np.array_equal(S.bits(trees.predict(X)), S.bits(want))
    staged = trees.staged_predict_device(X).cpu().numpy()
    assert np.array_equal(S.bits(staged), S.bits(S.staged_oblivious(m, X, [1, 2, 3]))) and np.array_equal(S.bits(staged[-1]), S.bits(want))


# ---- fitted models --------------------------------------------------------------------------------------------------------------------------------
T_FIT = 20


@functools.lru_cache(maxsize=None)
def fitted(dev):
    from bbbp_amd import cat, xgb
    Xtr, ytr, Xte, yte = S.fitted_problem()
    return (xgb.XGBRegressor(n_estimators=T_FIT, max_depth=3, device=dev).fit(Xtr, ytr),
            cat.CatBoostRegressor(iterations=T_FIT, depth=3, learning_rate=0.1, device=dev).fit(Xtr, ytr))


def test_fitted_staged_predict_ends_where_predict_and_the_fit_end(dev):
    Xtr, ytr, Xte, _ = S.fitted_problem()
    xreg, creg = fitted(dev)
    for reg, dtype in ((xreg, np.float32), (creg, np.float64)):
        for X in (Xtr, Xte):
            staged = reg.staged_predict(X)
            assert isinstance(staged, np.ndarray) and staged.dtype == dtype and staged.shape == (T_FIT, len(X))
            assert np.array_equal(S.bits(staged[-1]), S.bits(reg.predict(X)))
            assert [len(stage) for stage in staged] == [len(X)] * T_FIT            # iterating gives one stage per step
        on_device = reg.staged_predict(torch.from_numpy(Xte).to(dev))
        assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(S.bits(on_device.cpu().numpy()), S.bits(reg.staged_predict(Xte)))
    # the fit's own sums: CatBoost's bit for bit; XGBoost's fit adds base_score first, predict last (tests/test_gpu_xgb.py::test_prediction)
    assert np.array_equal(S.bits(creg.staged_predict(Xtr)[-1]), S.bits(creg.train_approx_))
    bound = T_FIT * np.spacing(np.float32(np.abs(xreg.train_margin_).max() + np.abs(xreg.base_score_)))
    assert np.abs(xreg.staged_predict(Xtr)[-1].astype(np.float64) - xreg.train_margin_.astype(np.float64)).max() <= bound
    # the restatement on the fitted arrays, and coarser periods
    ox, oc = S.of_xgb(xreg.trees_, xreg.base_score_, Xtr.shape[1]), S.of_cat(creg.trees_, creg.bias_, Xtr.shape[1])
    for period in (1, 3, 7, 20, 25):
        ends = boosters.stage_ends(T_FIT, period=period)
        assert np.array_equal(S.bits(xreg.staged_predict(Xte, period=period)), S.bits(S.staged_gbt(ox, Xte, ends)))
        assert np.array_equal(S.bits(creg.staged_predict(Xte, eval_period=period)), S.bits(S.staged_oblivious(oc, Xte, ends)))
    assert np.array_equal(S.bits(creg.staged_predict(Xte, 3, 17, 4)), S.bits(S.staged_oblivious(oc, Xte, boosters.stage_ends(T_FIT, 3, 17, 4), 3)))


def test_fitted_predict_over_a_tree_range(dev):
    _, _, Xte, _ = S.fitted_problem()
    xreg, creg = fitted(dev)
    Xd = torch.from_numpy(Xte).to(dev)
    for begin, end in ((3, 9), (0, 1), (19, 20), (5, 0), (0, 20)):
        stop = T_FIT if end == 0 else end
        want = xreg.booster_.truncated(begin, stop).predict(Xte)
        got = xreg.predict(Xte, iteration_range=(begin, end))
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(S.bits(got), S.bits(want)), (begin, end)
        on_device = xreg.predict(Xd, iteration_range=(begin, end))
        assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(S.bits(on_device.cpu().numpy()), S.bits(want))
        want = creg.model_.truncated(begin, stop).predict(Xte)
        got = creg.predict(Xte, ntree_start=begin, ntree_end=end)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(S.bits(got), S.bits(want)), (begin, end)
        on_device = creg.predict(Xd, ntree_start=begin, ntree_end=end)
        assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(S.bits(on_device.cpu().numpy()), S.bits(want))
    for whole in (None, (0, 0)):
        assert np.array_equal(S.bits(xreg.predict(Xte, iteration_range=whole)), S.bits(xreg.predict(Xte)))
    assert np.array_equal(S.bits(creg.predict(Xte, 0, 0)), S.bits(creg.predict(Xte)))


def test_eval_curves_equal_the_restatement_and_count_one_launch_per_eval_set(dev):
    Xtr, ytr, Xte, yte = S.fitted_problem()
    xreg, creg = fitted(dev)
    ox, oc = S.of_xgb(xreg.trees_, xreg.base_score_, Xtr.shape[1]), S.of_cat(creg.trees_, creg.bias_, Xtr.shape[1])
    all_ends = boosters.stage_ends(T_FIT)
    want_x = {"validation_0": {"rmse": S.rmse_curve(S.staged_gbt(ox, Xtr, all_ends), ytr)}, "validation_1": {"rmse": S.rmse_curve(S.staged_gbt(ox, Xte, all_ends), yte)}}
    want_c = {"learn": {"RMSE": S.rmse_curve(S.staged_oblivious(oc, Xtr, all_ends), ytr)}, "validation": {"RMSE": S.rmse_curve(S.staged_oblivious(oc, Xte, all_ends), yte)}}

    def same(got, want):
        assert list(got) == list(want)
        for key in want:
            (name, curve), = got[key].items()
            assert name == next(iter(want[key])) and isinstance(curve, list) and all(type(v) is float for v in curve)
            assert len(curve) == len(want[key][name]) and np.array_equal(S.bits(np.asarray(curve)), S.bits(np.asarray(want[key][name]))), key

    before = metrics._LAUNCHES["sq_sums"]
    got = xreg.eval_curves([(Xtr, ytr), (Xte, yte)])
    assert metrics._LAUNCHES["sq_sums"] == before + 2                       # one launch per eval set for all 20 stages
    same(got, want_x)
    assert xreg.evals_result() is got and xreg.evals_result_ is got and [len(v["rmse"]) for v in got.values()] == [T_FIT, T_FIT]
    before = metrics._LAUNCHES["sq_sums"]
    coarse = xreg.eval_curves([(torch.from_numpy(Xte).to(dev), yte)], period=7)
    assert metrics._LAUNCHES["sq_sums"] == before + 1                       # ... whatever K is
    same(coarse, {"validation_0": {"rmse": S.rmse_curve(S.staged_gbt(ox, Xte, [7, 14, 20]), yte)}})
    assert coarse["validation_0"]["rmse"][-1] == got["validation_1"]["rmse"][-1] and xreg.evals_result() is coarse

    before = metrics._LAUNCHES["sq_sums"]
    got = creg.eval_curves((Xte, yte), learn=(Xtr, ytr))
    assert metrics._LAUNCHES["sq_sums"] == before + 2
    same(got, want_c)
    assert creg.evals_result_ is got
    several = creg.eval_curves([(Xtr, ytr), (Xte, yte)])
    same(several, {"validation_0": want_c["learn"], "validation_1": want_c["validation"]})
    assert creg.get_best_iteration() == boosters.best_iteration(want_c["validation"]["RMSE"])[0]
    creg.eval_curves([(Xtr, ytr), (Xte, yte)], best_on=0)
    assert creg.get_best_iteration() == T_FIT - 1                           # the learn curve only falls
    before = metrics._LAUNCHES["sq_sums"]
    assert creg.eval_metrics((Xte, yte)) == want_c["validation"] and creg.eval_metrics((Xte, yte), metrics=["RMSE"]) == want_c["validation"]
    assert metrics._LAUNCHES["sq_sums"] == before + 2
    part = creg.eval_metrics((Xte, yte), "RMSE", ntree_start=2, ntree_end=17, eval_period=4)
    same({"v": part}, {"v": {"RMSE": S.rmse_curve(S.staged_oblivious(oc, Xte, boosters.stage_ends(T_FIT, 2, 17, 4), 2), yte)}})
    for bad_y in (np.where(np.arange(len(yte)) == 3, np.nan, yte), yte[:-1]):
        with pytest.raises(ValueError):
            creg.eval_curves((Xte, bad_y))
    bad_X = Xte.copy()
    bad_X[0, 0] = np.nan                                                   # a NaN feature is "missing" to predict and gives finite predictions
    assert np.isfinite(creg.eval_curves((bad_X, yte))["validation"]["RMSE"]).all()


def test_shrink_to_the_best_iteration_reproduces_use_best_model(dev):
    """The reference's ``fit(..., eval_set=(X_test, y_test), use_best_model=True)``: the curves, the best iteration and the truncated model,
    all after the fit.  The problem is chosen so that the numpy-fitted model's held-out optimum lies strictly inside the run; that is
    checked first, on the restatement alone."""
    from bbbp_amd import cat, xgb
    Xtr, ytr, Xte, yte = S.fitted_problem()
    ref = cn.fit(Xtr, ytr, iterations=T_FIT, depth=3, learning_rate=0.1)
    oc = S.of_cat(ref, ref["bias"], Xtr.shape[1])
    ends = boosters.stage_ends(T_FIT)
    learn, held_out = S.rmse_curve(S.staged_oblivious(oc, Xtr, ends), ytr), S.rmse_curve(S.staged_oblivious(oc, Xte, ends), yte)
    best = int(np.argmin(held_out))
    assert 0 < best < T_FIT - 1 and boosters.best_iteration(held_out) == (best, T_FIT), "the problem no longer has its optimum inside the run"
    assert np.all(np.diff(learn) <= 0)

    creg = cat.CatBoostRegressor(iterations=T_FIT, depth=3, learning_rate=0.1, device=dev).fit(Xtr, ytr)
    stages = creg.staged_predict(Xte)
    curves = creg.eval_curves((Xte, yte), learn=(Xtr, ytr))
    assert np.array_equal(S.bits(np.asarray(curves["learn"]["RMSE"])), S.bits(np.asarray(learn)))
    assert np.array_equal(S.bits(np.asarray(curves["validation"]["RMSE"])), S.bits(np.asarray(held_out)))
    assert creg.get_best_iteration() == creg.best_iteration_ == best
    assert creg.shrink(creg.get_best_iteration() + 1) is creg
    assert creg.tree_count_ == best + 1 == creg.model_.n_trees and creg.train_approx_ is None and creg.iterations == T_FIT
    assert np.array_equal(S.bits(creg.predict(Xte)), S.bits(stages[best]))
    again = cat.CatBoostRegressor(iterations=best + 1, depth=3, learning_rate=0.1, device=dev).fit(Xtr, ytr)
    assert all(np.array_equal(S.bits(creg.trees_[k]), S.bits(again.trees_[k])) for k in again.trees_)      # a shorter fit is a prefix of a longer one
    assert creg.evals_result_ is curves                                    # CatBoost keeps the full curves after the cut

    xreg = xgb.XGBRegressor(n_estimators=T_FIT, max_depth=3, device=dev).fit(Xtr, ytr)
    stages = xreg.staged_predict(Xte)
    curve = xreg.eval_curves([(Xtr, ytr), (Xte, yte)])["validation_1"]["rmse"]
    best_x, stop = boosters.best_iteration(curve, early_stopping_rounds=5)
    assert xreg.shrink(best_x + 1) is xreg and xreg.booster_.n_trees == best_x + 1 and xreg.train_margin_ is None
    assert np.array_equal(S.bits(xreg.predict(Xte)), S.bits(stages[best_x]))
    again = xgb.XGBRegressor(n_estimators=best_x + 1, max_depth=3, device=dev).fit(Xtr, ytr)
    assert all(np.array_equal(S.bits(xreg.trees_[k]), S.bits(again.trees_[k])) for k in again.trees_)
    assert xreg.get_model_json() == again.get_model_json() and 0 <= best_x < stop <= T_FIT


def test_staged_calls_work_on_a_classifiers_trees(dev):
    """Out of scope for the classifiers' own API, in scope for ``boosters``: the margins of an ``XGBClassifier``'s ``booster_`` and the raw
    values of a ``CatBoostClassifier``'s ``model_``, staged."""
    from bbbp_amd import cat, xgb
    Xtr, ytr, Xte, _ = S.fitted_problem()
    labels = (ytr > np.median(ytr)).astype(np.int64)
    xclf = xgb.XGBClassifier(n_estimators=5, max_depth=3, device=dev).fit(Xtr, labels)
    cclf = cat.CatBoostClassifier(iterations=5, depth=3, learning_rate=0.1, device=dev).fit(Xtr, labels)
    for trees, whole in ((xclf.booster_, xclf.decision_function(Xte)), (cclf.model_, cclf.predict(Xte, prediction_type="RawFormulaVal"))):
        staged = trees.staged_predict_device(Xte, period=2).cpu().numpy()
        assert staged.shape == (3, len(Xte)) and np.array_equal(S.bits(staged[-1]), S.bits(np.asarray(whole)))
        assert np.array_equal(S.bits(staged[0]), S.bits(trees.truncated(0, 2).predict(Xte)))
