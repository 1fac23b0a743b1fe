"""CPU: ``bbbp_amd.cat``'s algorithm as ``tests/cat_numpy.py`` restates it -- the border rule, the scores against exact rational
arithmetic, the invariants of a fit, the JSON round trip -- and the host API of ``cat.CatBoostRegressor``: refusals by name, aliases,
``sklearn.base.clone`` and the limits.  No GPU."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_numpy as cn  # noqa: E402
import xgb_numpy as xn  # noqa: E402
from bbbp_amd import boosters, cat  # noqa: E402


def data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, d)), 1).astype(np.float32)
    y = 1.5 * X[:, 0] + np.sin(3 * X[:, 1 % d]) + 0.1 * rng.normal(size=n)
    return X, y


# ---- the border rule ---------------------------------------------------------------------------------------------------------------------
def border_columns():
    rng = np.random.default_rng(17)
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    tiny = np.float32(1e-45)
    yield "adjacent floats", np.array([one, up, np.nextafter(up, np.float32(2.0)), one, up], np.float32)
    yield "signed zeros", np.array([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0, tiny, -tiny], np.float32)
    yield "the smallest and the largest", np.array([np.finfo(np.float32).min, np.finfo(np.float32).max, 0.0, tiny], np.float32)
    yield "duplicates", rng.integers(0, 7, size=200).astype(np.float32) / 3
    yield "two values", np.array([2.5, 2.5, -1.0, 2.5], np.float32)
    yield "more than 255 distinct values", rng.normal(size=1000).astype(np.float32)
    yield "more than 255 adjacent floats", (np.float32(3.0) + np.arange(700, dtype=np.float32) * np.spacing(np.float32(3.0)))[rng.permutation(700)]


@pytest.mark.parametrize("border_count", [254, 15, 1])
def test_border_rule(border_count):
    """For every value of the training column ``x > border`` iff ``bin(x) > c``, and the package's torch form gives cat_numpy's bits."""
    for what, col in border_columns():
        cuts = xn.cuts(col, border_count + 1)
        assert 1 <= len(cuts) <= border_count, what
        b = xn.bins(col, cuts).astype(np.int64)
        borders = np.array([cn.border(col, c) for c in cuts], np.float32)
        assert borders.dtype == np.float32
        for c in range(len(cuts)):
            assert np.array_equal(col > borders[c], b > c), f"{what}: cut {c} = {cuts[c]!r}, border {borders[c]!r}"
        got = cat.borders_of(torch.from_numpy(np.tile(col, (len(cuts), 1))), torch.from_numpy(cuts)).numpy()
        assert np.array_equal(got.view(np.int32), borders.view(np.int32)), what


# ---- the score against exact arithmetic ---------------------------------------------------------------------------------------------------
# A candidate's float64 score against its exact value, u = 2^-53, on problems of at most 3 levels (so at most 4 parts, 8 sides, when the
# last split is chosen) and |Q| < 2^53 (12 rows of |q| <= 2^48: (double)Q is exact).  A side's num term S (S / (m + lambda)) takes three
# roundings (the sum, the quotient, the product): 3u.  Its den term ((alpha alpha) m) takes two per alpha, one for the square and one for the
# product: 6u.  All terms are >= 0, so adding 8 of them one after the other costs at most 7u more: num within 10u, den within 13u.
# score = (num num) / den: 2 * 10u + 13u + 2u = 35u.  The fit picks the largest float score, so the chosen candidate's exact score is at
# least (1 - 35u) / (1 + 35u) >= 1 - 70u - O(u^2) of the exact maximum; 72u covers the second-order terms.
SCORE_BOUND = Fraction(72, 2 ** 53)


def exact_scores(right, q, parts, k, lam):
    lam = Fraction(lam)
    out = []
    for r in right:
        num = den = Fraction(0)
        for rows in parts:
            for side in (rows[~r[rows]], rows[r[rows]]):
                if len(side):
                    S = Fraction(int(q[side].sum())) / Fraction(2) ** k
                    alpha = S / (len(side) + lam)
                    num += alpha * S
                    den += alpha * alpha * len(side)
        out.append(num * num / den if den > 0 else Fraction(0))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_chosen_splits_have_the_exact_maximum_score(seed):
    rng = np.random.default_rng(100 + seed)
    n, d, depth = int(rng.integers(4, 13)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
    lam = (0.0, 3.0, 0.5)[seed % 3]
    X = rng.integers(0, 4, size=(n, d)).astype(np.float32)
    X[0, :] = 0; X[1, :] = 1                                          # every column is live
    y = rng.normal(size=n)
    T = 3
    model = cn.fit(X, y, iterations=T, depth=depth, learning_rate=0.5, l2_leaf_reg=lam)
    live, cc, B = xn.quantise(X, 255)
    cand = [(j, c) for j in range(len(live)) for c in range(len(cc[j]))]
    right = np.array([B[j].astype(np.int64) > c for j, c in cand])
    s, checked = np.zeros(n), 0
    for t in range(T):
        k, q = cn.quantise_gradients(y - (s + model["bias"]))
        assert np.abs(q).max() <= 2 ** 48
        parts, leaf_of, used = [np.arange(n)], np.zeros(n, np.int64), set()
        lo, hi = model["tree_first_split"][t], model["tree_first_split"][t + 1]
        assert hi - lo == min(depth, len(cand))
        for level, j in enumerate(range(lo, hi)):
            chosen = cand.index((int(np.searchsorted(live, model["split_feature"][j])), int(model["split_bin"][j])))
            assert chosen not in used
            exact = exact_scores(right, q, parts, k, lam)
            best = max(e for i, e in enumerate(exact) if i not in used)
            assert exact[chosen] >= best * (1 - SCORE_BOUND), f"tree {t} level {level}: {float(exact[chosen])!r} < {float(best)!r}"
            used.add(chosen); checked += 1
            parts = [side for rows in parts for side in (rows[~right[chosen][rows]], rows[right[chosen][rows]]) if len(side)]
            leaf_of |= right[chosen].astype(np.int64) << level
        s = s + model["leaf_values"][model["tree_first_leaf"][t] + leaf_of]
    assert checked >= T and np.array_equal(s + model["bias"], model["train_approx"])


# ---- invariants ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learning_rate, lam", [(0.3, 3.0), (1.0, 0.0), (1.0, 3.0)])
def test_invariants(learning_rate, lam):
    X, y = data(90, 5, seed=1)
    T, depth = 6, 4
    models = [cn.fit(X, y, iterations=t, depth=depth, learning_rate=learning_rate, l2_leaf_reg=lam) for t in range(1, T + 1)]
    full = models[-1]
    fs, fl = full["tree_first_split"], np.concatenate([full["tree_first_leaf"], [len(full["leaf_values"])]])
    for t in range(T):
        w, v = full["leaf_weights"][fl[t]:fl[t + 1]], full["leaf_values"][fl[t]:fl[t + 1]]
        assert w.sum() == len(X) and len(w) == 1 << (fs[t + 1] - fs[t])
        assert np.all(v[w == 0] == 0.0) and not np.signbit(v[w == 0]).any()
        pairs = list(zip(full["split_feature"][fs[t]:fs[t + 1]], full["split_bin"][fs[t]:fs[t + 1]]))
        assert len(set(pairs)) == len(pairs) == depth
    rmse = [np.sqrt(np.mean((y - np.mean(y)) ** 2))] + [np.sqrt(np.mean((y - m["train_approx"]) ** 2)) for m in models]
    assert all(b <= a for a, b in zip(rmse, rmse[1:])), rmse
    assert rmse[-1] < 0.8 * rmse[0]
    for m in models:                                                  # predict sums as the fit sums; a shorter model is a prefix
        assert np.array_equal(cn.predict(m, X).view(np.int64), m["train_approx"].view(np.int64))
        ns, nl = len(m["split_feature"]), len(m["leaf_values"])
        assert np.array_equal(m["split_feature"], full["split_feature"][:ns]) and np.array_equal(m["split_bin"], full["split_bin"][:ns])
        assert np.array_equal(m["split_border"].view(np.int32), full["split_border"][:ns].view(np.int32))
        assert np.array_equal(m["leaf_values"].view(np.int64), full["leaf_values"][:nl].view(np.int64)) and m["bias"] == full["bias"]


def test_constant_columns_are_dropped_and_all_constant_is_refused():
    X, y = data(40, 3, seed=2)
    wide = np.zeros((40, 7), np.float32)
    wide[:, [1, 4, 6]] = X
    wide[:, 2] = 5.0
    m, ref = cn.fit(wide, y, iterations=3, depth=3), cn.fit(X, y, iterations=3, depth=3)
    assert np.array_equal(m["split_feature"], np.array([1, 4, 6])[ref["split_feature"]]) and set(m["split_feature"]) <= {1, 4, 6}
    assert np.array_equal(m["leaf_values"].view(np.int64), ref["leaf_values"].view(np.int64))
    with pytest.raises(ValueError, match="all features are constant"):
        cn.fit(np.ones((10, 3), np.float32), np.arange(10.0), iterations=1)


# ---- JSON ---------------------------------------------------------------------------------------------------------------------------------
def test_model_json_round_trip(tmp_path):
    X, y = data(60, 4, seed=3)
    m = cn.fit(X, y, iterations=4, depth=3, learning_rate=0.2)
    keys = ("split_feature", "split_border", "split_bin", "tree_first_split", "tree_first_leaf", "leaf_values", "leaf_weights")
    reg = cat.CatBoostRegressor.from_trees({k: m[k] for k in keys}, m["bias"], X.shape[1], device="cpu", iterations=4, depth=3, learning_rate=0.2)
    assert reg.tree_count_ == 4 and reg.n_features_in_ == 4
    path = tmp_path / "cat.json"
    reg.save_model(str(path), format="json")
    text = path.read_text()
    assert text == reg.get_model_json()
    with pytest.raises(ValueError, match="json"):
        reg.save_model(str(path), format="cbm")
    doc = json.loads(text)
    assert set(doc) >= {"oblivious_trees", "features_info", "scale_and_bias"} and doc["scale_and_bias"] == [1.0, [m["bias"]]]
    assert len(doc["features_info"]["float_features"]) == 4 and len(doc["oblivious_trees"]) == 4
    tree = doc["oblivious_trees"][1]
    assert set(tree) == {"splits", "leaf_values", "leaf_weights"} and set(tree["splits"][0]) >= {"float_feature_index", "border", "split_type"}
    assert tree["splits"][0]["split_type"] == "FloatFeature" and sum(tree["leaf_weights"]) == 60
    flat = boosters.CatBoostTrees.flatten(doc)
    for got, key in zip(flat[:2] + flat[3:6], ("split_feature", "split_border", "tree_first_split", "tree_first_leaf", "leaf_values")):
        assert got.dtype == reg.model_.arrays[key].dtype and np.array_equal(got.view(np.uint8), reg.model_.arrays[key].view(np.uint8)), key
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(m[key]).view(np.uint8)), key
    assert not flat[2].any() and flat[6:] == (4, 1.0, float(m["bias"]))
    back = boosters.CatBoostTrees.from_json(text, device="cpu")
    assert back.n_trees == 4 and back.bias == float(m["bias"]) and back.scale == 1.0
    with pytest.raises(RuntimeError, match="needs a GPU"):
        reg.predict(X)


# ---- the host API -------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    R = cat.CatBoostRegressor
    for kw, name in [(dict(loss_function="MAE"), "loss_function"), (dict(objective="Quantile"), "objective"), (dict(boosting_type="Ordered"), "boosting_type"),
                     (dict(bootstrap_type="MVS"), "bootstrap_type"), (dict(bootstrap_type="Bayesian"), "bootstrap_type"), (dict(random_strength=1), "random_strength"),
                     (dict(subsample=0.8), "subsample"), (dict(bagging_temperature=1), "bagging_temperature"), (dict(rsm=0.5), "rsm"),
                     (dict(colsample_bylevel=0.5), "colsample_bylevel"), (dict(grow_policy="Depthwise"), "grow_policy"),
                     (dict(grow_policy="Lossguide"), "grow_policy"), (dict(min_data_in_leaf=2), "min_data_in_leaf"),
                     (dict(leaf_estimation_iterations=5), "leaf_estimation_iterations"), (dict(score_function="L2"), "score_function"),
                     (dict(score_function="NewtonCosine"), "score_function"), (dict(cat_features=[0]), "cat_features"), (dict(text_features=[1]), "text_features"),
                     (dict(early_stopping_rounds=5), "early_stopping_rounds"), (dict(od_type="Iter"), "od_type"), (dict(use_best_model=True), "use_best_model"),
                     (dict(monotone_constraints=[1]), "monotone_constraints"), (dict(nan_mode="Min"), "nan_mode"), (dict(langevin=True), "langevin"),
                     (dict(depth=0), "depth"), (dict(depth=17), "depth"), (dict(max_depth=17), "depth"), (dict(depth=None), "depth"),
                     (dict(iterations=10001), "10000 trees"), (dict(iterations=0), "iterations"), (dict(n_estimators=0), "iterations"),
                     (dict(border_count=256), "border_count"), (dict(border_count=0), "border_count"), (dict(learning_rate=0), "learning_rate"),
                     (dict(learning_rate=float("nan")), "learning_rate"), (dict(l2_leaf_reg=-1), "l2_leaf_reg"), (dict(reg_lambda=float("inf")), "l2_leaf_reg"),
                     (dict(random_seed="x"), "random_seed"), (dict(device=["cuda:0", "cuda:1"]), "more than one GPU"),
                     (dict(iterations=5, n_estimators=7), "alias"), (dict(colsample=1), "unknown parameter colsample")]:
        with pytest.raises(ValueError, match=name):
            R(**kw)
    R(loss_function="RMSE", boosting_type="Plain", bootstrap_type="No", random_strength=0, rsm=1, grow_policy="SymmetricTree", min_data_in_leaf=1,
      leaf_estimation_iterations=1, score_function="Cosine", subsample=None, cat_features=None, thread_count=4, task_type="GPU", random_state=42,
      verbose=0)                                                      # the neutral values pass
    R(iterations=300, learning_rate=0.01, depth=10, verbose=0, random_state=42)            # the reference's regressor builds as written
    X, y = data(20, 4, seed=4)
    reg = R()
    for kw, name in [(dict(sample_weight=np.ones(20)), "sample_weight"), (dict(eval_set=[(X, y)]), "eval_set"), (dict(early_stopping_rounds=3), "early stopping"),
                     (dict(cat_features=[0]), "categorical"), (dict(text_features=[0]), "text"), (dict(baseline=y), "baseline")]:
        with pytest.raises(ValueError, match=name):
            reg.fit(X, y, **kw)
    with pytest.raises(ValueError, match="8192"):
        reg.fit(np.zeros((8193, 2), np.float32), np.zeros(8193))
    with pytest.raises(ValueError, match="live features"):
        reg.fit(np.arange(2 * 65537, dtype=np.float32).reshape(2, 65537), np.zeros(2))
    with pytest.raises(ValueError, match="at least two rows"):
        reg.fit(X[:1], y[:1])
    bad = X.copy(); bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        reg.fit(bad, y)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        reg.fit(bad, y)
    with pytest.raises(ValueError, match="NaN or infinity"):
        reg.fit(X, np.where(np.arange(20) == 2, np.nan, y))
    with pytest.raises(ValueError, match="one output"):
        reg.fit(X, np.stack([y, y], axis=1))
    with pytest.raises(ValueError, match="all features are constant"):
        reg.fit(np.ones((20, 3), np.float32), y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R(device="cpu").fit(X, y)
    with pytest.raises(RuntimeError, match="not fitted"):
        reg.predict(X)
    with pytest.raises(ValueError, match="no problems"):
        cat.fit_regressors([])


def test_params_clone_and_aliases():
    from sklearn.base import clone
    reg = cat.CatBoostRegressor(n_estimators=7, max_depth=3, reg_lambda=2.0, random_state=42, learning_rate=0.01, verbose=0)
    assert (reg.iterations, reg.depth, reg.l2_leaf_reg, reg.random_seed, reg.learning_rate, reg.verbose) == (7, 3, 2.0, 42, 0.01, 0)
    twin = clone(reg)
    assert twin is not reg and twin.get_params() == reg.get_params()
    assert reg.set_params(max_depth=5, learning_rate=None) is reg and (reg.depth, reg.learning_rate) == (5, None)
    with pytest.raises(ValueError, match="depth"):
        reg.set_params(depth=0)
    assert reg.depth == 5
    with pytest.raises(ValueError, match="unknown"):
        reg.set_params(gamma=3)
    assert cat.CatBoostRegressor().get_params() == dict(iterations=1000, learning_rate=None, depth=6, l2_leaf_reg=3.0, border_count=254, random_seed=None,
                                                        verbose=None, device="cuda")
    assert cat.DEFAULT_LEARNING_RATE == 0.03 and (cat.MAX_ROWS, cat.MAX_LIVE_FEATURES, cat.MAX_DEPTH, cat.MAX_TREES) == (8192, 65536, 16, 10000)


def test_kernel_entry_points_validate_before_touching_the_gpu():
    import ctypes
    from bbbp_amd import _lib
    L = _lib.lib()
    assert L.bbbp_cat_fit_work_bytes(1058, 49319, 10) > 0 and L.bbbp_cat_fit_work_bytes(8192, 65536, 16) > L.bbbp_cat_fit_work_bytes(8192, 65536, 1)
    for args in ((1, 4, 3), (8193, 4, 3), (10, 0, 3), (10, 65537, 3), (10, 4, 0), (10, 4, 17)):
        assert L.bbbp_cat_fit_work_bytes(*args) == 0 and b"cat_fit_work_bytes" in L.bbbp_last_error()
    fake = 4096                                                       # never dereferenced: validation comes first
    good = dict(bins=fake, n_cuts=fake, y=fake, n=10, d=3, iterations=2, depth=3, l2_leaf_reg=3.0, learning_rate=0.03, bias=0.0, work=fake,
                split_feature=fake, split_bin=fake, leaf_values=fake, leaf_weights=fake, tree_depth=fake, approx=fake)
    for change, word in [(dict(n=1), b"n 1"), (dict(n=8193), b"n 8193"), (dict(d=0), b"d 0"), (dict(iterations=0), b"iterations"), (dict(iterations=10001), b"iterations"),
                         (dict(depth=17), b"depth"), (dict(depth=0), b"depth"), (dict(l2_leaf_reg=-1.0), b"l2_leaf_reg"), (dict(learning_rate=0.0), b"learning_rate"),
                         (dict(bias=float("nan")), b"bias"), (dict(work=None), b"null pointer"), (dict(approx=None), b"null pointer")]:
        arr = (_lib.CatProblem * 1)(_lib.CatProblem(**{**good, **change}))
        assert L.bbbp_cat_fit(None, arr, ctypes.c_void_p(fake), 1) == 1 and word in L.bbbp_last_error(), change
    arr = (_lib.CatProblem * 1)(_lib.CatProblem(**good))
    assert L.bbbp_cat_fit(None, arr, None, 1) == 1 and L.bbbp_cat_fit(None, arr, ctypes.c_void_p(fake), 0) == 1
    assert L.bbbp_cat_fit_last(None, None) == 1
    prev = L.bbbp_cat_fit_profile(1)
    assert L.bbbp_cat_fit_profile(prev) == 1
