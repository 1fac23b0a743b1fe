"""``bbbp_amd.cat`` on the GPU against its numpy restatement (``tests/cat_numpy.py``), bit for bit: splits, borders, leaf values, leaf
weights, the bias and the training approximations; then the edge cases, prediction, batch invariance and the stack.

The shapes are the smallest at which the kernels can go wrong: two rows whose candidates run out (shallow trees), 256 leaves for 40 rows
(mostly empty parts), parts on either side of the 64-row boundary between the lane-against-lane form and the histogram form (64 and 65
rows at the root, both forms inside one tree), features of at most 64 cuts (one cut per lane) and of more (four per lane), the quantile
rule (more distinct values than bins), one border per feature, and more feature blocks than one with dropped constant columns."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_numpy as cn  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("split_feature", "split_border", "split_bin", "tree_first_split", "tree_first_leaf", "leaf_values", "leaf_weights")


def data(n, d, seed):
    """Features rounded to two decimals (duplicates and ties on purpose), a target that needs several columns."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, d)), 2).astype(np.float32)
    y = 1.5 * X[:, 0] + np.sin(3 * X[:, 1 % d]) + 0.3 * X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    return X, y


def mixed_data(n=1058, seed=11):
    """``tests/test_gpu_xgb.py``'s recipe: 120 binary columns, 60 constant ones and 120 of 5-40 distinct values, interleaved: many
    live-feature blocks, remapped indices, ties."""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(300):
        kind = j % 5
        if kind in (0, 1):
            cols.append((rng.random(n) < 0.3).astype(np.float32))
        elif kind == 2:
            cols.append(np.full(n, np.float32(j % 7)))
        else:
            cols.append(rng.integers(0, 5 + (j * 7) % 36, size=n).astype(np.float32) / 4)
    X = np.stack(cols, axis=1)
    y = X[:, 0] - X[:, 5] + 0.5 * X[:, 3] * X[:, 8] + 0.2 * X[:, 13] + 0.1 * rng.normal(size=n)
    return X, y


# name: (n, d, trees, depth, border_count, learning_rate)
CASES = {
    "n2": (2, 1, 3, 3, 254, 0.3), "n3": (3, 5, 4, 4, 254, 0.3), "n40": (40, 12, 4, 8, 254, 0.3), "n64": (64, 7, 4, 6, 254, 0.1),
    "n65": (65, 7, 4, 6, 254, 0.1), "n300": (300, 20, 4, 6, 254, 0.3), "n257_border15": (257, 9, 3, 5, 15, 0.3),
    "n600_border1": (600, 4, 3, 4, 1, 0.3), "n1058_mixed": (1058, 300, 2, 10, 254, 0.01),
}


@functools.lru_cache(maxsize=None)
def case(name):
    n, d, T, depth, border_count, eta = CASES[name]
    X, y = mixed_data(n) if name == "n1058_mixed" else data(n, d, seed=n + d)
    params = dict(iterations=T, depth=depth, border_count=border_count, learning_rate=eta)
    return X, y, params, cn.fit(X, y, **params)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a


def reference_of(reg):
    return {**reg.trees_, "bias": reg.bias_, "train_approx": reg.train_approx_}


def assert_same_model(reg, ref, what=""):
    for key in KEYS:
        got, want = np.asarray(reg.trees_[key]), np.asarray(ref[key])
        assert got.shape == want.shape, f"{what}{key}: shape {got.shape}, the restatement has {want.shape}"
        assert got.dtype == want.dtype, f"{what}{key}: dtype {got.dtype} != {want.dtype}"
        assert np.array_equal(bits(got), bits(want)), f"{what}{key}: first difference at {int(np.flatnonzero(bits(got) != bits(want))[0])}"
    assert np.float64(reg.bias_).tobytes() == np.float64(ref["bias"]).tobytes(), f"{what}bias"
    assert reg.train_approx_.dtype == np.float64 and np.array_equal(bits(reg.train_approx_), bits(ref["train_approx"])), f"{what}train_approx_"
    m = reg.model_.arrays
    assert np.array_equal(m["split_feature"], ref["split_feature"]) and np.array_equal(bits(m["split_border"]), bits(ref["split_border"]))
    assert np.array_equal(bits(m["leaf_values"]), bits(ref["leaf_values"])) and reg.model_.scale == 1.0 and not m["nan_true"].any()


def fit(dev, X, y, **params):
    from bbbp_amd import cat
    return cat.CatBoostRegressor(device=dev, **params).fit(X, y)


@pytest.mark.parametrize("name", list(CASES))
def test_fit_equals_the_restatement_bit_for_bit(dev, name):
    X, y, params, ref = case(name)
    reg = fit(dev, X, y, **params)
    assert_same_model(reg, ref)
    assert reg.n_features_in_ == X.shape[1] and reg.tree_count_ == params["iterations"]
    levels = np.diff(ref["tree_first_split"])
    if name == "n2":                          # one candidate: every tree has one level
        assert np.array_equal(levels, [1, 1, 1])
    else:
        assert np.all(levels == params["depth"])
    if name == "n40":                         # 256 leaves for 40 rows
        assert (ref["leaf_weights"] == 0).sum() >= 4 * (256 - 40)
    if name == "n300":                        # both forms in one tree: at some level a part of more than 64 rows and one of at most 64
        w = ref["leaf_weights"][:1 << levels[0]]
        parts = [np.bincount(np.arange(len(w)) & ((1 << lv) - 1), weights=w) for lv in range(1, levels[0])]       # bit i is split i
        assert any((p > 64).any() and ((p > 0) & (p <= 64)).any() for p in parts)
    if name == "n1058_mixed":                 # constant columns never split, features keep their original indices
        used = np.unique(ref["split_feature"])
        assert not np.isin(used % 5, [2]).any() and len(used) > 1


def variant_data():
    return data(120, 6, seed=3)


def test_constant_y_gives_leaves_of_zero(dev):
    X, _ = variant_data()
    y = np.full(len(X), 0.75)
    reg = fit(dev, X, y, iterations=3, depth=4)
    assert_same_model(reg, cn.fit(X, y, iterations=3, depth=4))
    assert np.all(reg.trees_["leaf_values"] == 0) and np.all(reg.predict(X) == 0.75) and reg.bias_ == 0.75
    assert np.array_equal(reg.trees_["split_feature"][:4], [0, 0, 0, 0]) and np.array_equal(reg.trees_["split_bin"][:4], [0, 1, 2, 3])


def test_all_columns_constant_is_refused(dev):
    X = np.tile(np.float32([1.0, -2.0, 0.5]), (30, 1))
    y = np.linspace(-1, 1, 30)
    with pytest.raises(ValueError, match="all features are constant"):
        fit(dev, X, y, iterations=2)
    with pytest.raises(ValueError, match="all features are constant"):
        fit(dev, torch.from_numpy(X).to(dev), y, iterations=2)
    from bbbp_amd import cat
    X2 = X.copy(); X2[-1, 0] = 7.0            # live over all rows, constant over the fold's
    with pytest.raises(ValueError, match="all features are constant"):
        cat.fit_regressors([(X2, y, np.arange(29))], iterations=2, device=dev)


def test_duplicated_rows(dev):
    X, y = variant_data()
    X, y = np.concatenate([X, X[:50], X[:50]]), np.concatenate([y, y[:50], y[:50] + 0.5])
    assert_same_model(fit(dev, X, y, iterations=4, depth=7), cn.fit(X, y, iterations=4, depth=7))


def test_l2_leaf_reg_zero_and_aliases(dev):
    X, y = variant_data()
    assert_same_model(fit(dev, X, y, iterations=4, l2_leaf_reg=0), cn.fit(X, y, iterations=4, l2_leaf_reg=0), what="l2_leaf_reg=0: ")
    reg = fit(dev, X, y, n_estimators=3, max_depth=5, reg_lambda=0.5, random_state=42, verbose=0)
    assert_same_model(reg, cn.fit(X, y, iterations=3, depth=5, l2_leaf_reg=0.5), what="aliases, default learning rate: ")


def test_float64_input_and_a_row_strided_cuda_view(dev):
    X, y = variant_data()
    ref = cn.fit(X, y, iterations=3)
    assert_same_model(fit(dev, X.astype(np.float64), y, iterations=3), ref, what="float64: ")
    wide = torch.zeros((2 * len(X), X.shape[1] + 3), dtype=torch.float32, device=dev)
    wide[::2, :X.shape[1]] = torch.from_numpy(X).to(dev)
    view = wide[::2, :X.shape[1]]
    assert not view.is_contiguous()
    reg = fit(dev, view, y, iterations=3)
    assert_same_model(reg, ref, what="strided view: ")
    got = reg.predict(view)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), reg.predict(X))


def test_prediction(dev):
    """``predict`` sums in ``obl_sum_kernel``'s order, which is the fit's: the training rows' predictions equal ``train_approx_`` bit for
    bit, fresh rows equal ``cat_numpy.predict``; the JSON export reads back to a model that predicts the same bits."""
    from bbbp_amd import boosters
    X, y, params, ref = case("n300")
    reg = fit(dev, X, y, **params)
    got = reg.predict(X)
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(reg.train_approx_)) and np.array_equal(bits(got), bits(cn.predict(ref, X)))
    fresh = np.round(np.random.default_rng(9).normal(size=(257, X.shape[1])), 2).astype(np.float32)
    assert np.array_equal(bits(reg.predict(fresh)), bits(cn.predict(ref, fresh)))
    assert np.array_equal(bits(reg.predict_device(torch.from_numpy(fresh).to(dev)).cpu().numpy()), bits(cn.predict(ref, fresh)))
    back = boosters.CatBoostTrees.from_json(reg.get_model_json(), device=dev)
    assert np.array_equal(bits(back.predict(fresh)), bits(cn.predict(ref, fresh)))


def test_batch_invariance(dev):
    from bbbp_amd import cat
    shapes = [(2, 1, 3, 254), (40, 12, 8, 254), (65, 7, 6, 254), (130, 9, 5, 15), (300, 20, 6, 254), (64, 3, 4, 1)]
    problems = [data(n, d, seed=7 * n + d) for n, d, _, _ in shapes]
    regs = [cat.CatBoostRegressor(iterations=2 + (i % 2), depth=depth, border_count=bc, learning_rate=0.2, device=dev)
            for i, (_, _, depth, bc) in enumerate(shapes)]
    alone = [cat.CatBoostRegressor(**r.get_params()).fit(X, y) for r, (X, y) in zip(regs, problems)]
    for run in range(2):
        cat._fit(regs, problems)
        for i, (reg, one) in enumerate(zip(regs, alone)):
            assert_same_model(reg, reference_of(one), what=f"run {run} problem {i}: ")
    assert_same_model(alone[4], cn.fit(*problems[4], iterations=2, depth=6, learning_rate=0.2), what="alone vs restatement: ")


def test_folds_and_refit_in_one_batch(dev):
    from bbbp_amd import cat
    X, y = data(101, 6, seed=5)
    bounds = np.linspace(0, len(X), 6).astype(int)
    rows = [np.concatenate([np.arange(0, bounds[f]), np.arange(bounds[f + 1], len(X))]) for f in range(5)]
    params = dict(iterations=3, depth=5, learning_rate=0.1, device=dev)
    batch = cat.fit_regressors([(X, y, r) for r in rows] + [(X, y)], **params)
    for reg, r in zip(batch, rows + [np.arange(len(X))]):
        one = cat.CatBoostRegressor(**params).fit(X[r], y[r])
        assert_same_model(reg, reference_of(one), what=f"{len(r)} rows: ")
    assert_same_model(batch[0], cn.fit(X[rows[0]], y[rows[0]], iterations=3, depth=5, learning_rate=0.1), what="fold 0 vs restatement: ")


def test_stack_and_screen(dev):
    from bbbp_amd import cat, ensemble
    rng = np.random.default_rng(4)
    y = rng.normal(size=200)
    X = (y[:, None] + 0.3 * rng.normal(size=(200, 4))).astype(np.float32)             # the [N, 4] out-of-fold matrix [nn, rf, xgb, cat]
    stack = ensemble.StackingRegressor([("cat", cat.CatBoostRegressor(iterations=5, depth=3, learning_rate=0.3, device=dev))])
    out = stack.fit(X, y).predict(X)
    assert out.shape == (200,) and np.isfinite(out).all() and np.corrcoef(out, y)[0, 1] > 0.7
    reg = stack.estimators_[0][1]
    assert_same_model(reg, cn.fit(X, y, iterations=5, depth=3, learning_rate=0.3), what="the stack's full fit: ")

    class Net(torch.nn.Module):
        def forward(self, fp, im):
            return fp.sum(dim=1) + im.sum(dim=1)

    Xd = torch.from_numpy(X).to(dev)
    meta = ensemble.StackedEnsemble.from_coefficients([0.0, 1.0], 0.0)
    got = ensemble.screen(Net(), None, meta, Xd[:, :2], Xd[:, 2:], boosters=[reg.model_])
    assert np.array_equal(got.cpu().numpy(), reg.predict(X))
