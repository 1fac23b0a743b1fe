"""``bbbp_amd.xgb`` on the GPU against its numpy restatement (``tests/xgb_numpy.py``), bit for bit: every node array, every recorded
statistic, the training margins and the base score; then the variants, prediction, batch invariance and the stack.

The shapes are the smallest at which the kernels can go wrong: the smallest problem, nodes on either side of the 64-row boundary between the
lane-against-lane form and the histogram form (64 and 65 rows at the root, both forms inside one deep tree), more feature blocks than one,
dropped constant columns (index remapping), binary columns (ties between features), the quantile rule (more distinct values than bins)
and max_bin = 2."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xgb_numpy as xn  # noqa: E402
from oracle import reference_cpu as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

STATS = ("base_weights", "loss_changes", "sum_hessian")
KEYS = ("left", "right", "feature", "root", "parents", "default_left", "cond") + STATS


def data(n, d, seed):
    """Features rounded to two decimals (duplicates and ties on purpose), a target that needs several columns."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(size=(n, d)), 2).astype(np.float32)
    y = 1.5 * X[:, 0] + np.sin(3 * X[:, 1 % d]) + 0.3 * X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    return X, y


def mixed_data(n=1058, seed=11):
    """120 binary columns, 60 constant ones and 120 of 5-40 distinct values, interleaved: many live-feature blocks, remapped indices, ties."""
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


CASES = {
    "n2": (2, 1, 3, 1, 256, 0.3), "n3": (3, 5, 4, 30, 256, 0.3), "n40": (40, 12, 8, 6, 256, 0.3), "n64": (64, 7, 6, 30, 256, 0.1),
    "n65": (65, 7, 6, 30, 256, 0.1), "n300": (300, 20, 6, 30, 256, 0.3), "n257_bin16": (257, 9, 5, 5, 16, 0.3), "n600_bin2": (600, 4, 4, 8, 2, 0.3),
    "n1058_mixed": (1058, 300, 3, 30, 256, 0.01),
}


@functools.lru_cache(maxsize=None)
def case(name):
    n, d, T, depth, max_bin, eta = CASES[name]
    X, y = mixed_data(n) if name == "n1058_mixed" else data(n, d, seed=n + d)
    params = dict(n_estimators=T, max_depth=depth, max_bin=max_bin, learning_rate=eta)
    return X, y, params, xn.fit(X, y, **params)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_model(reg, ref, what=""):
    for key in KEYS:
        got, want = np.asarray(reg.trees_[key]), np.asarray(ref[key])
        assert got.shape == want.shape, f"{what}{key}: {got.shape} nodes, the restatement has {want.shape}"
        assert got.dtype == want.dtype, f"{what}{key}: dtype {got.dtype} != {want.dtype}"
        assert np.array_equal(bits(got), bits(want)), f"{what}{key}: first difference at node {int(np.flatnonzero(bits(got) != bits(want))[0])}"
    assert np.float32(reg.base_score_).tobytes() == np.float32(ref["base_score"]).tobytes(), f"{what}base_score"
    assert reg.train_margin_.dtype == np.float32 and np.array_equal(bits(reg.train_margin_), bits(ref["train_margin"])), f"{what}train_margin_"


def fit(dev, X, y, **params):
    from bbbp_amd import xgb
    return xgb.XGBRegressor(device=dev, **params).fit(X, y)


@pytest.mark.parametrize("name", list(CASES))
def test_fit_equals_the_restatement_bit_for_bit(dev, name):
    X, y, params, ref = case(name)
    reg = fit(dev, X, y, **params)
    assert_same_model(reg, ref)
    assert reg.n_features_in_ == X.shape[1]
    if name == "n300":                        # both forms in one tree, and trees that grow until rows are alone
        sizes = ref["sum_hessian"][ref["left"] >= 0]
        assert (sizes > 64).any() and (sizes <= 64).any() and (ref["sum_hessian"][ref["left"] < 0] == 1).any()
    if name == "n1058_mixed":                 # constant columns never split, features keep their original indices
        used = np.unique(ref["feature"][ref["left"] >= 0])
        assert not np.isin(used % 5, [2]).any() and used.max() > 240


def variant_data():
    return data(120, 6, seed=3)


def test_constant_y_gives_single_leaves_of_weight_zero(dev):
    X, _ = variant_data()
    y = np.full(len(X), 0.75)
    reg = fit(dev, X, y, n_estimators=3)
    assert_same_model(reg, xn.fit(X, y, n_estimators=3))
    assert np.array_equal(reg.trees_["root"], [0, 1, 2, 3]) and np.all(reg.trees_["cond"] == 0)
    assert np.all(reg.predict(X) == reg.base_score_) and reg.base_score_ == np.float32(0.75)


def test_all_columns_constant(dev):
    X = np.tile(np.float32([1.0, -2.0, 0.5]), (30, 1))
    y = np.linspace(-1, 1, 30)
    reg = fit(dev, X, y, n_estimators=2)
    assert_same_model(reg, xn.fit(X, y, n_estimators=2))
    assert np.array_equal(reg.trees_["root"], [0, 1, 2])


def test_duplicated_rows(dev):
    X, y = variant_data()
    X, y = np.concatenate([X, X[:50], X[:50]]), np.concatenate([y, y[:50], y[:50] + 0.5])
    assert_same_model(fit(dev, X, y, n_estimators=4, max_depth=30), xn.fit(X, y, n_estimators=4, max_depth=30))


def test_one_column_that_alone_separates_y(dev):
    X, _ = variant_data()
    y = np.where(X[:, 4] > 0.1, 2.0, -1.0)
    reg = fit(dev, X, y, n_estimators=3, max_depth=3)
    assert_same_model(reg, xn.fit(X, y, n_estimators=3, max_depth=3))
    assert reg.trees_["feature"][0] == 4 and np.all(X[:, 4][X[:, 4] > 0.1] >= reg.trees_["cond"][0])


def test_gamma_and_min_child_weight_split_less(dev):
    X, y = variant_data()
    plain = fit(dev, X, y, n_estimators=4)
    for extra in (dict(gamma=0.5), dict(min_child_weight=5), dict(min_split_loss=0.5, min_child_weight=4.5)):
        reg = fit(dev, X, y, n_estimators=4, **extra)
        kw = {("gamma" if k == "min_split_loss" else k): v for k, v in extra.items()}
        assert_same_model(reg, xn.fit(X, y, n_estimators=4, **kw), what=f"{extra}: ")
        assert len(reg.trees_["left"]) < len(plain.trees_["left"])
    assert fit(dev, X, y, n_estimators=4, min_child_weight=5).trees_["sum_hessian"].min() >= 5


def test_reg_lambda_zero_and_user_base_score(dev):
    X, y = variant_data()
    for extra in (dict(reg_lambda=0), dict(base_score=0.25), dict(**{"lambda": 3.5}, eta=0.05)):
        kw = {{"lambda": "reg_lambda", "eta": "learning_rate"}.get(k, k): v for k, v in extra.items()}
        assert_same_model(fit(dev, X, y, n_estimators=4, **extra), xn.fit(X, y, n_estimators=4, **kw), what=f"{extra}: ")
    assert fit(dev, X, y, n_estimators=1, base_score=0.25).base_score_ == np.float32(0.25)


def test_float64_input_and_a_row_strided_cuda_view(dev):
    X, y = variant_data()
    ref = xn.fit(X, y, n_estimators=3)
    assert_same_model(fit(dev, X.astype(np.float64), y, n_estimators=3), ref, what="float64: ")
    wide = torch.zeros((2 * len(X), X.shape[1] + 3), dtype=torch.float32, device=dev)
    wide[::2, :X.shape[1]] = torch.from_numpy(X).to(dev)
    view = wide[::2, :X.shape[1]]
    assert not view.is_contiguous()
    reg = fit(dev, view, y, n_estimators=3)
    assert_same_model(reg, ref, what="strided view: ")
    got = reg.predict(view)
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), reg.predict(X))


def test_prediction(dev):
    """``bbbp_gbt_predict`` adds the trees in ascending order and then ``base_score`` (csrc/forest.hip: gbt_sum_kernel), the fit adds
    ``base_score`` first: the training rows' predictions equal ``train_margin_`` within T float32 ulps of the largest partial sum, not bit
    for bit.  On fresh rows ``predict`` equals ``oracle.xgb_predict`` on ``trees_``, which sums in the kernel's order."""
    X, y, params, ref = case("n300")
    reg = fit(dev, X, y, **params)
    T = params["n_estimators"]
    got = reg.predict(X)
    bound = T * np.spacing(np.float32(np.abs(ref["train_margin"]).max() + np.abs(ref["base_score"])))
    err = np.abs(got.astype(np.float64) - reg.train_margin_.astype(np.float64)).max()
    print(f"predict(X_train) vs train_margin_: max difference {err:.3e}, bound {bound:.3e}")
    assert got.dtype == np.float32 and err <= bound
    fresh = np.round(np.random.default_rng(9).normal(size=(257, X.shape[1])), 2).astype(np.float32)
    t = reg.trees_
    want = oracle.xgb_predict(t["left"], t["right"], t["feature"], t["cond"], t["default_left"], t["root"], reg.base_score_, fresh)
    assert np.array_equal(bits(reg.predict(fresh)), bits(want))
    assert np.array_equal(bits(xn.predict(ref, X)), bits(ref["train_margin"]))


def test_batch_invariance(dev):
    from bbbp_amd import xgb
    shapes = [(2, 1, 1, 256), (40, 12, 6, 256), (65, 7, 30, 256), (130, 9, 5, 16), (300, 20, 30, 256), (64, 3, 8, 2)]
    problems = [data(n, d, seed=7 * n + d) for n, d, _, _ in shapes]
    regs = [xgb.XGBRegressor(n_estimators=3, max_depth=depth, max_bin=mb, device=dev) for _, _, depth, mb in shapes]
    alone = [xgb.XGBRegressor(**r.get_params()).fit(X, y) for r, (X, y) in zip(regs, problems)]
    for run in range(2):
        xgb._fit(regs, problems)
        for i, (reg, one) in enumerate(zip(regs, alone)):
            assert_same_model(reg, {**one.trees_, "base_score": one.base_score_, "train_margin": one.train_margin_}, what=f"run {run} problem {i}: ")
    assert_same_model(alone[4], xn.fit(*problems[4], n_estimators=3, max_depth=30), what="alone vs restatement: ")


def test_folds_and_refit_in_one_batch(dev):
    from bbbp_amd import xgb
    X, y = data(101, 6, seed=5)
    bounds = np.linspace(0, len(X), 6).astype(int)
    rows = [np.concatenate([np.arange(0, bounds[f]), np.arange(bounds[f + 1], len(X))]) for f in range(5)]
    params = dict(n_estimators=3, max_depth=30, learning_rate=0.1, device=dev)
    batch = xgb.fit_regressors([(X, y, r) for r in rows] + [(X, y)], **params)
    for reg, r in zip(batch, rows + [np.arange(len(X))]):
        one = xgb.XGBRegressor(**params).fit(X[r], y[r])
        assert_same_model(reg, {**one.trees_, "base_score": one.base_score_, "train_margin": one.train_margin_}, what=f"{len(r)} rows: ")
    assert_same_model(batch[0], xn.fit(X[rows[0]], y[rows[0]], n_estimators=3, max_depth=30, learning_rate=0.1), what="fold 0 vs restatement: ")


def test_stack_and_screen(dev):
    from bbbp_amd import ensemble, random_forest, xgb
    X, y = data(60, 8, seed=2)
    stack = ensemble.StackingRegressor([("xgb", xgb.XGBRegressor(n_estimators=3, max_depth=3, device=dev)),
                                        ("rf", random_forest.RandomForestRegressor(n_estimators=3, max_depth=3, random_state=0, device=dev))])
    out = stack.fit(X, y).predict(X)
    assert out.shape == (60,) and np.isfinite(out).all() and np.corrcoef(out, y)[0, 1] > 0.5
    reg = stack.estimators_[0][1]

    class Net(torch.nn.Module):
        def forward(self, fp, im):
            return fp.sum(dim=1) + im.sum(dim=1)

    Xd = torch.from_numpy(X).to(dev)
    meta = ensemble.StackedEnsemble.from_coefficients([0.0, 1.0], 0.0)
    got = ensemble.screen(Net(), None, meta, Xd[:, :5], Xd[:, 5:], boosters=[reg.booster_])
    assert np.array_equal(got.cpu().numpy(), reg.predict(X).astype(np.float64))
