"""GPU: gradient_boosting.GradientBoostingRegressor.  Ties between split candidates are broken by a fixed rule, so a fit is certified by the
replayer (tests/gbr_replay.py) instead of being compared tree for tree; on continuous features the training rows' predictions are compared
with scikit-learn's within a derived bound; prediction from adopted scikit-learn trees is compared bit for bit; quality is measured against
scikit-learn's own scatter over random_state."""
import functools

import numpy as np
import pytest
import torch

import gbr_replay as R
from poison import FILLS, poisoned_allocations

pytestmark = pytest.mark.gpu
IDS = [f"{'-'.join(str(v) for v in c)}-{v}-{T}" for c, v, T in R.CASES]


def GBR(*a, **kw):
    from bbbp_amd.gradient_boosting import GradientBoostingRegressor
    return GradientBoostingRegressor(*a, **kw)


def _fit(dev, case, variant=None, T=8, data=None):
    n, d, depth, mss, msl, lr = case
    X, y = R.make_data(n, d, variant=variant) if data is None else data
    return X, y, GBR(T, learning_rate=lr, max_depth=depth, min_samples_split=mss, min_samples_leaf=msl, device=dev).fit(X, y)


def _certify(reg, X, y):
    stages = np.array(list(reg.staged_predict(X)))
    seen = R.replay(X, y, reg.trees_, reg.init_, reg.learning_rate, reg.max_depth, reg.min_samples_split, reg.min_samples_leaf, raw_stages=stages,
                    train_score=reg.train_score_)
    return seen, stages


@pytest.mark.parametrize("case,variant,T", R.CASES, ids=IDS)
def test_certificate(dev, case, variant, T):
    n, d = case[:2]
    X, y, reg = _fit(dev, case, variant, T)
    seen, stages = _certify(reg, X, y)
    print(case, variant, {k: v for k, v in seen.items() if k != "raw"})
    assert reg.n_estimators_ == T and len(reg.train_score_) == T and reg.n_features_in_ == d
    assert reg.init_ == float(np.average(y))                                # targets and their mean go through unrounded
    pred = reg.predict(X)
    assert pred.dtype == np.float64 and np.array_equal(reg._train_raw, stages[-1]) and np.array_equal(pred, stages[-1])
    if variant == "constant_y":
        assert len(reg.trees_["left"]) == T and not reg.trees_["value"].any() and (pred == reg.init_).all() and not reg.train_score_.any()
        return
    if variant == "flat":
        first = slice(int(reg.trees_["root"][0]), int(reg.trees_["root"][1]))
        assert (reg.trees_["left"][first][1:3] < 0).any() and seen["stop_reasons"].get("impurity", 0) >= 1
    if variant == "constant":
        assert not (reg.trees_["feature"][reg.trees_["left"] >= 0] == min(2, d - 1)).any()
    assert seen["splits"] >= T and np.all(np.diff(reg.train_score_) < 0)


@functools.lru_cache(maxsize=None)
def _sklearn_model(case, variant, T):
    from sklearn.ensemble import GradientBoostingRegressor as SK
    n, d, depth, mss, msl, lr = case
    X, y = R.make_data(n, d, variant=variant)
    return X, y, SK(n_estimators=T, learning_rate=lr, max_depth=depth, min_samples_split=mss, min_samples_leaf=msl, random_state=0).fit(X, y)


@pytest.mark.parametrize("case,T", R.PARITY_CASES, ids=[f"{'-'.join(str(v) for v in c)}-{T}" for c, T in R.PARITY_CASES])
def test_training_rows_agree_with_sklearn(dev, case, T):
    """On continuous features exact score ties arise only between candidates that induce the same partition, so the training rows'
    predictions do not depend on the tie rule: every stage and train_score_ agree with scikit-learn's within ``gbr_replay.parity_bound``.
    (A failure here beside a passing certificate is a near tie between different partitions only if the printed ``optimal_margin`` lies
    inside its allowance; anything else is a defect.)"""
    X, y, sk = _sklearn_model(case, None, T)
    _, _, reg = _fit(dev, case, T=T)
    stages, sk_stages = np.array(list(reg.staged_predict(X))), np.array(list(sk.staged_predict(X)))
    bound, score_bound = R.parity_bound(y, sk_stages, case[5], float(np.average(y)))
    err, score_err = np.abs(stages - sk_stages).max(axis=1), np.abs(reg.train_score_ - sk.train_score_)
    print(f"{case}: max |ours - scikit-learn| {err.max():.3e} (bound at the last stage {bound[-1]:.3e}), train_score_ {score_err.max():.3e} "
          f"(bound {score_bound[-1]:.3e})")
    ok = (err <= bound).all() and (score_err <= score_bound).all()
    if not ok:
        print("optimal_margin", _certify(reg, X, y)[0]["optimal_margin"])
    assert ok and reg.init_ == float(np.ravel(sk.init_.constant_)[0]) and len(reg.trees_["left"]) == sum(e.tree_.node_count for e in sk.estimators_[:, 0])


def test_tie_rule_lowest_feature_wins(dev):
    """Column 3 is a copy of column 1: every score of one is a score of the other, bit for bit, and no split may name column 3."""
    X, y = R.make_data(257, 5)
    X[:, 3] = X[:, 1]
    _, _, reg = _fit(dev, (257, 5, 5, 2, 1, 0.1), T=10, data=(X, y))
    split = reg.trees_["left"] >= 0
    assert (reg.trees_["feature"][split] == 1).any() and not (reg.trees_["feature"][split] == 3).any()
    _certify(reg, X, y)


# ---- prediction from scikit-learn's trees: exact ----------------------------------------------------------------------------------------
def _threshold_queries(sk, X):
    """Training rows, and for every split node one row with that feature exactly on the threshold's float32 value, one float32 below and
    one above (a midpoint of two float32 values is often no float32 value: then the three straddle it)."""
    rs = np.random.RandomState(0)
    rows = [X.astype(np.float32)]
    for est in sk.estimators_[:, 0]:
        t = est.tree_
        for f, thr in zip(t.feature[t.feature >= 0], t.threshold[t.feature >= 0]):
            at = np.float32(thr)
            q = np.repeat(X[rs.randint(len(X))][None, :].astype(np.float32), 3, axis=0)
            q[:, f] = [np.nextafter(at, np.float32(-np.inf)), at, np.nextafter(at, np.float32(np.inf))]
            rows.append(q)
    return np.concatenate(rows)


@pytest.mark.parametrize("case,variant,T", R.CASES, ids=IDS)
def test_adopted_model_predicts_what_sklearn_predicts(dev, case, variant, T):
    from bbbp_amd.gradient_boosting import GradientBoostingRegressor
    X, y, sk = _sklearn_model(case, variant, T)
    reg = GradientBoostingRegressor.from_sklearn(sk, dev)
    Q = _threshold_queries(sk, X)
    assert np.array_equal(reg.predict(Q), sk.predict(Q))
    ours, theirs = list(reg.staged_predict(Q)), list(sk.staged_predict(Q))
    assert len(ours) == len(theirs) == T and all(np.array_equal(a, b) for a, b in zip(ours, theirs))
    on_device = reg.predict(torch.from_numpy(Q).to(dev))
    assert on_device.is_cuda and on_device.dtype == torch.float64 and np.array_equal(on_device.cpu().numpy(), sk.predict(Q))
    assert torch.equal(reg.predict_device(torch.from_numpy(Q).to(dev)), on_device)
    assert reg.n_estimators_ == T and reg.init_ == float(np.average(y)) and np.array_equal(reg.train_score_, sk.train_score_)


def test_from_sklearn_refuses_what_it_cannot_adopt(dev):
    from sklearn.ensemble import GradientBoostingClassifier, GradientBoostingRegressor as SK
    from sklearn.linear_model import LinearRegression
    from bbbp_amd.gradient_boosting import GradientBoostingRegressor
    X, y = R.make_data(64, 3)
    with pytest.raises(NotImplementedError, match="squared_error"):
        GradientBoostingRegressor.from_sklearn(SK(n_estimators=2, loss="huber").fit(X, y), dev)
    with pytest.raises(NotImplementedError, match="squared_error"):
        GradientBoostingRegressor.from_sklearn(GradientBoostingClassifier(n_estimators=2).fit(X, y > 0), dev)
    with pytest.raises(NotImplementedError, match="init"):
        GradientBoostingRegressor.from_sklearn(SK(n_estimators=2, init=LinearRegression()).fit(X, y), dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GradientBoostingRegressor.from_sklearn(SK(n_estimators=2).fit(X, y), "cpu")
    sk = SK(n_estimators=2, max_depth=None, min_samples_split=0.2).fit(X, y)        # limits this class would refuse are stored as None
    reg = GradientBoostingRegressor.from_sklearn(sk, dev)
    assert reg.max_depth is None and reg.min_samples_split is None and np.array_equal(reg.predict(X), sk.predict(X))
    assert reg.set_params(random_state=3) is reg and reg.random_state == 3      # set_params judges only what is being set


# ---- determinism --------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def _batch(dev, problems):
    """Fit the chains of ``problems`` -- (X, y, (n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf)) -- in one
    batch: per chain (trees, raw scores, train scores)."""
    from bbbp_amd import gradient_boosting as G
    chains = []
    for X, y, params in problems:
        mat = G._Matrix(np.ascontiguousarray(X, dtype=np.float32), dev)
        chains.append(G._Chain(mat, torch.from_numpy(y).to(dev), float(np.average(y)), *params))
    keep = G._fit_chains(chains, "bbbp_gbr_fit")
    out = [(c.trees(), c.raw.cpu().numpy(), c.train_score.cpu().numpy()) for c in chains]
    del keep
    return out


def test_determinism_alone_in_a_batch_reversed_and_again(dev):
    X, y = R.make_data(257, 5)
    mine = (X, y, (10, 0.1, 5, 2, 1))
    others = [(X, y, (4, 0.05, 3, 5, 1)), R.make_data(1025, 3) + ((12, 0.1, 7, 2, 3),), (X, y, (10, 0.01, 5, 2, 1)), R.make_data(65, 9, seed=3) + ((3, 0.1, 1, 10, 1),)]
    alone = _batch(dev, [mine])[0]
    mixed = others[:2] + [mine] + others[2:]
    batch = _batch(dev, mixed)
    backwards = _batch(dev, mixed[::-1])
    again = _batch(dev, [mine])[0]
    for name, got in (("in a batch", batch[2]), ("in the reversed batch", backwards[2]), ("a second run", again)):
        assert _same(alone[0], got[0]) and np.array_equal(alone[1], got[1]) and np.array_equal(alone[2], got[2]), name
    assert all(_same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(batch, backwards[::-1]))
    reg = GBR(10, learning_rate=0.1, max_depth=5, device=dev).fit(X, y)
    assert _same(alone[0], reg.trees_) and np.array_equal(alone[1], reg._train_raw) and np.array_equal(alone[2], reg.train_score_)


def test_prefixes_of_a_longer_fit(dev):
    """Without subsampling the first k trees of a 12-tree fit are the k-tree fit, bit for bit, and its staged predictions are that fit's."""
    X, y = R.make_data(257, 5)
    kw = dict(learning_rate=0.1, max_depth=4, device=dev)
    long = GBR(12, **kw).fit(X, y)
    staged = list(long.staged_predict(X[:64]))
    for k in (1, 5, 12):
        short = GBR(k, **kw).fit(X, y)
        end = int(long.trees_["root"][k])
        cut = {name: (v[:k + 1] if name == "root" else v[:end]) for name, v in long.trees_.items()}
        assert _same(cut, short.trees_) and np.array_equal(long.train_score_[:k], short.train_score_), k
        assert np.array_equal(staged[k - 1], short.predict(X[:64])), k


def test_batched_folds_equal_single_fits(dev):
    """The bake-off's shape: five shuffled folds and the refit in one bbbp_gbr_fit batch, each equal to its single fit bit for bit."""
    from sklearn.model_selection import KFold
    from bbbp_amd.gradient_boosting import fit_regressors
    X, y = R.make_data(257, 5)
    problems = [(X[tr], y[tr]) for tr, _ in KFold(5, shuffle=True, random_state=42).split(X)] + [(X, y)]
    kw = dict(n_estimators=8, learning_rate=0.1, max_depth=5, random_state=42, device=dev)
    batch = fit_regressors(problems, **kw)
    assert len(batch) == 6
    for (Xp, yp), reg in zip(problems, batch):
        single = GBR(**kw).fit(Xp, yp)
        assert _same(reg.trees_, single.trees_) and np.array_equal(reg.train_score_, single.train_score_) and np.array_equal(reg._train_raw, single._train_raw)
        assert reg.init_ == single.init_ == float(np.average(yp)) and np.array_equal(reg.predict(X), single.predict(X))
    col = torch.from_numpy(y[:, None]).to(dev)                              # [n, 1] targets and device-resident inputs are the same problem
    again = GBR(**kw).fit(torch.from_numpy(X).to(dev), col)
    assert _same(again.trees_, batch[-1].trees_)


def test_stacking_regressor_takes_the_regressor(dev, monkeypatch):
    """ensemble.StackingRegressor clones the learner, fits it on all rows and on KFold(5) training parts: its meta column is the out-of-fold
    predictions of five direct fits."""
    from bbbp_amd import ensemble
    X, y = R.make_data(60, 4)
    seen = {}
    fit = ensemble.StackedEnsemble.fit
    monkeypatch.setattr(ensemble.StackedEnsemble, "fit", lambda self, M, t: (seen.update(meta=np.array(M)), fit(self, M, t))[1])
    stack = ensemble.StackingRegressor([("gb", GBR(8, max_depth=3, device=dev))]).fit(X, y)
    p = stack.predict(X)
    assert p.shape == (60,) and np.isfinite(p).all()
    fitted = dict(stack.estimators_)["gb"]
    assert type(fitted).__name__ == "GradientBoostingRegressor" and fitted.n_estimators_ == 8
    assert np.array_equal(fitted.predict(X), GBR(8, max_depth=3, device=dev).fit(X, y).predict(X))
    want = np.empty(60)
    for f in range(5):
        test = np.arange(12 * f, 12 * f + 12)
        train = np.setdiff1d(np.arange(60), test)
        want[test] = GBR(8, max_depth=3, device=dev).fit(X[train], y[train]).predict(X[test])
    assert seen["meta"].shape == (60, 1) and np.array_equal(seen["meta"][:, 0], want)


# ---- poisoned memory ------------------------------------------------------------------------------------------------------------------------
def test_fit_and_predict_under_poison(dev, monkeypatch):
    """Outputs, the work area and the node slots come out of pools filled with 0x00, 0xFF and 0x7B: nothing may depend on what an
    allocation held (the table slot the squared error leaves unused among them), and no guard band may be written (tests/poison.py)."""
    X, y = R.make_data(257, 5)
    results = {}
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            reg = GBR(6, learning_rate=0.1, max_depth=7, device=dev).fit(X, y)
            pred = reg.predict(X[:100])
            staged = np.array(list(reg.staged_predict(X[:33])))
            torch.cuda.synchronize()
        assert pa.check() >= 10, "the chain's allocations did not go through the pools"
        pa.release()
        results[fill] = (reg.trees_, reg.train_score_, reg._train_raw, pred, staged)
    clean = GBR(6, learning_rate=0.1, max_depth=7, device=dev).fit(X, y)
    first = (clean.trees_, clean.train_score_, clean._train_raw, clean.predict(X[:100]), np.array(list(clean.staged_predict(X[:33]))))
    for fill in FILLS:
        got = results[fill]
        assert _same(first[0], got[0]) and all(np.array_equal(a, b) for a, b in zip(first[1:], got[1:])), hex(fill)
    assert np.isfinite(first[1]).all() and np.isfinite(first[3]).all()
    _certify(reg, X, y)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu_box(dev):
    from bbbp_amd.gradient_boosting import MAX_ROWS, MAX_FEATURES
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GBR(device="cpu")
    with pytest.raises(ValueError, match="BBBP_GBT_FIT_MAX_N"):
        GBR(device=dev).fit(torch.zeros(MAX_ROWS + 1, 2, device=dev), np.zeros(MAX_ROWS + 1))
    with pytest.raises(ValueError, match="BBBP_GBT_FIT_MAX_D"):
        GBR(device=dev).fit(torch.zeros(4, MAX_FEATURES + 1, device=dev), np.zeros(4))
    with pytest.raises(ValueError, match="NaN"):
        GBR(device=dev).fit(torch.full((4, 2), float("nan"), device=dev), np.zeros(4))
    with pytest.raises(ValueError, match="NaN or infinity"):
        GBR(device=dev).fit(torch.zeros(4, 2, device=dev), torch.tensor([0.0, 1.0, float("inf"), 2.0], device=dev))
    with pytest.raises(NotImplementedError, match="more than one output"):
        GBR(device=dev).fit(torch.zeros(4, 2, device=dev), torch.zeros(4, 2, device=dev))
    with pytest.raises(ValueError, match="overflows float64"):
        GBR(device=dev).fit(torch.zeros(4, 2, device=dev), np.array([1e200, -1e200, 1e200, -1e200]))
    reg = GBR(2, device=dev).fit(np.arange(8.0).reshape(4, 2), np.array([0.0, 0.5, 4.0, 4.5]))
    with pytest.raises(ValueError, match="queries"):
        reg.predict(np.zeros((3, 5)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.predict(torch.zeros(3, 2))
    with pytest.raises(TypeError, match="CUDA"):
        reg.predict_device(np.zeros((3, 2)))
    p = reg.predict(np.array([[0.0, 1.0], [6.0, 7.0]]))
    assert p[0] < reg.init_ < p[1] and reg.predict(np.zeros((0, 2))).shape == (0,)


# ---- quality against scikit-learn's own scatter -----------------------------------------------------------------------------------------
def _quality_data():
    """n = 600 (400 rows to fit, 200 held out), d = 12, on which scikit-learn itself scatters at depth 3 as well as 5.  On continuous targets
    its fits agree on every large node whatever the random_state, so the yardstick would have no width.  The targets are therefore rounded to
    halves, and column 11 is the most informative column with its values permuted among the training rows of each target value: in the first
    tree the two columns' sorted target sequences, hence every prefix sum and score, are equal bit for bit while the rows on either side
    differ; scikit-learn takes whichever its random feature order visits first, and the fits part from the first split on."""
    rs = np.random.RandomState(4)
    X = rs.randn(600, 12)
    y = np.round(2.0 * (X[:, :6] @ rs.randn(6) + np.sin(2.0 * X[:, 0]) + 0.7 * rs.randn(600))) / 2.0
    perm = np.random.RandomState(104)
    best = int(np.argmax(np.abs([np.corrcoef(X[:400, j], y[:400])[0, 1] for j in range(12)])))
    for level in np.unique(y[:400]):
        idx = np.nonzero(y[:400] == level)[0]
        X[idx, 11] = X[perm.permutation(idx), best]
    X[400:, 11] = X[perm.permutation(np.arange(400, 600)), best]
    return X[:400], y[:400], X[400:], y[400:]


@pytest.mark.parametrize("depth", [3, 5])
def test_quality_within_sklearn_scatter(dev, depth):
    """30 trees: the held-out R^2 lies within scikit-learn's own min-max range over random_state 0..9, widened by that range's width on
    each side.  Measured on one MI355X (DESIGN.md records the same figures):
    depth 3: R^2 0.578519, scikit-learn [0.578094, 0.587999]
    depth 5: R^2 0.582632, scikit-learn [0.562622, 0.581267] (0.0014 above scikit-learn's highest, inside the widened range that ends at 0.599912)."""
    from sklearn.ensemble import GradientBoostingRegressor as SK
    from sklearn.metrics import r2_score
    X, y, Xt, yt = _quality_data()
    theirs = [float(r2_score(yt, SK(n_estimators=30, max_depth=depth, random_state=rs).fit(X, y).predict(Xt))) for rs in range(10)]
    ours = float(r2_score(yt, GBR(30, max_depth=depth, device=dev).fit(X, y).predict(Xt)))
    print(f"depth {depth}: held-out R^2 {ours:.6f}, scikit-learn [{min(theirs):.6f}, {max(theirs):.6f}]")
    w = max(theirs) - min(theirs)
    assert w > 0, "scikit-learn's own fits do not scatter on this problem: the yardstick has no width"
    assert min(theirs) - w <= ours <= max(theirs) + w
