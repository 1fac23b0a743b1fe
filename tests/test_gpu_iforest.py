"""GPU: isolation_forest.IsolationForest.  A fit has no summation order (hashes, float32 minima and maxima, three float64 roundings per
threshold), so the GPU's trees are compared bit for bit with the numpy restatement (tests/iforest_numpy.py), which tests/test_iforest_cpu.py
ties to scikit-learn in distribution, and certified by the replayer (tests/iforest_replay.py); scores are compared bit for bit with
scikit-learn's on adopted models and with the restatement's on own fits."""
import functools
import warnings

import numpy as np
import pytest
import torch

import iforest_numpy as N
import iforest_replay as R
from poison import FILLS, moated, poisoned_allocations
from test_iforest_cpu import problem

pytestmark = pytest.mark.gpu

TREE_KEYS = ("left", "right", "feature", "threshold", "value", "n_node_samples", "root")


def IF(**kw):
    from bbbp_amd.isolation_forest import IsolationForest
    return IsolationForest(**kw)


def _same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def _long_problem():
    """1 100 rows of the shared problem's kind: room for a tree of BBBP_IFOREST_MAX_SAMPLES rows."""
    rng = np.random.default_rng(20261021)
    X = rng.standard_normal((1100, 6)).astype(np.float32)
    X[:, 1] = np.round(X[:, 1], 1)
    X[:, 5] = X[:, 5] > 0
    X.setflags(write=False)
    return X


def _data(name):
    if name == "d1":
        return np.ascontiguousarray(problem()[:, :1])
    if name == "constant":
        return problem(True)
    if name == "identical":
        return np.ascontiguousarray(np.tile(problem()[3], (50, 1)))
    if name == "long":
        return _long_problem()
    return problem(n=int(name))


# data, max_samples, max_samples_.  2: depth 1; 65: a second wave; 256: "auto"; 257: the first row slot beyond the work-group's width;
# 600 / 1000: the clamp to n; 1024 on 600 rows: the clamp again; 1024 on 1 100 rows: BBBP_IFOREST_MAX_SAMPLES itself
CASES = [("600", 2, 2), ("600", 3, 3), ("600", 64, 64), ("600", 65, 65), ("600", "auto", 256), ("600", 257, 257), ("600", 600, 600),
         ("100", "auto", 100), ("100", 1000, 100), ("600", 1024, 600), ("long", 1024, 1024), ("long", 0.5, 550),
         ("d1", 64, 64), ("constant", "auto", 256), ("identical", "auto", 50)]
SEED, TREES = 5, 3


@functools.lru_cache(maxsize=None)
def _want(data, S, seed=SEED, T=TREES):
    trees, samples = N.fit_forest(_data(data), T, S, seed)
    for a in list(trees.values()) + [samples]:
        a.setflags(write=False)
    return trees, samples


_FITS = {}


def _fit(dev, data, max_samples, seed=SEED, T=TREES):
    """One GPU fit per case, shared by the tests that look at it."""
    key = (data, max_samples, seed, T)
    if key not in _FITS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)   # the clamp's warning, scikit-learn's
            _FITS[key] = IF(n_estimators=T, max_samples=max_samples, random_state=seed, device=dev).fit(_data(data))
    return _FITS[key]


@pytest.mark.parametrize("data,max_samples,S", CASES)
def test_fit_equals_the_restatement(dev, data, max_samples, S):
    est = _fit(dev, data, max_samples)
    X = _data(data)
    want, rows = _want(data, S)
    assert est.max_samples_ == S and est.n_features_in_ == X.shape[1] and est.n_estimators_ == TREES and est.offset_ == -0.5
    assert tuple(est.trees_) == TREE_KEYS
    for k in TREE_KEYS:
        assert est.trees_[k].dtype == want[k].dtype and np.array_equal(est.trees_[k], want[k]), k
    assert est.estimators_samples_.dtype == np.int32 and est.estimators_samples_.shape == (TREES, S)
    assert np.array_equal(est.estimators_samples_, rows) and (np.diff(rows, axis=1) > 0).all()
    split = want["left"] >= 0
    if data == "identical":                                # every feature is constant: the root is a leaf that holds all rows
        assert not split.any() and (est.trees_["n_node_samples"] == 50).all() and len(est.trees_["left"]) == TREES
    elif data == "constant":
        assert split.any() and not (est.trees_["feature"][split] == 6).any()
    else:
        assert split.any()
    if S == 2:
        assert len(est.trees_["left"]) == 3 * TREES           # depth 1: a root and two leaves


@pytest.mark.parametrize("data,max_samples,S", CASES)
def test_replayer_certifies_the_fit(dev, data, max_samples, S):
    est = _fit(dev, data, max_samples)
    seen = R.replay(_data(data), est.trees_, est.estimators_samples_, S, seed=SEED)
    assert seen["nodes"] == len(est.trees_["left"]) and seen["max_depth"] <= N.depth_limit(S)
    if data in ("600", "constant") and S >= 64:
        assert seen["redraws"] > 0


def test_seeds_differ_and_fewer_trees_are_a_prefix(dev):
    a, b = _fit(dev, "600", 64), _fit(dev, "600", 64, seed=6)
    assert not np.array_equal(a.estimators_samples_, b.estimators_samples_) and not _same(a.trees_, b.trees_)
    assert _same(b.trees_, _want("600", 64, seed=6)[0])
    more = _fit(dev, "600", 64, T=7)
    k = int(a.trees_["root"][-1])
    assert np.array_equal(more.estimators_samples_[:TREES], a.estimators_samples_) and np.array_equal(more.trees_["root"][:TREES + 1], a.trees_["root"])
    assert all(np.array_equal(more.trees_[key][:k], a.trees_[key]) for key in TREE_KEYS if key != "root")


# ---- scoring ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _queries():
    Q = np.random.default_rng(7).standard_normal((1000, 6)).astype(np.float32) * 1.5
    Q[:600:2] = problem()[:600:2]                          # half of the first rows are training rows
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def _sk(n_estimators, max_samples, contamination):
    from sklearn.ensemble import IsolationForest
    return IsolationForest(n_estimators=n_estimators, max_samples=max_samples, contamination=contamination, random_state=42).fit(problem())


@pytest.mark.parametrize("n_estimators,max_samples,contamination", [(1, 64, "auto"), (7, 256, "auto"), (100, 64, 0.05), (100, "auto", 0.05),
                                                                    (7, 600, "auto")])
def test_adopted_sklearn_models_score_bit_for_bit(dev, n_estimators, max_samples, contamination):
    from bbbp_amd.isolation_forest import IsolationForest
    sk = _sk(n_estimators, max_samples, contamination)
    est = IsolationForest.from_sklearn(sk, device=dev)
    assert est.offset_ == sk.offset_ and est.max_samples_ == sk.max_samples_ and est.n_estimators_ == n_estimators
    for m in (1, 255, 257, 1000):
        Xq = _queries()[:m]
        s = est.score_samples(Xq)
        assert isinstance(s, np.ndarray) and s.dtype == np.float64 and np.array_equal(s, sk.score_samples(Xq)), m
        assert np.array_equal(est.decision_function(Xq), sk.decision_function(Xq)), m
        p = est.predict(Xq)
        assert p.dtype == sk.predict(Xq).dtype and np.array_equal(p, sk.predict(Xq)), m
    Xd = torch.from_numpy(_queries()[:257].copy()).to(dev)
    s = est.score_samples(Xd)
    assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.float64 and np.array_equal(s.cpu().numpy(), sk.score_samples(_queries()[:257]))
    assert np.array_equal(est.decision_function(Xd).cpu().numpy(), sk.decision_function(_queries()[:257]))
    assert np.array_equal(est.predict(Xd), sk.predict(_queries()[:257]))


@pytest.mark.parametrize("contamination", ["auto", 0.05])
def test_own_fits_score_like_the_restatement(dev, contamination):
    from bbbp_amd import isolation_forest as F
    X = problem()
    before = F._GROWN["launches"]
    est = IF(n_estimators=20, contamination=contamination, random_state=42, device=dev).fit(X)
    assert F._GROWN["launches"] == before + 1              # all trees in one launch
    want = N.score_samples(est.trees_, X, est.max_samples_)
    assert _same(est.trees_, N.fit_forest(X, 20, 256, 42)[0])
    for Xq in (X, torch.from_numpy(X.copy()).to(dev)):
        s = est.score_samples(Xq)
        assert np.array_equal(s if isinstance(s, np.ndarray) else s.cpu().numpy(), want)
    assert est.offset_ == (-0.5 if contamination == "auto" else np.percentile(want, 100.0 * contamination))
    assert np.array_equal(est.decision_function(X), want - est.offset_)
    flags = IF(n_estimators=20, contamination=contamination, random_state=42, device=dev).fit_predict(X)
    assert flags.dtype == np.ones(1, dtype=int).dtype and np.array_equal(flags, est.predict(X)) and np.array_equal(flags, N.predict(est.trees_, X, 256, est.offset_))
    if contamination == 0.05:
        assert (flags == -1).sum() == 30 and (flags[:30] == -1).sum() >= 20      # 5 % of 600, most of them the planted outliers
    assert est.score_samples(X[:0]).shape == (0,)


def test_fit_from_a_device_matrix_equals_the_numpy_fit(dev):
    X = problem()
    a = _fit(dev, "600", 64)
    b = IF(n_estimators=TREES, max_samples=64, random_state=SEED, device=dev).fit(torch.from_numpy(X.copy()).to(dev))
    assert _same(a.trees_, b.trees_) and np.array_equal(a.estimators_samples_, b.estimators_samples_)


# ---- poisoned memory ------------------------------------------------------------------------------------------------------------------------
def test_fit_and_path_sum_under_poison(dev, monkeypatch):
    """Node slots, row sets, node counts and path sums come out of pools filled with 0x00, 0xFF and 0x7B: nothing may depend on what an
    allocation held, and no guard band may be written (tests/poison.py)."""
    X = problem()
    results = {}
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            est = IF(n_estimators=4, max_samples=257, contamination=0.05, random_state=3, device=dev).fit(X)
            s = est.score_samples(X[:300])
            torch.cuda.synchronize()
        assert pa.check() >= 8, "the forest's allocations did not go through the pools"
        pa.release()
        results[fill] = (est.trees_, est.estimators_samples_, s, est.offset_)
    first = results[FILLS[0]]
    for fill in FILLS[1:]:
        got = results[fill]
        assert _same(first[0], got[0]) and np.array_equal(first[1], got[1]) and np.array_equal(first[2], got[2]) and first[3] == got[3], hex(fill)
    assert _same(first[0], N.fit_forest(X, 4, 257, 3)[0]) and np.isfinite(first[2]).all()


@pytest.mark.parametrize("fill", FILLS)
def test_moated_queries_with_a_padded_leading_dimension(dev, fill):
    est = _fit(dev, "600", 64)
    Xq = _queries()[:257]
    view, check = moated(torch.from_numpy(Xq.copy()), fill, ld=11, offset=1, device=dev)
    assert view.stride() == (11, 1)
    sums = est._path_sums(view).cpu().numpy()
    torch.cuda.synchronize()
    check()
    assert np.array_equal(sums, N.path_sums(est.trees_, Xq, est.trees_["value"]))
    assert np.array_equal(N.scores_of_path_sums(sums, TREES, 64), est.score_samples(Xq))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_parameter(dev):
    import scipy.sparse as sp
    from bbbp_amd import isolation_forest as F
    X = problem()
    for kw, exc, name in ((dict(max_features=0.5), NotImplementedError, "max_features"), (dict(bootstrap=True), NotImplementedError, "bootstrap"),
                          (dict(warm_start=True), NotImplementedError, "warm_start")):
        with pytest.raises(exc, match=name):
            IF(device=dev, **kw)
    est = IF(random_state=0, device=dev)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        est.fit(X, sample_weight=np.ones(len(X)))
    with pytest.raises(NotImplementedError, match="sparse"):
        est.fit(sp.csc_matrix(X))
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[5, 2] = bad
        with pytest.raises(ValueError, match="X contains NaN, infinity"):
            est.fit(Xb)
        with pytest.raises(ValueError, match="X contains NaN, infinity"):
            est.fit(torch.from_numpy(Xb).to(dev))
        with pytest.raises(ValueError, match="X contains NaN, infinity"):
            _fit(dev, "600", 64).score_samples(Xb)
    with pytest.raises(ValueError, match="random_state"):
        IF(device=dev).fit(X)
    with pytest.raises(NotImplementedError, match="sparse"):
        _fit(dev, "600", 64).score_samples(sp.csr_matrix(X))
    # over-limit arguments return before any GPU call
    before = F._GROWN["launches"]
    big = _data("long")
    for ms in (1025, 0.99):                                # 0.99 of 1 100 rows is 1 089
        with pytest.raises(ValueError, match="max_samples.*BBBP_IFOREST_MAX_SAMPLES"):
            IF(max_samples=ms, random_state=0, device=dev).fit(big)
    with pytest.raises(ValueError, match="BBBP_IFOREST_MAX_D"):
        IF(random_state=0, device=dev).fit(np.zeros((4, 1025), dtype=np.float32))
    assert F._GROWN["launches"] == before
    L = F._lib.lib()
    fake = 4096                                            # never dereferenced: validation comes first
    assert L.bbbp_iforest_fit(None, fake, 6, 600, 6, 1025, 3, 0, fake, fake, fake, fake, fake, fake, fake) == 1
    assert b"BBBP_IFOREST_MAX_SAMPLES" in L.bbbp_last_error()
    assert L.bbbp_iforest_fit(None, fake, 6, 100, 6, 256, 3, 0, fake, fake, fake, fake, fake, fake, fake) == 1
    assert b"above n" in L.bbbp_last_error()
    assert L.bbbp_iforest_path_sum(None, fake, 5, 10, 6, fake, fake, fake, fake, fake, fake, 3, fake) == 1
    assert b"leading dimension" in L.bbbp_last_error()
