"""CPU: the numpy restatement of ``isolation_forest`` (tests/iforest_numpy.py) and its replayer (tests/iforest_replay.py).  The scoring half
is pinned to scikit-learn's ``score_samples`` / ``decision_function`` / ``predict`` / ``offset_`` bit for bit on scikit-learn's own trees;
the fit rule, whose random stream cannot match scikit-learn's, is certified by the replayer and compared with scikit-learn in distribution.
tests/test_gpu_iforest.py holds the kernels to the restatement bit for bit."""
import functools

import numpy as np
import pytest

import iforest_numpy as N
import iforest_replay as R
from sklearn_trees import trees_of_sklearn


@functools.lru_cache(maxsize=None)
def _problem(constant_column):
    rng = np.random.default_rng(20261020)
    X = rng.standard_normal((600, 6))
    X[:30] += 4.0 * rng.standard_normal((30, 6))
    X = X.astype(np.float32)
    X[:, 1] = np.round(X[:, 1], 1)
    X[:, 5] = X[:, 5] > 0                                  # binary: constant inside many nodes, so the feature is drawn again
    if constant_column:
        X = np.hstack([X, np.full((600, 1), 2.5, dtype=np.float32)])
    X.setflags(write=False)
    return X


def problem(constant_column=False, n=600):
    """The shared problem: 600 x 6 float32, the first 30 rows outliers, column 1 on a grid of 0.1, column 5 binary; optionally a seventh,
    constant column.  Read-only: the tests share it."""
    return _problem(bool(constant_column))[:n]


SK_CONFIGS = [dict(), dict(max_samples=64, n_estimators=7), dict(max_samples=600), dict(contamination=0.05)]


@functools.lru_cache(maxsize=None)
def sk_model(i, seed=42):
    from sklearn.ensemble import IsolationForest
    return IsolationForest(random_state=seed, **SK_CONFIGS[i]).fit(problem())


@pytest.mark.parametrize("i", range(len(SK_CONFIGS)))
def test_scoring_restatement_equals_sklearn_bit_for_bit(i):
    sk = sk_model(i)
    trees = trees_of_sklearn(sk)
    X = problem()
    assert np.array_equal(N.node_depths(trees), np.concatenate([e.tree_.compute_node_depths() for e in sk.estimators_]))
    off = N.offset(trees, X, sk._max_samples, sk.contamination)
    assert off == sk.offset_
    for Xq in (X[17:18], X):
        s = N.score_samples(trees, Xq, sk._max_samples)
        assert s.dtype == np.float64 and np.array_equal(s, sk.score_samples(Xq))
        assert np.array_equal(s - off, sk.decision_function(Xq))
        assert np.array_equal(N.predict(trees, Xq, sk._max_samples, off), sk.predict(Xq))
    if i == 3:
        assert (sk.predict(X) == -1).sum() == 30


def test_replayer_passes_sklearns_trees_and_the_restatements():
    X = problem()
    for i in (1, 0):
        sk = sk_model(i)
        seen = R.replay(X, trees_of_sklearn(sk), R.samples_of_sklearn(sk), sk.max_samples_, own=False)
        assert seen["splits"] > 0 and seen["nodes"] == sum(e.tree_.node_count for e in sk.estimators_)
    for S, T, Xp in ((64, 5, X), (256, 3, problem(True)), (2, 3, X), (3, 3, X)):
        trees, samples = N.fit_forest(Xp, T, S, 11)
        seen = R.replay(Xp, trees, samples, S, seed=11)
        assert seen["nodes"] == len(trees["left"]) and seen["max_depth"] <= N.depth_limit(S)
        if S >= 64:
            assert seen["redraws"] > 0                     # the binary (and the constant) column made a node draw again
            assert not (trees["feature"][trees["left"] >= 0] == 6).any()
    assert seen["stop_reasons"].keys() <= {"rows", "depth", "constant"}


def _corrupt(check):
    """The restatement's forest (64 rows per tree, seed 11) corrupted in one way, and the replayer's arguments for it."""
    X = problem()
    trees, samples = N.fit_forest(X, 2, 64, 11)
    trees, samples, seed = {k: v.copy() for k, v in trees.items()}, samples.copy(), None
    inner = np.nonzero(trees["left"] >= 0)[0]
    node = int(inner[3])
    if check == "stop":                                    # the root becomes a leaf that no rule allows
        trees["left"][0] = trees["right"][0] = -1
    elif check == "samples":
        trees["n_node_samples"][node] += 1
    elif check == "valid":                                 # a threshold above the feature's maximum: nothing would go right
        trees["threshold"][node] = 1e30
    elif check == "sample":
        samples[1, 5] = samples[1, 4]
    elif check == "draw":                                  # still inside [lo, hi), but not the hash's
        trees["threshold"][0] = np.nextafter(trees["threshold"][0], -np.inf)
        seed = 11
    return X, trees, samples, seed


@pytest.mark.parametrize("check", ["stop", "samples", "valid", "sample", "draw"])
def test_replayer_names_each_corruption(check):
    X, trees, samples, seed = _corrupt(check)
    with pytest.raises(R.ReplayError) as e:
        R.replay(X, trees, samples, 64, seed=seed)
    assert e.value.check == check, str(e.value)


def test_split_on_constant_feature_is_not_valid():
    X = problem(True)
    trees, samples = N.fit_forest(X, 1, 64, 3)
    trees = {k: v.copy() for k, v in trees.items()}
    trees["feature"][0], trees["threshold"][0] = 6, 2.5
    with pytest.raises(R.ReplayError) as e:
        R.replay(X, trees, samples, 64)
    assert e.value.check == "valid"


def test_hash_equals_the_librarys_under_the_new_tag():
    from bbbp_amd import _lib
    L = _lib.lib()
    for seed in (0, 42, 2 ** 63 + 5):
        for t in (0, 1, 99):
            key = L.bbbp_rf_hash(L.bbbp_rf_hash(seed, N.TAG), t)
            assert key == N.tree_key(seed, t)
            assert L.bbbp_rf_hash(key, 0) == N.child_key(key, 0) and L.bbbp_rf_hash(key, N.THRESHOLD) == int(N.rf_hash(key, N.THRESHOLD))
            stream = L.bbbp_rf_hash(key, N.SAMPLE)
            assert [L.bbbp_rf_hash(stream, i) for i in range(5)] == [int(v) for v in N.rf_hash(stream, np.arange(5, dtype=np.uint64))]
    from rf_numpy import tree_key as forest_key
    assert N.tree_key(42, 0) != forest_key(42, 0)          # the tag keeps these streams apart from the forests'
    assert L.bbbp_iforest_tree_capacity(256) == 511 and L.bbbp_iforest_tree_capacity(N.MAX_SAMPLES + 1) == 0
    assert b"BBBP_IFOREST_MAX_SAMPLES" in L.bbbp_last_error()
    assert 0 < L.bbbp_iforest_work_bytes(N.MAX_SAMPLES) <= 128 * 1024 and L.bbbp_iforest_work_bytes(0) == 0


def test_constructor_refusals_and_clone_without_a_gpu():
    from sklearn.base import clone
    from bbbp_amd.isolation_forest import IsolationForest, depth_limit, resolve_max_samples
    est = IsolationForest(n_estimators=7, max_samples=0.5, contamination=0.05, random_state=42)
    twin = clone(est)
    assert twin is not est and twin.get_params() == est.get_params()
    assert twin.set_params(n_estimators=9).n_estimators == 9
    for kw, exc, name in ((dict(max_features=0.5), NotImplementedError, "max_features"), (dict(max_features=1), NotImplementedError, "max_features"),
                          (dict(bootstrap=True), NotImplementedError, "bootstrap"), (dict(warm_start=True), NotImplementedError, "warm_start"),
                          (dict(contamination=0.7), ValueError, "contamination"), (dict(max_samples="all"), ValueError, "max_samples"),
                          (dict(random_state=np.random.RandomState(0)), ValueError, "random_state"), (dict(n_estimators=0), ValueError, "n_estimators"),
                          (dict(colour=1), ValueError, "colour")):
        with pytest.raises(exc, match=name):
            IsolationForest(**kw)
    with pytest.raises(ValueError, match="n_estimators"):
        est.set_params(n_estimators=0)
    # max_samples as scikit-learn resolves it, and the depth limit
    assert resolve_max_samples("auto", 600) == 256 and resolve_max_samples("auto", 100) == 100 and resolve_max_samples(0.5, 601) == 300
    with pytest.warns(UserWarning, match="max_samples"):
        assert resolve_max_samples(1000, 100) == 100
    for S in (1, 2, 3, 4, 5, 64, 65, 256, 257, 1024):
        assert depth_limit(S) == int(np.ceil(np.log2(max(S, 2)))) == N.depth_limit(S)


def _mean_terms_and_scores(forests, X):
    """Per forest (trees, max_samples): every row's mean path term and its score."""
    means, scores = [], []
    for trees, S in forests:
        T = len(trees["root"]) - 1
        sums = N.path_sums(trees, X)
        means.append(sums / T)
        scores.append(N.scores_of_path_sums(sums, T, S))
    return np.stack(means), np.stack(scores)


def _compare(a, b):
    """(rms z, max |z|, overlap of the 30 lowest-scored rows) between two sets of S forests' (mean terms [S, m], scores [S, m])."""
    (ma, sa), (mb, sb) = a, b
    S = ma.shape[0]
    z = (ma.mean(axis=0) - mb.mean(axis=0)) / np.sqrt(ma.var(axis=0, ddof=1) / S + mb.var(axis=0, ddof=1) / S)
    low = lambda s: set(np.argsort(s.mean(axis=0), kind="stable")[:30].tolist())  # noqa: E731
    return float(np.sqrt(np.mean(z * z))), float(np.abs(z).max()), len(low(sa) & low(sb))


def test_agrees_with_sklearn_in_distribution():
    """Over S = 8 seeds of 100 trees (max_samples 256), per row z = (mean_ours - mean_sk) / sqrt(var_ours / S + var_sk / S) on the mean path
    term, against the same statistic between two disjoint sets of 8 scikit-learn seeds.  Our rms z may exceed scikit-learn-against-itself by
    at most 1.5x (a bias of one standard error per row gives more), and of the 30 lowest-scored rows by seed-mean at least as many as
    scikit-learn shares with itself, minus 2, must be shared with scikit-learn.

    Measured with the hash-driven restatement (seeds 0..7 against scikit-learn's random_state 0..7 and 100..107):
        ours vs scikit-learn          rms z 0.98, max |z| 3.1, overlap 29 / 30
        scikit-learn vs scikit-learn  rms z 0.84, max |z| 4.0, overlap 29 / 30"""
    from sklearn.ensemble import IsolationForest
    X = problem()
    S = 8
    ours = _mean_terms_and_scores([(N.fit_forest(X, 100, 256, seed)[0], 256) for seed in range(S)], X)
    sk = [[(trees_of_sklearn(m), m._max_samples) for m in (IsolationForest(random_state=first + s).fit(X) for s in range(S))] for first in (0, 100)]
    sk_a, sk_b = (_mean_terms_and_scores(f, X) for f in sk)
    rms, top, overlap = _compare(ours, sk_a)
    rms_sk, top_sk, overlap_sk = _compare(sk_a, sk_b)
    print(f"ours vs scikit-learn: rms z {rms:.2f}, max |z| {top:.1f}, overlap {overlap}/30; "
          f"scikit-learn vs scikit-learn: rms z {rms_sk:.2f}, max |z| {top_sk:.1f}, overlap {overlap_sk}/30")
    assert rms <= 1.5 * rms_sk
    assert overlap >= overlap_sk - 2
