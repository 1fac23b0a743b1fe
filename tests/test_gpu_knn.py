"""GPU: the fused float64 k-nearest-neighbour search (bbbp_knn_f64) against the direct-difference oracle of tests/knn_oracle.py -- exact
indices wherever the oracle's own gaps exceed the expansion's error bound a thousandfold --, and neighbors.KNeighborsClassifier /
grid_search_cv against scikit-learn's brute-force classifier."""
import functools
import itertools

import numpy as np
import pytest
import torch

from bbbp_amd.neighbors import KNeighborsClassifier, NearestNeighbors, grid_search_cv
from knn_oracle import U53, knn, make_points, min_gap_over_bound

pytestmark = pytest.mark.gpu

MS = (1, 63, 65, 130)
NS = ("k", 64, 65, 333, 4097)
DS = (1, 3, 16, 17, 100, 167)
KS = (1, 3, 7, 32)
DTYPES = (("f32", "f32"), ("f64", "f64"), ("f32", "f64"), ("f64", "f32"))
SLICES = (0, 1, 2, 7)
POOL_D = 200                     # operands are [:rows, :d] views of pools this wide: leading dimensions differ from d
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}


@functools.lru_cache(maxsize=None)
def _pool():
    """Host pools drawn once (values exact in float32, so every dtype combination sees the same numbers)."""
    return {"q": make_points(130, POOL_D, 11), "t": make_points(4097, POOL_D, 12)}


@functools.lru_cache(maxsize=None)
def _pool_dev():
    out = {}
    for name, v in _pool().items():
        out[name, "f64"] = torch.from_numpy(v).cuda()
        out[name, "f32"] = torch.from_numpy(v.astype(np.float32)).cuda()
    return out


def _check(dist, ind, Q, T, k, what, exclude_self=False):
    """The oracle's own gaps must exceed 1000 B for every query (asserted, no query exempt); then indices are exact and distances
    agree within the d-term-sum bound of both sides."""
    d = Q.shape[1]
    ratio = min_gap_over_bound(Q, T, k, exclude_self)
    assert (ratio >= 1000.0).all(), f"{what}: the test's inputs are too close to a tie (gap / B = {ratio.min():.3g})"
    want_dist, want_ind, _ = knn(Q, T, k, exclude_self)
    assert ind.dtype == np.int64 and dist.dtype == np.float64 and ind.shape == want_ind.shape == dist.shape
    assert np.array_equal(ind, want_ind), f"{what}: {np.count_nonzero(ind != want_ind)} indices differ"
    err = np.abs(dist - want_dist)
    assert (err <= 2.0 * (d + 4) * U53 * want_dist).all(), f"{what}: worst error / bound = {(err / (2.0 * (d + 4) * U53 * want_dist + 1e-300)).max():.3g}"


def _all_slices(nn, Xq, k, what, slices=SLICES):
    """kneighbors for every forced slice count and a repeat of the first: all torch.equal; returns the first as numpy."""
    first = None
    for s in tuple(slices) + (slices[0],):
        dist, ind = nn.kneighbors(Xq, k, slices=s) if Xq is not None else map(torch.from_numpy, nn.kneighbors(None, k, slices=s))
        if first is None:
            first = (dist, ind)
        else:
            assert torch.equal(dist, first[0]) and torch.equal(ind, first[1]), f"{what}: slices {s} differs from slices {slices[0]}"
    return first[0].cpu().numpy(), first[1].cpu().numpy()


@pytest.mark.parametrize("d", DS)
def test_search_against_oracle(dev, d):
    di = DS.index(d)
    for i, (m, n) in enumerate(itertools.product(MS, NS)):
        k = KS[(i + di) % 4]
        n = k if n == "k" else n
        qdt, tdt = DTYPES[(i // 4 + di) % 4]
        Q, T = _pool()["q"][:m, :d], _pool()["t"][:n, :d]
        Qd, Td = _pool_dev()["q", qdt][:m, :d], _pool_dev()["t", tdt][:n, :d]
        assert d == POOL_D or Td.stride(0) == POOL_D
        what = f"m {m} n {n} d {d} k {k} {qdt}/{tdt}"
        nn = NearestNeighbors(k).fit(Td)
        dist, ind = _all_slices(nn, Qd, k, what)
        _check(dist, ind, Q, T, k, what)


def test_large_mean(dev):
    """T = 1e6 + 1e-3 randn: an uncentred expansion is wrong by ~1 against squared distances of ~1e-4; centring at staging passes."""
    rs = np.random.RandomState(5)
    T, Q = 1e6 + 1e-3 * rs.randn(300, 50), 1e6 + 1e-3 * rs.randn(70, 50)
    nn = NearestNeighbors(7).fit(T)
    for s in (0, 2):
        dist, ind = nn.kneighbors(Q, slices=s)
        _check(dist, ind, Q, T, 7, f"large mean, slices {s}")


@functools.lru_cache(maxsize=None)
def _duplicated():
    H = make_points(150, 20, 21)
    return H, np.concatenate([H, H]), np.concatenate([H[:40], make_points(25, 20, 22)])


@pytest.mark.parametrize("k", [3, 4, 7])
def test_duplicates_and_exact_ties(dev, k):
    H, T, Q = _duplicated()
    nn = NearestNeighbors(k).fit(T)
    dist, ind = _all_slices(nn, torch.from_numpy(Q).cuda(), k, f"duplicates k {k}", slices=(1, 2, 7))
    want_dist, want_ind, _ = knn(Q, T, k)
    assert np.array_equal(ind, want_ind)
    for j in range(0, k - 1, 2):                     # pairs (i, i + 150), in that order, at equal distance
        assert (ind[:, j] < 150).all() and np.array_equal(ind[:, j + 1], ind[:, j] + 150) and np.array_equal(dist[:, j], dist[:, j + 1])
    if k % 2:
        assert (ind[:, k - 1] < 150).all()           # the last slot holds the lower index of its pair
    assert np.array_equal(ind[:40, 0], np.arange(40)) and (dist[:40, 0] == 0.0).all() and (dist[:40, 1] == 0.0).all()
    assert (dist[40:, 0] > 0.0).all()
    assert (np.abs(dist - want_dist) <= 2.0 * 24 * U53 * want_dist).all()


@pytest.mark.parametrize("n", [65, 333])
def test_kneighbors_of_the_training_rows(dev, n):
    T = _pool()["t"][:n, :100]
    nn = NearestNeighbors(5).fit(_pool_dev()["t", "f64"][:n, :100])
    dist, ind = _all_slices(nn, None, 5, f"X=None n {n}")
    assert isinstance(nn.kneighbors()[0], np.ndarray)
    _check(dist, ind, T, T, 5, f"X=None n {n}", exclude_self=True)
    assert (ind != np.arange(n)[:, None]).all()


def test_kneighbors_of_a_duplicated_training_set(dev):
    _, T, _ = _duplicated()
    dist, ind = NearestNeighbors(3).fit(T).kneighbors()
    twin = (np.arange(300) + 150) % 300
    assert np.array_equal(ind[:, 0], twin) and (dist[:, 0] == 0.0).all() and (dist[:, 1] > 0.0).all()
    want_dist, want_ind, _ = knn(T, T, 3, exclude_self=True)
    assert np.array_equal(ind, want_ind)


@functools.lru_cache(maxsize=None)
def _labelled(n_classes, sep=10.0):
    """600 x 100 training rows and 200 queries: make_points plus `sep` times a unit direction per class.  At sep = 10 the classes mix in
    some neighbourhoods (probabilities strictly between 0 and 1 occur) yet scikit-learn's own vote is nowhere tied: its top two
    probabilities differ by >= 0.33 (binary) / 0.13 (three classes) over k in {3, 5, 7} and both weightings."""
    rs = np.random.RandomState(33)
    y, yq = rs.randint(0, n_classes, 600), rs.randint(0, n_classes, 200)
    v = rs.randn(n_classes, 100)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    X, Q = make_points(600, 100, 31) + sep * v[y], make_points(200, 100, 32) + sep * v[yq]
    return X.astype(np.float32).astype(np.float64), y, Q.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n_classes", [2, 3])
def test_classifier_against_sklearn(dev, n_classes):
    from sklearn.neighbors import KNeighborsClassifier as SkKNN
    X, y, Q = _labelled(n_classes)
    labels = np.array(["a", "b", "c"])[y] if n_classes == 3 else y          # any sortable labels
    for k, weights in itertools.product((3, 5, 7), ("uniform", "distance")):
        sk = SkKNN(k, weights=weights, algorithm="brute").fit(X, labels)
        want = sk.predict_proba(Q)
        top2 = np.sort(want, axis=1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0] > 1e-9).all(), "the test's inputs leave scikit-learn's own vote tied"
        clf = KNeighborsClassifier(k, weights=weights).fit(X, labels)
        assert np.array_equal(clf.classes_, sk.classes_)
        got = clf.predict_proba(Q)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, f"k {k} {weights}: {np.abs(got - want).max():.3g}"
        assert np.array_equal(clf.predict(Q), sk.predict(Q))
        assert torch.equal(clf.predict_proba(torch.from_numpy(Q).cuda()).cpu(), torch.from_numpy(got))


def test_classifier_query_equal_to_a_training_row(dev):
    X, y, Q = _labelled(3)
    Q = np.concatenate([X[17:18], Q[:3]])
    clf = KNeighborsClassifier(5, weights="distance").fit(X, y)
    p = clf.predict_proba(Q)
    onehot = np.zeros(3)
    onehot[y[17]] = 1.0
    assert np.array_equal(p[0], onehot) and clf.predict(Q)[0] == y[17]
    assert (p[1:] < 1.0).any(axis=1).all() and np.abs(p.sum(axis=1) - 1.0).max() <= 1e-15


def test_grid_search_cv_against_sklearn(dev):
    from sklearn.model_selection import GridSearchCV
    from sklearn.neighbors import KNeighborsClassifier as SkKNN
    X, y, _ = _labelled(2, 6.0)                      # closer classes: the grid points score differently
    X, y = X[:400], y[:400]
    grid = {"n_neighbors": [3, 5, 7], "weights": ["uniform", "distance"]}
    sk = GridSearchCV(SkKNN(algorithm="brute"), grid, cv=5, scoring="f1").fit(X, y)
    best, scores, fitted = grid_search_cv(X, y, grid, cv=5)
    want = sk.cv_results_["mean_test_score"]
    assert [dict(p) for p in sk.cv_results_["params"]] == [dict(zip(sorted(grid), v)) for v in itertools.product(*(grid[k] for k in sorted(grid)))]
    assert np.abs(np.asarray(scores) - want).max() <= 1e-12
    assert best == sk.cv_results_["params"][int(np.argmax(want))]
    assert fitted.n_neighbors == best["n_neighbors"] and fitted.weights == best["weights"] and fitted.n_samples_fit_ == 400


def test_contract(dev):
    T, Q = _pool()["t"][:333, :17], _pool()["q"][:65, :17]
    nn = NearestNeighbors(4).fit(T)
    dist, ind = nn.kneighbors(Q)
    assert isinstance(dist, np.ndarray) and dist.shape == (65, 4) and ind.dtype == np.int64
    assert np.array_equal(nn.kneighbors(Q, return_distance=False), ind)
    assert nn.mean_.shape == (17,) and np.abs(nn.mean_ - T.mean(axis=0)).max() <= 1e-13
    # non-contiguous input: the same bits as its contiguous copy
    Qt = torch.from_numpy(np.ascontiguousarray(Q.T)).cuda().t()
    assert not Qt.is_contiguous()
    d2, i2 = nn.kneighbors(Qt)
    assert d2.is_cuda and torch.equal(d2.cpu(), torch.from_numpy(dist)) and torch.equal(i2.cpu(), torch.from_numpy(ind))
    nn_t = NearestNeighbors(4).fit(torch.from_numpy(np.ascontiguousarray(T.T)).cuda().t())
    d3, i3 = nn_t.kneighbors(Q)
    assert np.array_equal(d3, dist) and np.array_equal(i3, ind)
    # float32 input: the same indices as its float64 cast
    i32 = NearestNeighbors(4).fit(T.astype(np.float32)).kneighbors(Q.astype(np.float32), return_distance=False)
    assert np.array_equal(i32, ind)
    # non-finite input
    for bad in (np.nan, np.inf, -np.inf):
        Tb, Qb = T.copy(), Q.copy()
        Tb[200, 5], Qb[64, 16] = bad, bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            NearestNeighbors(4).fit(Tb)
        with pytest.raises(ValueError, match="NaN or infinity"):
            nn.kneighbors(Qb)
    # feature mismatch and n_neighbors limits
    with pytest.raises(ValueError, match="features"):
        nn.kneighbors(_pool()["q"][:5, :16])
    with pytest.raises(ValueError, match="n_neighbors"):
        nn.kneighbors(Q, 33)
    with pytest.raises(ValueError, match="n_neighbors"):
        nn.kneighbors(Q, 0)
    small = NearestNeighbors(3).fit(T[:3])
    assert small.kneighbors(Q)[1].shape == (65, 3)
    with pytest.raises(ValueError, match="exceeds"):
        small.kneighbors(Q, 4)
    with pytest.raises(ValueError, match="exceeds"):
        small.kneighbors()                            # X=None leaves n - 1 = 2 candidates
    assert small.kneighbors(None, 2)[1].shape == (3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nn.kneighbors(torch.zeros(2, 17))
