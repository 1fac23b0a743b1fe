"""CPU: the kNN oracle is pinned to scikit-learn's brute-force search; the search's workspace query, every entry point's argument
checks and neighbors' Python argument handling work without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from bbbp_amd import _lib
from knn_oracle import knn, make_points, min_gap_over_bound

ERR_ARG = 1
SHAPES = [(1000, 300, 100), (333, 77, 167), (65, 130, 3), (4097, 64, 100)]      # (n, m, d)


@pytest.mark.parametrize("n,m,d", SHAPES)
def test_oracle_equals_sklearn_brute(n, m, d):
    from sklearn.neighbors import NearestNeighbors as SkNN
    T, Q = make_points(n, d, 1), make_points(m, d, 2)
    dist, ind, _ = knn(Q, T, 7)
    sk_dist, sk_ind = SkNN(n_neighbors=7, algorithm="brute").fit(T).kneighbors(Q)
    assert np.array_equal(ind, sk_ind)
    assert (np.abs(dist - sk_dist) <= 1e-13 * dist).all()
    ratio = min_gap_over_bound(Q, T, 7).min()
    print(f"n {n} m {m} d {d}: smallest gap / B = {ratio:.3g}")
    assert ratio >= 1e7


def _desc(**kw):
    base = dict(m=130, n=1000, d=100, k=7, q_dtype=0, t_dtype=1, ldq=100, ldt=100, exclude_self=0, slices=0)
    base.update(kw)
    return _lib.KnnDesc(**base)


def test_knn_workspace_bytes_without_gpu():
    L = _lib.lib()
    ws = lambda **kw: L.bbbp_knn_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert ws(slices=7) == 7 * 130 * 7 * (8 + 4)            # [S][m][k] squared distances + indices
    assert ws(slices=2, m=1, k=32) == 2 * 1 * 32 * 12
    assert ws(slices=1) == 0
    assert ws(m=1 << 20, n=10000) == 0                      # 16384 query tiles fill the chip: one slice
    few = ws(m=64, n=10000)                                 # one query tile: the training rows are cut up
    assert few > 0 and few % (64 * 7 * 12) == 0 and few // (64 * 7 * 12) <= 10000 // 256
    assert ws(m=64, n=300) == 0                             # too few training rows for a second slice
    for bad, word in ((dict(k=0), b"k 0"), (dict(k=33), b"k 33"), (dict(n=5), b"exceeds"), (dict(q_dtype=2), b"dtype"), (dict(t_dtype=-1), b"dtype"),
                      (dict(slices=65), b"slices"), (dict(m=0), b"positive"), (dict(exclude_self=1), b"exclude_self"),
                      (dict(exclude_self=1, m=7, n=7), b"exceeds")):
        assert ws(**bad) == 0 and word in L.bbbp_last_error(), bad


def test_knn_entry_points_validate_before_touching_the_gpu():
    L = _lib.lib()
    fake = 4096                                              # never dereferenced: validation comes first
    ptrs = dict(Q=fake, T=fake, q_norm=fake, t_norm=fake, dist=fake, ind=fake)
    run = lambda **kw: L.bbbp_knn_f64(None, ctypes.byref(_desc(**{**ptrs, **kw})), None, 0)  # noqa: E731
    for bad, word in ((dict(k=0), b"k 0"), (dict(k=33), b"k 33"), (dict(k=8, n=7), b"exceeds"), (dict(q_dtype=5), b"dtype"), (dict(Q=None), b"null"),
                      (dict(t_norm=None), b"null"), (dict(ind=None), b"null"), (dict(ldt=99), b"leading"),
                      (dict(exclude_self=1, m=1000, T=8192), b"exclude_self"), (dict(exclude_self=1), b"exclude_self"),
                      (dict(exclude_self=1, m=1000, t_dtype=0, ldt=101), b"exclude_self")):
        assert run(**bad) == ERR_ARG and word in L.bbbp_last_error(), bad
    assert L.bbbp_knn_f64(None, None, None, 0) == ERR_ARG
    assert run(slices=3) == 3 and b"workspace" in L.bbbp_last_error()          # BBBP_ERR_WORKSPACE, still before any HIP call
    # row norms
    assert L.bbbp_knn_row_norms(None, None, 0, 4, 4, 4, None, fake, fake) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert L.bbbp_knn_row_norms(None, fake, 0, 4, 4, 4, None, fake, None) == ERR_ARG
    assert L.bbbp_knn_row_norms(None, fake, 3, 4, 4, 4, None, fake, fake) == ERR_ARG and b"dtype" in L.bbbp_last_error()
    assert L.bbbp_knn_row_norms(None, fake, 0, 4, 4, 3, None, fake, fake) == ERR_ARG
    assert L.bbbp_knn_row_norms(None, fake, 0, 0, 4, 4, None, fake, fake) == ERR_ARG
    # vote
    vote = lambda m=4, k=7, kk=7, n=9, nc=2, w=0, dist=fake, labels=fake: L.bbbp_knn_vote(None, dist, fake, m, k, kk, labels, n, nc, w, fake, fake)  # noqa: E731
    assert vote(dist=None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert vote(labels=None) == ERR_ARG
    assert vote(k=0, kk=0) == ERR_ARG and vote(k=33, kk=3) == ERR_ARG and vote(kk=8) == ERR_ARG and vote(kk=0) == ERR_ARG
    assert b"kk" in L.bbbp_last_error()
    assert vote(nc=33) == ERR_ARG and b"n_classes" in L.bbbp_last_error()
    assert vote(nc=0) == ERR_ARG and vote(w=2) == ERR_ARG and b"weights" in L.bbbp_last_error()
    assert vote(m=0) == ERR_ARG and vote(n=0) == ERR_ARG


def test_neighbors_argument_handling():
    from bbbp_amd.neighbors import KNeighborsClassifier, NearestNeighbors, grid_search_cv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NearestNeighbors(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KNeighborsClassifier(3, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NearestNeighbors(3).fit(torch.zeros(8, 4))
    for k in (0, 33, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="n_neighbors"):
            NearestNeighbors(k)
    for kw in (dict(weights="rank"), dict(weights=None), dict(metric="manhattan"), dict(p=1), dict(algorithm="kd_tree"), dict(radius=1.0)):
        with pytest.raises(ValueError):
            KNeighborsClassifier(3, **kw)
    with pytest.raises(ValueError):
        NearestNeighbors(3, radius=2.0)
    with pytest.raises(RuntimeError, match="not fitted"):
        NearestNeighbors(3).kneighbors(np.zeros((2, 4)))
    with pytest.raises(RuntimeError, match="not fitted"):
        KNeighborsClassifier(3).predict(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="classes"):
        KNeighborsClassifier(3).fit(np.zeros((40, 2)), np.arange(40))
    with pytest.raises(ValueError, match="1-D"):
        KNeighborsClassifier(3).fit(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="grid keys"):
        grid_search_cv(np.zeros((10, 2)), np.zeros(10), {"n_neighbors": [3], "p": [1]})
    with pytest.raises(ValueError, match="n_neighbors"):
        grid_search_cv(np.zeros((10, 2)), np.zeros(10), {"n_neighbors": [3, 40]})
    assert not hasattr(NearestNeighbors, "radius_neighbors")
