"""GPU: imbalance.SMOTE, TomekLinks and SMOTETomek equal the numpy restatement (tests/smote_numpy.py) bit for bit -- ``X_res`` compared as
integers, ``y_res``, ``sample_indices_`` -- in float64 and float32, at the synthesis kernel's edges, for every kind of input.

The GPU search selects with a centred expansion, unique only where ``knn_oracle.min_gap_over_bound > 1``; every comparison below asserts
that on the CPU first (``S.gap``), for the class searches at k and for the 1-NN search on the set Tomek sees.  A Tomek comparison also
asserts that its set holds links, so that it cannot pass vacuously."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import smote_numpy as S
from bbbp_amd import imbalance

pytestmark = pytest.mark.gpu

K, SEED = 5, 42
DTYPES = ["float64", "float32"]
CANARY = (300, 17, 100, 3)
# (n, d, n_min, seed, k, strategy): d = 1; one element past a wave-wide chunk and past two; a single synthetic row; one wave past 64 work-groups
# of four; a class of k + 1 rows, where every other row is a neighbour; the search's smallest and largest k
EDGES = [(65, 1, 7, 1, 5, "auto"), (80, 65, 20, 1, 5, "auto"), (80, 130, 20, 2, 5, "auto"), (65, 3, 7, 1, 5, {1: 8}), (297, 4, 20, 6, 5, "auto"),
         (65, 3, 6, 1, 5, "auto"), (130, 5, 40, 2, 1, "auto"), (130, 5, 40, 2, 32, "auto")]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@functools.lru_cache(maxsize=None)
def _reference(p, dtype):
    """Problem, restatement results and preconditions, computed once per (problem, dtype) and left unchanged."""
    X, y = S.problem(*p, dtype=dtype)
    smote = S.smote(X, y, K, SEED)
    ref = dict(X=X, y=y, smote=smote, tomek=S.tomek(X, y, "auto"), smote_tomek=S.smote_tomek(X, y, K, SEED),
               gap_class=S.gap(X[y == 1], K), gap_all=S.gap(X, 1), gap_res=S.gap(smote[0], 1),
               links=int(S.tomek_members(X, y).sum()), links_res=int(S.tomek_members(*smote).sum()))
    for a in (*smote, *ref["tomek"], *ref["smote_tomek"]):               # (X and y stay writable: torch warns about read-only arrays)
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("p", S.PROBLEMS[:4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_smote_tomeklinks_and_smotetomek_equal_the_restatement(dev, p, dtype):
    r = _reference(p, dtype)
    assert r["gap_class"] > 1 and r["gap_all"] > 1 and r["gap_res"] > 1 and r["links"] > 0 and r["links_res"] > 0
    X_res, y_res = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(r["X"], r["y"])
    assert _same(X_res, r["smote"][0]) and _same(y_res, r["smote"][1])
    tl = imbalance.TomekLinks(device=dev)
    X_res, y_res = tl.fit_resample(r["X"], r["y"])
    assert _same(X_res, r["tomek"][0]) and _same(y_res, r["tomek"][1]) and _same(tl.sample_indices_, r["tomek"][2].astype(np.int64))
    assert len(y_res) == len(r["y"]) - int((S.tomek_members(r["X"], r["y"]) & (r["y"] == 0)).sum()) < len(r["y"])
    X_res, y_res = imbalance.SMOTETomek(random_state=SEED, device=dev).fit_resample(r["X"], r["y"])
    assert _same(X_res, r["smote_tomek"][0]) and _same(y_res, r["smote_tomek"][1])
    assert len(y_res) == len(r["smote"][1]) - r["links_res"]


@pytest.mark.parametrize("n,d,n_min,seed,k,strategy", EDGES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_at_the_synthesis_kernels_edges(dev, n, d, n_min, seed, k, strategy, dtype):
    X, y = S.problem(n, d, n_min, seed, dtype=dtype)
    assert S.gap(X[y == 1], k) > 1
    want = S.smote(X, y, k, SEED, strategy)
    assert len(want[1]) - n == (1 if isinstance(strategy, dict) else n - 2 * n_min)              # 1, or 257 for (297, 4, 20)
    X_res, y_res = imbalance.SMOTE(strategy, random_state=SEED, k_neighbors=k, device=dev).fit_resample(X, y)
    assert _same(X_res, want[0]) and _same(y_res, want[1])


def _fused(X, y, k, seed):
    """The synthetic rows of S.smote for float64 ``X`` with the product and the sum fused: a + s * t rounded once (exact rational
    arithmetic, one correctly rounded conversion), t = fl(b - a)."""
    record = []
    S.smote(X, y, k, seed, record=record)
    (c, rows, nbrs, steps), = record
    Xc = X[y == c]
    a, t = Xc[rows], Xc[nbrs] - Xc[rows]
    out = np.empty_like(a)
    for j in range(a.shape[0]):
        s = Fraction(float(steps[j]))
        for col in range(a.shape[1]):
            out[j, col] = float(Fraction(float(a[j, col])) + s * Fraction(float(t[j, col])))
    return out


def test_contraction_canary_a_fused_multiply_add_would_change_the_bits(dev):
    """Precondition: on this problem the fused form differs from the restatement, so bit equality of the GPU result shows that the kernel
    does not contract the product and the sum."""
    r = _reference(CANARY, "float64")
    n = len(r["y"])
    fused = _fused(r["X"], r["y"], K, SEED)
    differing = int((_bits(fused) != _bits(r["smote"][0][n:])).sum())
    assert differing > 0
    assert np.abs(fused - r["smote"][0][n:]).max() <= 2.0 ** -52 * np.abs(r["X"]).max()          # and by no more than a last bit
    assert r["gap_class"] > 1
    X_res, _ = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(r["X"], r["y"])
    assert _same(X_res, r["smote"][0])


def test_float32_rows_round_the_difference_first(dev):
    """numpy rounds the float32 difference before widening it: the result differs from the expression evaluated in float64 throughout and
    rounded once, and the GPU equals the former."""
    r = _reference(CANARY, "float32")
    X, y = r["X"], r["y"]
    n = len(y)
    record = []
    S.smote(X, y, K, SEED, record=record)
    (c, rows, nbrs, steps), = record
    Xc = X[y == c].astype(np.float64)
    all_in_float64 = (Xc[rows] + steps[:, None] * (Xc[nbrs] - Xc[rows])).astype(np.float32)
    assert int((_bits(all_in_float64) != _bits(r["smote"][0][n:])).sum()) > 0
    assert r["gap_class"] > 1
    X_res, _ = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(X, y)
    assert _same(X_res, r["smote"][0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kinds_of_input_and_output(dev, dtype):
    p = S.PROBLEMS[1]
    r = _reference(p, dtype)
    X, y = r["X"], r["y"]
    n, d = X.shape
    assert r["gap_class"] > 1 and r["gap_all"] > 1 and r["gap_res"] > 1 and r["links_res"] > 0
    # a CUDA tensor in, a CUDA tensor out on the same device
    Xt = torch.from_numpy(np.array(X)).to(dev)
    for est, want in ((imbalance.SMOTE(random_state=SEED, device=dev), r["smote"]), (imbalance.SMOTETomek(random_state=SEED, device=dev), r["smote_tomek"]),
                      (imbalance.TomekLinks(device=dev), r["tomek"])):
        X_res, y_res = est.fit_resample(Xt, y)
        assert isinstance(X_res, torch.Tensor) and X_res.device == Xt.device and isinstance(y_res, np.ndarray)
        assert _same(X_res.cpu().numpy(), want[0]) and _same(y_res, want[1])
    # a column slice of a wider matrix and a row slice of a longer one, used in place
    wide = torch.full((n + 9, d + 8), 7.0, dtype=Xt.dtype, device=dev)
    wide[4:4 + n, 3:3 + d] = Xt
    for view in (wide[4:4 + n, 3:3 + d], wide[4:4 + n][:, 3:3 + d]):
        assert view.stride(0) == d + 8 and not view.is_contiguous()
        X_res, y_res = imbalance.SMOTETomek(random_state=SEED, device=dev).fit_resample(view, y)
        assert X_res.is_contiguous() and _same(X_res.cpu().numpy(), r["smote_tomek"][0]) and _same(y_res, r["smote_tomek"][1])
    long_ = torch.cat([Xt[:3], Xt, Xt[:2]])
    X_res, y_res = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(long_[3:3 + n], y)
    assert _same(X_res.cpu().numpy(), r["smote"][0])
    assert bool((wide[:4] == 7).all()) and bool((wide[:, :3] == 7).all()) and bool((wide[:, 3 + d:] == 7).all()) and bool((wide[4 + n:] == 7).all())
    # string labels come back as strings
    names = np.array(["BBB-", "BBB+"])
    X_res, y_res = imbalance.SMOTETomek(random_state=SEED, device=dev).fit_resample(X, names[y])
    assert y_res.dtype == names.dtype and _same(X_res, r["smote_tomek"][0]) and np.array_equal(y_res, names[r["smote_tomek"][1]])
    X_res, y_res = imbalance.SMOTE({"BBB+": 77}, random_state=SEED, device=dev).fit_resample(X, names[y])
    want = S.smote(X, y, K, SEED, {1: 77})
    assert _same(X_res, want[0]) and np.array_equal(y_res, names[want[1]])
    # a float ratio
    X_res, y_res = imbalance.SMOTE(0.8, random_state=SEED, device=dev).fit_resample(X, y)
    want = S.smote(X, y, K, SEED, 0.8)
    assert np.bincount(y_res).tolist() == [90, 72] and _same(X_res, want[0]) and _same(y_res, want[1])


def test_balanced_input_returns_a_copy_and_launches_nothing(dev):
    """The matrix holds NaN: any search would raise."""
    X, y = S.problem(64, 3, 32, 1)
    X = np.array(X)
    X[5, 1] = np.nan
    before = dict(imbalance._LAUNCHES)
    X_res, y_res = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(X, y)
    assert X_res is not X and y_res is not y and _same(X_res, X) and _same(y_res, y)
    Xt = torch.from_numpy(X).to(dev)
    X_res, y_res = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(Xt, y)
    assert X_res.data_ptr() != Xt.data_ptr() and X_res.device == Xt.device and _same(X_res.cpu().numpy(), X) and _same(y_res, y)
    assert imbalance._LAUNCHES == before
    # an imbalanced matrix with the NaN in a class that is not resampled raises the search's error
    y2 = np.array(y)
    y2[np.flatnonzero(y == 1)[:10]] = 0
    y2[5] = 0
    for est in (imbalance.SMOTE(random_state=SEED, device=dev), imbalance.SMOTETomek(random_state=SEED, device=dev), imbalance.TomekLinks(device=dev)):
        with pytest.raises(ValueError, match="NaN or infinity"):
            est.fit_resample(X, y2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_classes(dev, dtype):
    X, y = S.problem3(*CANARY, dtype=dtype)
    assert np.bincount(y).tolist() == [180, 100, 20]
    for c in (1, 2):
        assert S.gap(X[y == c], K) > 1
    want = S.smote(X, y, K, SEED)
    assert np.bincount(want[1]).tolist() == [180, 180, 180]
    X_res, y_res = imbalance.SMOTE(random_state=SEED, device=dev).fit_resample(X, y)
    assert _same(X_res, want[0]) and _same(y_res, want[1])
    # a RandomState instance runs on through the classes
    want_rs = S.smote(X, y, K, np.random.RandomState(SEED))
    assert not _same(want_rs[0], want[0])
    X_res, y_res = imbalance.SMOTE(random_state=np.random.RandomState(SEED), device=dev).fit_resample(X, y)
    assert _same(X_res, want_rs[0]) and _same(y_res, want_rs[1])
    # "minority" resamples the smallest class only; SMOTETomek cleans every class
    want_min = S.smote(X, y, K, SEED, "minority")
    X_res, y_res = imbalance.SMOTE("minority", random_state=SEED, device=dev).fit_resample(X, y)
    assert np.bincount(y_res).tolist() == [180, 100, 180] and _same(X_res, want_min[0]) and _same(y_res, want_min[1])
    assert S.gap(want[0], 1) > 1 and int(S.tomek_members(*want).sum()) > 0
    X_res, y_res = imbalance.SMOTETomek(random_state=SEED, device=dev).fit_resample(X, y)
    want_st = S.smote_tomek(X, y, K, SEED)
    assert _same(X_res, want_st[0]) and _same(y_res, want_st[1])


def test_an_index_outside_its_array_yields_nan_and_reads_nothing(dev):
    Xc = torch.arange(24, dtype=torch.float64, device=dev).reshape(8, 3)
    nn = torch.tensor([[(r + 1) % 8, (r + 2) % 8] for r in range(8)], dtype=torch.int64, device=dev)
    nn[2, 1] = 8
    nn[3, 0] = -1
    idx = torch.tensor([0, -1, 16, 5, 6, 2 ** 40], dtype=torch.int64, device=dev)
    steps = torch.full((6,), 0.5, dtype=torch.float64, device=dev)
    out = torch.zeros((6, 3), dtype=torch.float64, device=dev)
    imbalance._synthesize(Xc, nn, idx, steps, out)
    got = out.cpu().numpy()
    assert np.isnan(got[[1, 2, 3, 4, 5]]).all()                          # idx below 0, past n_c k; nn past n_c, below 0; idx far past
    assert np.array_equal(got[0], [1.5, 2.5, 3.5])                       # row 0 towards row 1
