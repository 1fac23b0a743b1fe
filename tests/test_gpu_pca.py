"""GPU: the float64 centred product (bbbp_gemm_f64c) against numpy float64 at the standard summation bound, and decomposition.PCA
against the exact (centred SVD) oracle of tests/pca_oracle.py, through to the shipped PCA-fusion weights."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from bbbp_amd import mlp
from bbbp_amd.decomposition import PCA, gemm_f64c
from helpers import GOLDEN, assert_close
from pca_oracle import SHAPES, make_matrix, pca_full, transform

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SIZES = (1, 15, 17, 64, 65, 130)
KS = (1, 3, 4, 5, 63, 65, 1000)
SPLITS = (0, 1, 2, 7)
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}


@functools.lru_cache(maxsize=None)
def _pool():
    """Host operands, drawn once: k-contiguous [130, 1000] and k-major [1000, 130] pools in both dtypes, shift and scale vectors."""
    rs = np.random.RandomState(7)
    p = {"nt64": rs.randn(2, 130, 1000), "tn64": rs.randn(2, 1000, 130)}
    p["nt32"], p["tn32"] = p["nt64"].astype(np.float32), p["tn64"].astype(np.float32)
    p["shift"] = rs.randn(2, 1000)
    p["scale"] = rs.randn(130) + 2.0
    return p


@functools.lru_cache(maxsize=None)
def _pool_dev():
    return {k: torch.from_numpy(v).cuda() for k, v in _pool().items()}


def _operands(layout, which, dtype, M_or_N, K):
    """(device view, host float64 [rows, K]) of operand `which` (0 = A, 1 = B): a slice of the pool, so the leading dimension is the pool's."""
    key = ("nt" if layout == "NT" else "tn") + ("32" if dtype == "f32" else "64")
    if layout == "NT":
        return _pool_dev()[key][which, :M_or_N, :K], _pool()[key][which, :M_or_N, :K].astype(np.float64)
    return _pool_dev()[key][which, :K, :M_or_N], _pool()[key][which, :K, :M_or_N].astype(np.float64).T


def _shift(layout, which, on, extent, K):
    if not on:
        return None, 0.0
    n = K if layout == "NT" else extent
    host = _pool()["shift"][which, :n]
    dev = _pool_dev()["shift"][which, :n].contiguous()
    return dev, (host[None, :] if layout == "NT" else host[:, None])


def _check(got, Ac, Bc, K, scale=None, out32=False, what=""):
    """|got - want| <= 2 K 2^-53 (|A - sa| |B - sb|^T) elementwise (+ one rounding of the result where a row scale multiplies it, + one float32 ulp
    for a float32 result): the standard bound of a K-term sum, whatever the order on either side."""
    want = Ac @ Bc.T
    bound = 2.0 * K * U53 * (np.abs(Ac) @ np.abs(Bc).T)
    if scale is not None:
        want, bound = want * scale[:, None], bound * np.abs(scale)[:, None]
        bound = bound + U53 * np.abs(want)                  # the epilogue multiply rounds once more
    if out32:
        bound = bound + 2.0 ** -23 * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    assert got.shape == want.shape and (err <= bound).all(), f"{what}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}"


@pytest.mark.parametrize("layout", ["NT", "TN"])
@pytest.mark.parametrize("adt,bdt", [("f32", "f32"), ("f64", "f64"), ("f32", "f64"), ("f64", "f32")])
def test_gemm_f64c_against_numpy(dev, layout, adt, bdt):
    modes = [(1, 1), (0, 0), (1, 0), (0, 1)]
    for i, (M, N, K) in enumerate(itertools.product(SIZES, SIZES, KS)):
        # K has period 7 in i: the split count (period 4) and the shift mode (period 16) meet every K, also K < the slab count
        split, (sa_on, sb_on), use_scale, out32 = SPLITS[i % 4], modes[(i // 4) % 4], i % 3 == 1, i % 5 in (2, 4)
        A, Ah = _operands(layout, 0, adt, M, K)
        B, Bh = _operands(layout, 1, bdt, N, K)
        sa, sah = _shift(layout, 0, sa_on, M, K)
        sb, sbh = _shift(layout, 1, sb_on, N, K)
        scale = _pool_dev()["scale"][:M].contiguous() if use_scale else None
        kw = dict(layout=layout, a_shift=sa, b_shift=sb, row_scale=scale, out_dtype=torch.float32 if out32 else torch.float64, split_k=split)
        got = gemm_f64c(A, B, **kw)
        assert got.dtype == kw["out_dtype"]
        _check(got.cpu().numpy(), Ah - sah, Bh - sbh, K, _pool()["scale"][:M] if use_scale else None, out32,
               f"{layout} {adt}x{bdt} M{M} N{N} K{K} shifts {sa_on}{sb_on} scale {use_scale} out32 {out32} split {split}")
        if i % 5 == 0:
            assert torch.equal(got, gemm_f64c(A, B, **kw)), "two identical calls differ"


@pytest.mark.parametrize("layout", ["NT", "TN"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_gemm_f64c_symmetric(dev, layout, dt):
    for M, K, split in itertools.product(SIZES, KS, SPLITS):
        A, Ah = _operands(layout, 0, dt, M, K)
        s, sh = _shift(layout, 0, True, M, K)
        sym = gemm_f64c(A, A, layout=layout, a_shift=s, b_shift=s, symmetric=True, split_k=split)
        assert torch.equal(sym, sym.T), f"{layout} {dt} M{M} K{K} split {split}: not bitwise symmetric"
        assert torch.equal(sym, gemm_f64c(A, A, layout=layout, a_shift=s, b_shift=s, symmetric=True, split_k=split))
        what = f"symmetric {layout} {dt} M{M} K{K} split {split}"
        _check(sym.cpu().numpy(), Ah - sh, Ah - sh, K, what=what)
        full = gemm_f64c(A, A, layout=layout, a_shift=s, b_shift=s, symmetric=False, split_k=split).cpu().numpy()
        bound = 2.0 * K * U53 * (np.abs(Ah - sh) @ np.abs(Ah - sh).T)
        assert (np.abs(sym.cpu().numpy() - full) <= bound).all(), what + " against the non-symmetric call"
    out32 = gemm_f64c(A, A, layout=layout, symmetric=True, out_dtype=torch.float32)
    assert out32.dtype == torch.float32 and torch.equal(out32, out32.T)
    _check(out32.cpu().numpy(), Ah, Ah, K, out32=True, what="symmetric float32 output")


@pytest.mark.parametrize("layout", ["NT", "TN"])
def test_gemm_f64c_long_k(dev, layout):
    """M = N = 17, K = 49 152 (the image width): many chunks per slab, the plan's own slab count and a forced odd one."""
    K = 49152
    rs = np.random.RandomState(11)
    Ah, Bh, sh = rs.randn(17, K).astype(np.float32), rs.randn(17, K), rs.randn(K)
    A = torch.from_numpy(Ah if layout == "NT" else np.ascontiguousarray(Ah.T)).to(dev)
    B = torch.from_numpy(Bh if layout == "NT" else np.ascontiguousarray(Bh.T)).to(dev)
    if layout == "NT":
        sa = sb = torch.from_numpy(sh).to(dev)
        Ac, Bc = Ah.astype(np.float64) - sh, Bh - sh
    else:
        sa, sb = torch.from_numpy(sh[:17].copy()).to(dev), torch.from_numpy(sh[17:34].copy()).to(dev)
        Ac, Bc = Ah.astype(np.float64) - sh[:17, None], Bh - sh[17:34, None]
    for split in (0, 7):
        got = gemm_f64c(A, B, layout=layout, a_shift=sa, b_shift=sb, split_k=split)
        _check(got.cpu().numpy(), Ac, Bc, K, what=f"long K {layout} split {split}")
        assert torch.equal(got, gemm_f64c(A, B, layout=layout, a_shift=sa, b_shift=sb, split_k=split))


def test_gemm_f64c_large_mean_is_centred_in_float64(dev):
    """float32 X = 1000 + 0.01 randn with shift = column mean: the bound is the CENTRED one, 2 K u |Xc|^T |Xc| -- a float32 subtraction
    (error 6e-5 per element against a spread of 0.01) or the X^T X - n mu mu^T shortcut (cancellation at 1e6 against 1e-4) misses it
    by many orders."""
    rs = np.random.RandomState(3)
    X = (1000.0 + 0.01 * rs.randn(130, 65)).astype(np.float32)
    mu = X.astype(np.float64).mean(axis=0)
    Xc = X.astype(np.float64) - mu
    Xd, mud = torch.from_numpy(X).to(dev), torch.from_numpy(mu).to(dev)
    for split in (0, 2):
        cov = gemm_f64c(Xd, Xd, layout="TN", a_shift=mud, b_shift=mud, symmetric=True, split_k=split)
        _check(cov.cpu().numpy(), Xc.T, Xc.T, 130, what="large-mean covariance")
        gram = gemm_f64c(Xd, Xd, layout="NT", a_shift=mud, b_shift=mud, symmetric=True, split_k=split)
        _check(gram.cpu().numpy(), Xc, Xc, 65, what="large-mean Gram")
        onesided = gemm_f64c(Xd, torch.from_numpy(np.ascontiguousarray(Xc[:17])).to(dev), layout="NT", a_shift=mud, split_k=split)
        _check(onesided.cpu().numpy(), Xc, Xc[:17], 65, what="large-mean transform-like product")


# ---- PCA against the oracle ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(i):
    n, d, r, k = SHAPES[i]
    X = make_matrix(n, d, r, 1)
    return X, pca_full(X.astype(np.float64), k)


@functools.lru_cache(maxsize=None)
def _fitted(i):
    X, _ = _case(i)
    return PCA(SHAPES[i][3]).fit(torch.from_numpy(X).cuda())


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"n{n}_d{d}_k{k}" for n, d, _, k in SHAPES])
def test_pca_fit_against_oracle(dev, i):
    n, d, r, k = SHAPES[i]
    X, o = _case(i)
    p = _fitted(i)
    for name in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
        a = getattr(p, name)
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == getattr(o, name).shape, name
    assert (p.n_components_, p.n_samples_, p.n_features_in_) == (k, n, d)
    err = {"components": np.abs(p.components_ - o.components_).max(),
           "singular": (np.abs(p.singular_values_ - o.singular_values_) / o.singular_values_).max(),
           "variance": (np.abs(p.explained_variance_ - o.explained_variance_) / o.explained_variance_).max(),
           "ratio": np.abs(p.explained_variance_ratio_ - o.explained_variance_ratio_).max()}
    print(f"PCA n{n} d{d} k{k}: " + ", ".join(f"{key} {v:.3g}" for key, v in err.items()))
    assert err["components"] <= 1e-9
    assert err["singular"] <= 1e-10 and err["variance"] <= 1e-10
    assert err["ratio"] <= 1e-12
    X64 = X.astype(np.float64)
    assert (np.abs(p.mean_ - o.mean_) <= n * U53 * np.abs(X64).mean(axis=0)).all()
    # noise variance = mean of the discarded eigenvalues / (n - 1).  Each eigenvalue moves by at most the 2-norm of the matrix error: the
    # product's (2 K u per element against |Xc|^T |Xc|, whose norm is at most the trace; K = the reduction length max(n, d)) plus the
    # eigen-solver's backward error (a few min(n, d) u times the largest eigenvalue, again at most the trace)
    total_var = (X64 - o.mean_).var(axis=0, ddof=1).sum()
    assert abs(p.noise_variance_ - o.noise_variance_) <= (2 * max(n, d) + 4 * min(n, d)) * U53 * total_var
    Y = p.fit_transform(torch.from_numpy(X).to(dev))
    Yt = p.transform(torch.from_numpy(X).to(dev))
    assert Y.dtype == torch.float32 and Y.shape == (n, k)
    assert (Y.double() - Yt.double()).abs().max().item() <= 1e-9 * Yt.abs().max().item()
    Y64 = PCA(k).fit_transform(X64)                                     # numpy float64 in, numpy float64 out
    assert isinstance(Y64, np.ndarray) and Y64.dtype == np.float64
    assert np.abs(Y64 - transform(o, X64)).max() <= 1e-9 * np.abs(Y64).max()


@functools.lru_cache(maxsize=None)
def _fresh_rows(i, m):
    """m rows the fit has not seen, in the span the fit describes: random mixtures of the training rows plus the same noise level"""
    X, _ = _case(i)
    rs = np.random.RandomState(100 + m)
    n, d = X.shape
    return ((rs.randn(m, n) / np.sqrt(n)) @ X.astype(np.float64) + 1e-3 * rs.randn(m, d)).astype(np.float32)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"n{n}_d{d}_k{k}" for n, d, _, k in SHAPES])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pca_transform_fresh_rows(dev, i, dt):
    _, o = _case(i)
    p = _fitted(i)
    k = SHAPES[i][3]
    for m in (0, 1, 77, 1001):
        Xn = _fresh_rows(i, m).astype(np.float32 if dt == "f32" else np.float64)
        Y = p.transform(torch.from_numpy(Xn).to(dev))
        assert Y.dtype == TORCH_DT[dt] and Y.shape == (m, k) and Y.is_cuda
        Yn = p.transform(Xn)
        assert isinstance(Yn, np.ndarray) and Yn.dtype == Xn.dtype and Yn.shape == (m, k)
        if m == 0:
            continue
        assert np.array_equal(Yn, Y.cpu().numpy())
        want = transform(o, Xn)
        tol = 1e-10 * np.abs(want).max() + (2.0 ** -23 * np.abs(want) if dt == "f32" else 0.0)
        err = np.abs(Yn.astype(np.float64) - want)
        print(f"transform shape {i} m{m} {dt}: max err {err.max():.3g} at scale {np.abs(want).max():.3g}")
        assert (err <= tol).all()


# ---- contract -----------------------------------------------------------------------------------------------------------------
def test_pca_rejects_bad_n_components_and_nan(dev):
    X = torch.from_numpy(make_matrix(37, 203, 12, 1)).to(dev)
    for bad in (0, 38, 204):
        with pytest.raises(ValueError, match="n_components"):
            PCA(bad).fit(X)
    with pytest.raises(ValueError, match="n_components"):
        PCA(20).fit(X.T.contiguous()[:, :19])                       # covariance regime: min(n, d) = 19
    Xn = X.clone()
    Xn[3, 5] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        PCA(4).fit(Xn)
    Xn[3, 5] = float("inf")
    with pytest.raises(ValueError, match="NaN or infinity"):
        PCA(4).fit(Xn)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PCA(4).fit(X.cpu())
    with pytest.raises(ValueError, match="features"):
        PCA(4).fit(X).transform(X[:, :100])


def test_pca_gram_regime_rank_rule(dev):
    rs = np.random.RandomState(4)
    half = rs.randn(10, 50)
    dup = np.concatenate([half, half])                               # 20 rows, 10 distinct: the centred matrix has rank 9
    with pytest.raises(ValueError, match=r"numerical rank 9\b"):
        PCA(12).fit(dup)
    assert PCA(9).fit(dup).components_.shape == (9, 50)
    full = rs.randn(20, 50)
    assert PCA(12).fit(full).components_.shape == (12, 50)
    with pytest.raises(ValueError, match=r"numerical rank 19\b"):   # centred data has rank <= n - 1
        PCA(20).fit(full)


def test_pca_non_contiguous_input_same_bits(dev):
    X = torch.from_numpy(make_matrix(61, 2 * 203, 12, 1)).to(dev)
    view = X[:, ::2]
    assert not view.is_contiguous()
    a, b = PCA(8), PCA(8)
    Ya, Yb = a.fit_transform(view), b.fit_transform(view.contiguous())
    assert torch.equal(Ya, Yb) and np.array_equal(a.components_, b.components_) and np.array_equal(a.mean_, b.mean_)
    Xt = X.T                                                         # covariance regime through a transposed view
    assert torch.equal(PCA(8).fit_transform(Xt), PCA(8).fit_transform(Xt.contiguous()))


def test_pca_from_sklearn_randomized(dev):
    from sklearn.decomposition import PCA as SkPCA
    X = make_matrix(300, 167, 80, 1)
    X64 = X.astype(np.float64)
    sk = SkPCA(64, svd_solver="randomized", random_state=0).fit(X64)
    p = PCA.from_sklearn(sk)
    assert p.n_components_ == 64 and np.array_equal(p.components_, sk.components_)
    for Xin in (X64, X):
        want = sk.transform(Xin.astype(np.float64))
        got = p.transform(Xin)
        assert got.dtype == Xin.dtype
        tol = 1e-10 * np.abs(want).max() + (2.0 ** -23 * np.abs(want) if Xin.dtype == np.float32 else 0.0)
        assert (np.abs(got.astype(np.float64) - want) <= tol).all()


def test_pca_output_feeds_the_mlp_grid(dev):
    """Models/model_opt_maccs.py:104-109: PCA(100) features are what mlp.grid_search_cv trains on ([n, 100] float64)."""
    X = make_matrix(300, 167, 120, 6).astype(np.float64)
    Y = PCA(100).fit_transform(X)
    assert isinstance(Y, np.ndarray) and Y.dtype == np.float64 and Y.shape == (300, 100) and Y.flags.c_contiguous and np.isfinite(Y).all()
    t = mlp.GridMLPTrainer(Y, (np.arange(300) % 2).astype(np.float64))
    assert (t.n, t.n_features) == (300, 100) and t.X.dtype == torch.float64


def test_pca_features_through_shipped_weights(dev):
    """...transformer_cnn_opt.py:30-33 end to end: fingerprints [200, 167] -> 64 and images [200, 49152] -> 128 on the GPU, through the
    reference's best_nn_model_maccs.pth, against the same model fed the oracle's features."""
    from bbbp_amd.variants import PCAFusionModel
    m = PCAFusionModel(64, 128)
    m.load_state_dict(torch.load(os.path.join(GOLDEN, "best_nn_model_maccs.pth"), map_location="cpu", weights_only=True), strict=True)
    m = m.to(dev).eval()
    fp, img = make_matrix(200, 167, 100, 2), make_matrix(200, 49152, 160, 3)
    got = [PCA(k).fit_transform(torch.from_numpy(x).to(dev)) for x, k in ((fp, 64), (img, 128))]
    want = [torch.from_numpy(transform(pca_full(x.astype(np.float64), k), x).astype(np.float32)).to(dev) for x, k in ((fp, 64), (img, 128))]
    assert got[0].shape == (200, 64) and got[1].shape == (200, 128) and got[0].dtype == got[1].dtype == torch.float32
    with torch.no_grad():
        out, ref = m(*got), m(*want)
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, what="PCA features through best_nn_model_maccs.pth")
