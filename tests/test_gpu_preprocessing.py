"""GPU: ``preprocessing.StandardScaler`` and ``PolynomialFeatures`` equal the numpy restatement (tests/preprocessing_numpy.py) bit for bit --
every float64 array compared as integers -- for a tensor in and an array in, at the smallest shapes at which the kernels can go wrong.
``tests/test_preprocessing_cpu.py`` pins the restatement to scikit-learn 1.7 in turn.

Scaler shapes: one element; fewer rows than the load batch; a single column (65 rows: four batches and a remainder); one column past a wave;
257 x 257: past a work-group of 64 columns four times over, more rows than the load batch, odd leading dimension (the 8-byte accesses);
1058 x 167: the reference's fingerprint table.  Every matrix holds the column kinds of ``scaler_matrix`` as far as its width allows."""
import functools

import numpy as np
import pytest
import torch

import preprocessing_numpy as R
from bbbp_amd import decomposition, preprocessing

pytestmark = pytest.mark.gpu

SCALER_SHAPES = [(1, 1), (2, 3), (65, 1), (9, 65), (257, 257), (1058, 167)]
POLY_CASES = [(1, 1, 2, False), (3, 2, 3, True), (65, 5, 3, False), (7, 65, 2, True), (257, 60, 2, True)]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want):
    if isinstance(got, torch.Tensor):
        assert got.is_cuda and got.dtype == torch.float64
    else:
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
    return tuple(got.shape) == tuple(np.shape(want)) and np.array_equal(_bits(got), _bits(want))


@functools.lru_cache(maxsize=None)
def _scaler_reference(n, d):
    """Matrix, unseen rows and restated results, computed once per shape and left unchanged."""
    X = R.scaler_matrix(n, d, seed=n + d)
    Z = np.random.RandomState(n).standard_normal((11, d)) * 5.0
    mean, var, scale, N = R.moments(X)
    ref = dict(X=X, Z=Z, mean=mean, var=var, scale=scale, N=N, XT=R.transform(X, mean, scale), ZT=R.transform(Z, mean, scale),
               ZI=R.inverse_transform(Z, mean, scale))
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def _fitted_equals(s, r):
    return (_same(s.mean_, r["mean"]) and _same(s.var_, r["var"]) and _same(s.scale_, r["scale"]) and s.n_samples_seen_ == r["N"]
            and isinstance(s.n_samples_seen_, int) and s.n_features_in_ == r["X"].shape[1])


@pytest.mark.parametrize("n,d", SCALER_SHAPES)
@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_scaler_equals_the_restatement(dev, n, d, kind):
    r = _scaler_reference(n, d)
    give = (lambda a: np.array(a)) if kind == "array" else (lambda a: torch.from_numpy(np.array(a)).to(dev))
    s = preprocessing.StandardScaler(device=dev)
    assert s.fit(give(r["X"])) is s and _fitted_equals(s, r)
    assert _same(s.transform(give(r["X"])), r["XT"])
    assert _same(s.transform(give(r["Z"])), r["ZT"])                     # rows the fit has not seen
    assert _same(s.inverse_transform(give(r["Z"])), r["ZI"])
    s2 = preprocessing.StandardScaler(device=dev)
    assert _same(s2.fit_transform(give(r["X"])), r["XT"]) and _fitted_equals(s2, r)
    if d >= 5:
        assert s.scale_[0] == 1.0 and s.scale_[1] == 1.0 and s.var_[1] > 0 and (n < 9 or s.scale_[2] < 1e-159) and s.scale_[2] != 1.0


def test_scaler_integer_and_bool_inputs_convert_exactly(dev):
    rng = np.random.RandomState(3)
    for X in (rng.randint(0, 256, size=(129, 5)).astype(np.uint8), rng.randint(0, 2, size=(65, 3)).astype(bool),
              rng.randint(-1000, 1000, size=(40, 4)).astype(np.int64)):
        mean, var, scale, _ = R.moments(X)
        for give in (X, torch.from_numpy(X).to(dev)):
            s = preprocessing.StandardScaler(device=dev)
            assert _same(s.fit_transform(give), R.transform(X, mean, scale))
            assert _same(s.mean_, mean) and _same(s.var_, var) and _same(s.scale_, scale)


@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_partial_fit_series_equals_one_restated_series(dev, kind):
    X = R.scaler_matrix(230, 67, seed=7)
    batches = [X[:100], X[100:200], X[200:]]
    s = preprocessing.StandardScaler(device=dev)
    for (mean, var, scale, N), B in zip(R.fit_series(batches), batches):
        s.partial_fit(B.copy() if kind == "array" else torch.from_numpy(B.copy()).to(dev))
        assert _same(s.mean_, mean) and _same(s.var_, var) and _same(s.scale_, scale) and s.n_samples_seen_ == N
    assert _same(s.transform(X), R.transform(X, mean, scale))
    with pytest.raises(ValueError, match="features"):
        s.partial_fit(X[:, :5].copy())
    s.fit(batches[2].copy())                                             # fit starts anew
    assert _same(s.mean_, R.moments(batches[2])[0]) and s.n_samples_seen_ == 30


@pytest.mark.parametrize("with_mean,with_std", [(True, False), (False, True), (False, False)])
def test_flag_combinations(dev, with_mean, with_std):
    X = R.scaler_matrix(129, 67, seed=11)
    mean, var, scale, _ = R.moments(X)
    Xt = torch.from_numpy(X).to(dev)
    s = preprocessing.StandardScaler(with_mean=with_mean, with_std=with_std, device=dev).fit(Xt)
    if with_mean or with_std:
        assert _same(s.mean_, mean)
    else:
        assert s.mean_ is None
    if with_std:
        assert _same(s.var_, var) and _same(s.scale_, scale)
    else:
        assert s.var_ is None and s.scale_ is None
    args = (mean if with_mean else None, scale if with_std else None)
    assert _same(s.transform(Xt), R.transform(X, *args)) and _same(s.inverse_transform(Xt), R.inverse_transform(X, *args))
    s.partial_fit(Xt[:30])
    assert s.n_samples_seen_ == 159
    if with_mean or with_std:
        m2, v2, sc2, _ = R.moments(X[:30], mean, var if with_std else None, 129)
        assert _same(s.mean_, m2) and (not with_std or (_same(s.var_, v2) and _same(s.scale_, sc2)))


@pytest.mark.parametrize("n,d", [(9, 65), (257, 100)])
def test_padded_view_at_an_odd_base_is_read_in_place(dev, n, d):
    """ld = d + 7 at a base 8 bytes past a 16-byte boundary: the scalar path of the apply kernel, the strided reads of both."""
    r = _scaler_reference(n, d) if (n, d) in SCALER_SHAPES else None
    X = r["X"] if r else R.scaler_matrix(n, d, seed=n + d)
    mean, var, scale, _ = R.moments(X)
    pool = torch.full((n * (d + 7) + 1,), float("nan"), dtype=torch.float64, device=dev)
    view = pool[1:].view(n, d + 7)[:, :d]
    view.copy_(torch.from_numpy(np.array(X)))
    assert view.stride() == (d + 7, 1) and view.data_ptr() % 16 == 8
    assert preprocessing._moved(view, dev).data_ptr() == view.data_ptr()
    s = preprocessing.StandardScaler(device=dev).fit(view)
    assert _same(s.mean_, mean) and _same(s.var_, var) and _same(s.scale_, scale)
    assert _same(s.transform(view), R.transform(X, mean, scale)) and _same(s.inverse_transform(view), R.inverse_transform(X, mean, scale))
    p = preprocessing.PolynomialFeatures(2, device=dev)
    assert _same(p.fit_transform(view[:, :9]), R.polynomial(X[:, :9], 2, False, True))
    # a column-major tensor is copied: same values, summed in row order
    col_major = torch.from_numpy(np.array(X)).to(dev).t().contiguous().t()
    assert col_major.stride(1) != 1 or d == 1
    assert _same(preprocessing.StandardScaler(device=dev).fit(col_major).var_, var)


def test_non_finite_input_raises(dev):
    X = R.scaler_matrix(70, 67, seed=2)
    s = preprocessing.StandardScaler(device=dev).fit(X)
    p = preprocessing.PolynomialFeatures(2, interaction_only=True, include_bias=False, device=dev).fit(X)
    for value, at in ((np.nan, (69, 66)), (np.inf, (0, 0)), (-np.inf, (33, 64))):
        bad = X.copy()
        bad[at] = value
        for call in (preprocessing.StandardScaler(device=dev).fit, preprocessing.StandardScaler(device=dev).fit_transform, s.partial_fit, s.transform,
                     s.inverse_transform, p.transform, p.fit_transform):
            with pytest.raises(ValueError, match="NaN or infinity"):
                call(torch.from_numpy(bad).to(dev))
    big = np.full((2, 3), 1e200)                                         # finite inputs whose products overflow are no input error
    assert np.isinf(p.fit_transform(big)).any()


def test_from_sklearn_and_from_arrays(dev):
    sk = pytest.importorskip("sklearn.preprocessing")
    X = R.scaler_matrix(129, 67, seed=5)
    Z = np.random.RandomState(0).standard_normal((9, 67))
    for with_mean, with_std in ((True, True), (True, False), (False, True), (False, False)):
        ref = sk.StandardScaler(with_mean=with_mean, with_std=with_std).fit(X)
        s = preprocessing.StandardScaler.from_sklearn(ref, device=dev)
        assert _same(s.transform(Z), ref.transform(Z)) and _same(s.inverse_transform(Z), ref.inverse_transform(Z))
        assert s.n_samples_seen_ == 129 and s.n_features_in_ == 67
        ref.partial_fit(Z)
        s.partial_fit(Z)                                                 # the adopted state continues the series
        for name in ("mean_", "var_", "scale_"):
            a, b = getattr(s, name), getattr(ref, name)
            assert (a is None and b is None) or _same(a, b), name
    mean, var, scale, _ = R.moments(X)
    s = preprocessing.StandardScaler.from_arrays(mean, scale, device=dev)
    assert _same(s.transform(torch.from_numpy(Z).to(dev)), R.transform(Z, mean, scale))
    with pytest.raises(RuntimeError, match="partial_fit cannot continue"):
        s.partial_fit(Z)


# ---- the expansion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,degree,interaction_only", POLY_CASES)
@pytest.mark.parametrize("include_bias", [False, True])
@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_polynomial_equals_the_restatement(dev, n, d, degree, interaction_only, include_bias, kind):
    X = np.random.RandomState(n + d).standard_normal((n, d)) * 3.0
    want = R.polynomial(X, degree, interaction_only, include_bias)
    p = preprocessing.PolynomialFeatures(degree, interaction_only=interaction_only, include_bias=include_bias, device=dev)
    got = p.fit_transform(X if kind == "array" else torch.from_numpy(X).to(dev))
    assert _same(got, want)
    assert p.n_features_in_ == d and p.n_output_features_ == want.shape[1]
    assert p.powers_.dtype == np.int64 and np.array_equal(p.powers_, R.powers(d, degree, interaction_only, include_bias))
    assert _same(p.fit(X).transform(X[: max(n // 2, 1)].copy()), want[: max(n // 2, 1)])


def test_polynomial_reads_from_global_memory_when_the_rows_do_not_fit_the_lds(dev):
    """d = 513: one column past the staged path's 512."""
    X = np.random.RandomState(9).standard_normal((9, 513))
    p = preprocessing.PolynomialFeatures(2, interaction_only=True, include_bias=True, device=dev)
    assert _same(p.fit_transform(torch.from_numpy(X).to(dev)), R.polynomial(X, 2, True, True))
    with pytest.raises(ValueError, match="features"):
        p.transform(X[:, :5].copy())


def test_pipeline_stays_on_the_device(dev):
    """StandardScaler -> PCA(30) -> PolynomialFeatures(2, interaction_only, no bias) on a CUDA tensor equals the same three steps with a
    numpy round trip between them, bit for bit."""
    X = R.scaler_matrix(300, 100, seed=12)
    Xt = torch.from_numpy(X).to(dev)

    def steps():
        return (preprocessing.StandardScaler(device=dev), decomposition.PCA(30, device=dev),
                preprocessing.PolynomialFeatures(2, interaction_only=True, include_bias=False, device=dev))

    out = Xt
    for est in steps():
        out = est.fit_transform(out)
        assert isinstance(out, torch.Tensor) and out.is_cuda
    assert out.shape == (300, 465) and out.dtype == torch.float64
    host = X
    for est in steps():
        host = est.fit_transform(host)
        assert isinstance(host, np.ndarray)
    assert _same(out, host)
