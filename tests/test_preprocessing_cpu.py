"""CPU: the numpy restatement of ``bbbp_amd.preprocessing`` (tests/preprocessing_numpy.py) equals scikit-learn 1.7 bit for bit -- ``mean_``,
``var_``, ``scale_``, ``transform``, ``inverse_transform``, a ``partial_fit`` series, the flags, the polynomial columns and ``powers_`` --
so that the GPU tests, which compare the kernels with the restatement, stand on scikit-learn's own results.  Skipped without the package.

Also here, because they need no GPU: the refusals by name, and the argument errors of the three entry points (reported before any HIP
call).

``d == 1`` is the known deviation: numpy sums a single column pairwise, the restatement (and the kernel) in row order.  There the two are
held together only by the bound of floating-point summation: a sum of n terms computed in any order differs from the exact sum by at most
(n - 1) eps' sum|term| to first order, eps' = 2^-53, so two orders differ by at most 2 (n - 1) eps' sum|term| < 2 n eps sum|term| with
eps = 2^-52 -- derived, not measured.  The measured distance in ulp is printed."""
import ctypes
import math

import numpy as np
import pytest
import torch

import preprocessing_numpy as R
from bbbp_amd import _lib, preprocessing

SCALER_SHAPES = [(1, 3), (2, 2), (9, 2), (129, 5), (257, 65), (1058, 167), (2000, 100)]
EPS = 2.0 ** -52


def _sk():
    return pytest.importorskip("sklearn.preprocessing")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype == np.float64 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# ---- the scaler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", SCALER_SHAPES)
def test_moments_transform_and_inverse_equal_sklearn(n, d):
    sk = _sk()
    X = R.scaler_matrix(n, d, seed=n + d)
    ref = sk.StandardScaler().fit(X)
    mean, var, scale, N = R.moments(X)
    assert _same(mean, ref.mean_) and _same(var, ref.var_) and _same(scale, ref.scale_) and N == ref.n_samples_seen_
    assert _same(R.transform(X, mean, scale), ref.transform(X))
    Z = np.random.RandomState(1).standard_normal((7, d))                 # rows the fit has not seen
    assert _same(R.transform(Z, mean, scale), ref.transform(Z))
    assert _same(R.inverse_transform(Z, mean, scale), ref.inverse_transform(Z))


def test_the_column_kinds_are_what_they_claim():
    sk = _sk()
    X = R.scaler_matrix(129, 5, seed=134)
    assert np.ptp(X[:, 0]) == 0 and set(np.unique(X[:, 1])) == {1e8, 1e8 + np.spacing(1e8)} and set(np.unique(X[:, 3])) == {0.0, 1.0}
    mean, var, scale, _ = R.moments(X)
    assert scale[0] == 1.0 and var[0] == 0.0
    assert scale[1] == 1.0 and var[1] > 0.0                              # constant by the bound, not by its variance
    assert 1e-161 < scale[2] < 1e-159 and scale[2] < 10 * EPS            # the 10 eps rule would call it constant; scikit-learn does not
    assert _same(scale, sk.StandardScaler().fit(X).scale_)


def test_uint8_and_bool_matrices_convert_exactly():
    sk = _sk()
    rng = np.random.RandomState(3)
    for X in (rng.randint(0, 256, size=(129, 5)).astype(np.uint8), rng.randint(0, 2, size=(65, 3)).astype(bool),
              rng.randint(-1000, 1000, size=(40, 4)).astype(np.int64)):
        ref = sk.StandardScaler().fit(X)
        mean, var, scale, _ = R.moments(X)
        assert _same(mean, ref.mean_) and _same(var, ref.var_) and _same(scale, ref.scale_)
        assert _same(R.transform(X, mean, scale), ref.transform(X))


def test_partial_fit_series_100_100_30():
    sk = _sk()
    X = R.scaler_matrix(230, 5, seed=7)
    ref = sk.StandardScaler()
    for (mean, var, scale, N), B in zip(R.fit_series([X[:100], X[100:200], X[200:]]), (X[:100], X[100:200], X[200:])):
        ref.partial_fit(B)
        assert _same(mean, ref.mean_) and _same(var, ref.var_) and _same(scale, ref.scale_) and N == ref.n_samples_seen_
    np.testing.assert_allclose(R.moments(X)[1][3:], var[3:], rtol=1e-12)          # and the series ends near the one-batch variance


@pytest.mark.parametrize("with_mean,with_std", [(True, False), (False, True), (False, False)])
def test_flag_combinations(with_mean, with_std):
    sk = _sk()
    X = R.scaler_matrix(129, 5, seed=11)
    ref = sk.StandardScaler(with_mean=with_mean, with_std=with_std).fit(X)
    mean, var, scale, _ = R.moments(X)
    if with_mean or with_std:
        assert _same(mean, ref.mean_)                                    # scikit-learn keeps the mean whenever it computes anything
    else:
        assert ref.mean_ is None
    if with_std:
        assert _same(var, ref.var_) and _same(scale, ref.scale_)
    else:
        assert ref.var_ is None and ref.scale_ is None
    args = (mean if with_mean else None, scale if with_std else None)
    assert _same(R.transform(X, *args), ref.transform(X)) and _same(R.inverse_transform(X, *args), ref.inverse_transform(X))
    # a second batch with the variance switched off: the mean alone continues
    ref.partial_fit(X[:30])
    if with_mean or with_std:
        m2 = R.moments(X[:30], mean, var if with_std else None, 129)[0]
        assert _same(m2, ref.mean_)


@pytest.mark.parametrize("n", [65, 1058, 7807])
def test_single_column_is_within_the_summation_bound(n):
    sk = _sk()
    X = np.random.RandomState(n).standard_normal((n, 1)) * 3.0 + 40.0
    ref = sk.StandardScaler().fit(X)
    mean, var, scale, _ = R.moments(X)
    x = X[:, 0]
    # mean = S / n: the two sums differ by at most 2 n eps sum|x|; the division adds half an ulp to each
    bound_mean = (2 * n * EPS * np.abs(x).sum()) / n + EPS * abs(ref.mean_[0])
    assert abs(mean[0] - ref.mean_[0]) <= bound_mean
    # var = (sum t^2 - (sum t)^2 / n) / n with t = x - T: both Ts lie within bound_mean of each other, which moves every t by that much
    t = x - ref.mean_[0]
    dt = bound_mean + EPS * np.abs(t).max()
    sum_sq = (t * t).sum()
    bound_sq = 2 * n * EPS * sum_sq + 2 * dt * np.abs(t).sum() + n * dt * dt
    bound_corr = (2 * n * EPS * np.abs(t).sum() + n * dt) ** 2 / n
    bound_var = (bound_sq + bound_corr) / n + 4 * EPS * ref.var_[0]
    assert abs(var[0] - ref.var_[0]) <= bound_var
    assert abs(scale[0] - ref.scale_[0]) <= bound_var / (2 * ref.scale_[0]) * 1.01 + EPS * ref.scale_[0]
    print(f"d == 1, n = {n}: mean {R.ulp_distance(mean, ref.mean_)} ulp, var {R.ulp_distance(var, ref.var_)} ulp, "
          f"scale {R.ulp_distance(scale, ref.scale_)} ulp from scikit-learn")


# ---- the expansion ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 5, 65])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("interaction_only", [False, True])
@pytest.mark.parametrize("include_bias", [False, True])
def test_polynomial_columns_and_powers_equal_sklearn(d, degree, interaction_only, include_bias):
    sk = _sk()
    n = 3 if d == 65 and degree == 3 else 17
    X = np.random.RandomState(d * 10 + degree).standard_normal((n, d)) * 3.0
    ref = sk.PolynomialFeatures(degree, interaction_only=interaction_only, include_bias=include_bias).fit(X)
    want = ref.transform(X)
    got = R.polynomial(X, degree, interaction_only, include_bias)
    assert got.shape == (n, ref.n_output_features_) and _same(got, want)
    assert np.array_equal(R.powers(d, degree, interaction_only, include_bias), ref.powers_)
    assert preprocessing._n_output_features(d, degree, interaction_only, include_bias) == ref.n_output_features_
    table = [tuple(c) for c in preprocessing._combinations(d, degree, interaction_only, include_bias)]
    assert table == R.combinations(d, degree, interaction_only, include_bias)


def test_interaction_only_degree_3_on_two_features_adds_no_degree_3_column():
    sk = _sk()
    X = np.random.RandomState(0).standard_normal((9, 2))
    ref = sk.PolynomialFeatures(3, interaction_only=True, include_bias=False).fit(X)
    assert ref.n_output_features_ == 3 == len(R.combinations(2, 3, True, False)) == preprocessing._n_output_features(2, 3, True, False)
    assert _same(R.polynomial(X, 3, True, False), ref.transform(X))


class _Sparse:
    """What marks a scipy.sparse matrix for the input check."""
    shape = (4, 3)

    def tocsr(self):
        return self


# ---- refusals by name (none of them reaches the device) -----------------------------------------------------------------------------------
def test_refusals_by_name():
    P = preprocessing
    X = np.zeros((4, 3))
    for make in (lambda: P.StandardScaler(), lambda: P.PolynomialFeatures()):
        est = make()
        for name in ("float32", "float16"):
            with pytest.raises(TypeError, match=name + r".*\.double\(\)"):
                est.fit(X.astype(name))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            est.fit(torch.zeros(4, 3, dtype=torch.float64))
        with pytest.raises(ValueError, match="2-D"):
            est.fit(np.zeros(4))
        with pytest.raises(TypeError, match="sparse"):
            est.fit(_Sparse())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.StandardScaler(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.PolynomialFeatures(device="cpu")
    s = P.StandardScaler()
    for call in (s.fit, s.partial_fit, s.fit_transform):
        with pytest.raises(ValueError, match="sample_weight"):
            call(X, sample_weight=np.ones(4))
    for call in (s.transform, s.inverse_transform):
        with pytest.raises(ValueError, match="copy=False"):
            call(X, copy=False)
    with pytest.raises(ValueError, match="with_mean"):
        P.StandardScaler(with_mean=1)
    with pytest.raises(ValueError, match=r"\(min_degree, max_degree\)"):
        P.PolynomialFeatures((1, 2))
    for degree in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="degree"):
            P.PolynomialFeatures(degree)
    with pytest.raises(ValueError, match="order"):
        P.PolynomialFeatures(order="F")
    with pytest.raises(ValueError, match=f"{math.comb(3003, 3)} output columns"):
        P.PolynomialFeatures(3).fit(np.zeros((1, 3000)))
    with pytest.raises(ValueError, match="unknown parameters"):
        s.set_params(copy=False)
    assert s.get_params() == {"with_mean": True, "with_std": True, "device": torch.device("cuda")}
    assert s.set_params(with_std=False).with_std is False
    with pytest.raises(ValueError, match="scale of 0"):
        P.StandardScaler.from_arrays(np.zeros(3), np.zeros(3), device="cuda")


# ---- argument errors of the entry points, before any HIP call -----------------------------------------------------------------------------
def test_entry_points_validate_their_arguments_before_touching_the_gpu():
    L = _lib.lib()
    ERR_ARG = 1
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)               # never dereferenced: validation comes first
    mom = L.bbbp_scaler_moments
    assert mom(None, fake, 3, 0, 3, None, None, 0, fake, fake, fake, fake) == ERR_ARG and b"positive" in L.bbbp_last_error()
    assert mom(None, fake, 3, 4, 0, None, None, 0, fake, fake, fake, fake) == ERR_ARG
    assert mom(None, fake, 2, 4, 3, None, None, 0, fake, fake, fake, fake) == ERR_ARG and b"leading dimension" in L.bbbp_last_error()
    assert mom(None, fake, 3, 4, 3, None, None, -1, fake, fake, fake, fake) == ERR_ARG and b"last_n" in L.bbbp_last_error()
    assert mom(None, fake, 3, 4, 3, None, None, 5, fake, fake, fake, fake) == ERR_ARG and b"last_mean" in L.bbbp_last_error()
    assert mom(None, fake, 3, 4, 3, None, None, 0, fake, fake, fake, None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert mom(None, None, 3, 4, 3, None, None, 0, fake, fake, fake, fake) == ERR_ARG
    assert mom(None, odd, 3, 4, 3, None, None, 0, fake, fake, fake, fake) == ERR_ARG and b"aligned" in L.bbbp_last_error()
    app = L.bbbp_scaler_apply
    assert app(None, fake, 3, -1, 3, fake, fake, 0, fake, 3, None) == ERR_ARG and b"negative" in L.bbbp_last_error()
    assert app(None, fake, 2, 4, 3, fake, fake, 0, fake, 3, None) == ERR_ARG and b"leading dimensions" in L.bbbp_last_error()
    assert app(None, fake, 3, 4, 3, fake, fake, 0, fake, 2, None) == ERR_ARG
    assert app(None, fake, 3, 4, 3, fake, fake, 2, fake, 3, None) == ERR_ARG and b"inverse" in L.bbbp_last_error()
    assert app(None, fake, 3, 4, 3, fake, fake, 0, None, 3, None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert app(None, fake, 3, 4, 3, fake, fake, 0, odd, 3, None) == ERR_ARG and b"aligned" in L.bbbp_last_error()
    assert app(None, fake, 3, 0, 3, fake, fake, 0, fake, 3, None) == 0                                          # empty: nothing to do
    exp = L.bbbp_poly_expand
    assert exp(None, fake, 3, -1, 3, fake, 6, fake, 6, None) == ERR_ARG and b"positive" in L.bbbp_last_error()
    assert exp(None, fake, 3, 4, 0, fake, 6, fake, 6, None) == ERR_ARG
    assert exp(None, fake, 3, 4, 3, fake, 0, fake, 6, None) == ERR_ARG
    assert exp(None, fake, 2, 4, 3, fake, 6, fake, 6, None) == ERR_ARG and b"leading dimensions" in L.bbbp_last_error()
    assert exp(None, fake, 3, 4, 3, fake, 6, fake, 5, None) == ERR_ARG
    assert exp(None, fake, 3, 4, 3, None, 6, fake, 6, None) == ERR_ARG and b"null" in L.bbbp_last_error()
    assert exp(None, odd, 3, 4, 3, fake, 6, fake, 6, None) == ERR_ARG and b"aligned" in L.bbbp_last_error()
    assert exp(None, fake, 3, 0, 3, fake, 6, fake, 6, None) == 0                                                # empty: nothing to do
