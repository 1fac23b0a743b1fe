"""GPU: ``preprocessing.StandardScaler`` and ``PolynomialFeatures`` with every ``torch.empty`` served from poisoned, guarded pools
(tests/poison.py), and with inputs and outputs inside moats at odd bases with padded leading dimensions.

The moment vectors with their flag word, the transformed matrix, the expanded matrix and the flag words of the two other kernels are
``torch.empty``: the kernels have to write every element of their outputs and nothing else, the flag has to be set by the call itself, and
nothing may be read that was not given.  So under the three fills the results must equal those of an unpoisoned run bit for bit, and no
guard band or moat may be touched.  65 columns put one behind a wave, 257 rows one behind sixteen load batches; 60 -> 1830 columns is the
reference's expansion, 5 -> 55 its smallest degree-3 relative."""
import numpy as np
import pytest
import torch

import preprocessing_numpy as R
from bbbp_amd import _dense, _lib, preprocessing
from poison import FILLS, moated, poisoned_allocations

pytestmark = pytest.mark.gpu

SCALER_SHAPES = [(65, 65), (257, 100)]
POLY_SHAPES = [(65, 5, 3), (257, 60, 2)]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run_scaler(dev, X, Z):
    """Every path once: a fit, a continued fit, the transform of seen and unseen rows, the inverse."""
    s = preprocessing.StandardScaler(device=dev)
    out = [s.fit_transform(X), s.mean_, s.var_, s.scale_, s.transform(Z), s.inverse_transform(Z)]
    s.partial_fit(Z)
    out += [s.mean_, s.var_, s.scale_, s.transform(X)]
    return [_bits(a) for a in out]


def _run_poly(dev, X, degree):
    p = preprocessing.PolynomialFeatures(degree, device=dev)
    q = preprocessing.PolynomialFeatures(degree, interaction_only=True, include_bias=False, device=dev)
    return [_bits(p.fit_transform(X)), _bits(q.fit_transform(X))]


def _scaler_problem(n, d):
    X = R.scaler_matrix(n, d, seed=n + d)
    Z = np.random.RandomState(d).standard_normal((37, d)) * 4.0
    return X, Z


def _scaler_restated(X, Z):
    mean, var, scale, N = R.moments(X)
    m2, v2, s2, _ = R.moments(Z, mean, var, N)
    return [_bits(a) for a in (R.transform(X, mean, scale), mean, var, scale, R.transform(Z, mean, scale), R.inverse_transform(Z, mean, scale),
                               m2, v2, s2, R.transform(X, m2, s2))]


def _compare(want, got, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: result {i} differs"


@pytest.mark.parametrize("n,d", SCALER_SHAPES)
@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_scaler_results_do_not_depend_on_the_fill(dev, monkeypatch, n, d, kind):
    X, Z = _scaler_problem(n, d)
    give = (lambda a: a.copy()) if kind == "array" else (lambda a: torch.from_numpy(a.copy()).to(dev))
    want = _run_scaler(dev, give(X), give(Z))
    _compare(_scaler_restated(X, Z), want, "unpoisoned run against the restatement")
    for fill in FILLS:
        Xg, Zg = give(X), give(Z)
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run_scaler(dev, Xg, Zg)
            torch.cuda.synchronize()
        assert pa.check() >= 9, "the moment vectors, the outputs and the flag words did not go through the pools"
        pa.release()
        _compare(want, got, f"fill {fill:#04x}")


@pytest.mark.parametrize("n,d,degree", POLY_SHAPES)
@pytest.mark.parametrize("kind", ["array", "tensor"])
def test_polynomial_results_do_not_depend_on_the_fill(dev, monkeypatch, n, d, degree, kind):
    X = np.random.RandomState(n).standard_normal((n, d)) * 3.0
    give = (lambda a: a.copy()) if kind == "array" else (lambda a: torch.from_numpy(a.copy()).to(dev))
    want = _run_poly(dev, give(X), degree)
    _compare([_bits(R.polynomial(X, degree, False, True)), _bits(R.polynomial(X, degree, True, False))], want, "unpoisoned run against the restatement")
    for fill in FILLS:
        Xg = give(X)
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run_poly(dev, Xg, degree)
            torch.cuda.synchronize()
        assert pa.check() >= 4, "the expanded matrices and their flag words did not go through the pools"
        pa.release()
        _compare(want, got, f"fill {fill:#04x}")


@pytest.mark.parametrize("n,d", SCALER_SHAPES)
def test_moated_scaler_input_with_an_odd_base_and_a_padded_leading_dimension(dev, monkeypatch, n, d):
    X, Z = _scaler_problem(n, d)
    want = _run_scaler(dev, X.copy(), Z.copy())
    for fill in FILLS:
        view, check = moated(torch.from_numpy(X.copy()), fill, ld=d + 7, offset=3, device=dev)
        zview, zcheck = moated(torch.from_numpy(Z.copy()), fill, ld=d + 5, offset=1, device=dev)
        assert view.stride(0) == d + 7 and view.data_ptr() % 16 != 0 and zview.data_ptr() % 16 != 0
        assert preprocessing._moved(view, dev).data_ptr() == view.data_ptr(), "the view would be copied, not read in place"
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run_scaler(dev, view, zview)
            torch.cuda.synchronize()
        pa.check()
        pa.release()
        check()
        zcheck()
        _compare(want, got, f"fill {fill:#04x}")


@pytest.mark.parametrize("n,d", SCALER_SHAPES)
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("ld_in,off_in,ld_out,off_out", [(7, 3, 5, 1), (8, 2, 6, 4)])
def test_the_apply_kernel_reads_and_writes_moated_operands_in_place(dev, n, d, inverse, ld_in, off_in, ld_out, off_out):
    """``bbbp_scaler_apply`` itself, input and output both in moats: (7, 3, 5, 1) puts both at odd bases with odd leading dimensions (the
    8-byte accesses), (8, 2, 6, 4) at 16-byte aligned bases with even leading dimensions (the 16-byte accesses, with an odd d at 65)."""
    X, _ = _scaler_problem(n, d)
    mean, var, scale, _ = R.moments(X)
    want = _bits((R.inverse_transform if inverse else R.transform)(X, mean, scale))
    mean_d, scale_d = torch.from_numpy(mean).to(dev), torch.from_numpy(scale).to(dev)
    for fill in FILLS:
        src, check_src = moated(torch.from_numpy(X.copy()), fill, ld=d + ld_in, offset=off_in, device=dev)
        out, check_out = moated((n, d), fill, ld=d + ld_out, offset=off_out, device=dev, dtype=torch.float64)
        assert (src.data_ptr() % 16 == 0) == (off_in % 2 == 0) and (out.data_ptr() % 16 == 0) == (off_out % 2 == 0)
        flag = torch.full((1,), fill * 0x01010101 & 0x7FFFFFFF, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bbbp_scaler_apply(_dense.stream(), src.data_ptr(), d + ld_in, n, d, mean_d.data_ptr(), scale_d.data_ptr(), inverse,
                                                    out.data_ptr(), d + ld_out, flag.data_ptr()), "bbbp_scaler_apply")
        torch.cuda.synchronize()
        check_src()
        check_out()
        assert int(flag.cpu()[0]) == 0
        assert np.array_equal(_bits(out), want), f"fill {fill:#04x}"


@pytest.mark.parametrize("n,d,degree", POLY_SHAPES)
def test_the_expansion_kernel_reads_and_writes_moated_operands_in_place(dev, n, d, degree):
    X = np.random.RandomState(n).standard_normal((n, d)) * 3.0
    want = _bits(R.polynomial(X, degree, False, True))
    p = preprocessing.PolynomialFeatures(degree, device=dev).fit(X)
    P = p.n_output_features_
    for fill in FILLS:
        src, check_src = moated(torch.from_numpy(X.copy()), fill, ld=d + 7, offset=3, device=dev)
        out, check_out = moated((n, P), fill, ld=P + 5, offset=1, device=dev, dtype=torch.float64)
        assert src.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
        flag = torch.full((1,), fill * 0x01010101 & 0x7FFFFFFF, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bbbp_poly_expand(_dense.stream(), src.data_ptr(), d + 7, n, d, p._table_d.data_ptr(), P, out.data_ptr(), P + 5,
                                                   flag.data_ptr()), "bbbp_poly_expand")
        torch.cuda.synchronize()
        check_src()
        check_out()
        assert int(flag.cpu()[0]) == 0
        assert np.array_equal(_bits(out), want), f"fill {fill:#04x}"


@pytest.mark.parametrize("n,d", SCALER_SHAPES)
def test_the_moments_kernel_reads_a_moated_input_in_place(dev, n, d):
    X, Z = _scaler_problem(n, d)
    mean, var, scale, N = R.moments(X)
    m2, v2, s2, _ = R.moments(Z, mean, var, N)
    L = _lib.lib()
    for fill in FILLS:
        src, check_src = moated(torch.from_numpy(Z.copy()), fill, ld=d + 7, offset=3, device=dev)
        res, check_res = moated((1, 3 * d + 1), fill, offset=1, device=dev, dtype=torch.float64)
        res = res[0]
        last = torch.from_numpy(np.concatenate([mean, var])).to(dev)
        with torch.cuda.device(dev):
            _lib.check(L.bbbp_scaler_moments(_dense.stream(), src.data_ptr(), d + 7, Z.shape[0], d, last[:d].data_ptr(), last[d:].data_ptr(), N,
                                             res[:d].data_ptr(), res[d:2 * d].data_ptr(), res[2 * d:3 * d].data_ptr(), res[3 * d:].data_ptr()),
                       "bbbp_scaler_moments")
        torch.cuda.synchronize()
        check_src()
        check_res()
        host = res.cpu().numpy()
        assert host[3 * d:].view(np.int32)[0] == 0
        assert np.array_equal(_bits(host[:d]), _bits(m2)) and np.array_equal(_bits(host[d:2 * d]), _bits(v2)) and np.array_equal(_bits(host[2 * d:3 * d]), _bits(s2))
