"""GPU: the pack, count and jll paths of naive_bayes with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py), and
with the input matrix inside a moat at an odd base with a padded leading dimension.

The packed words, the counts and the joint log-likelihoods are ``torch.empty``: the pack kernel has to write every word whole, the
padding bits of the last word of a plane or a row as 0, and the count and jll kernels may read nothing else.  So under the three fills
the results must equal those of an unpoisoned run bit for bit -- a difference is a read of memory the kernels do not own -- and no guard
band or moat may be touched.  65 rows and 65 features put one bit into the last word of both layouts."""
import numpy as np
import pytest
import torch

import bnb_numpy as N
from poison import FILLS, moated, poisoned_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(65, 65), (257, 100), (64, 130)]
THRESHOLDS = [0.0, 0.5]


def NB():
    from bbbp_amd import naive_bayes
    return naive_bayes


def _run(dev, X, y):
    """Every path once: a batch of fits, the packed words themselves, single and batched joint log-likelihoods."""
    nb = NB()
    n = len(y)
    rows = [None, np.arange(n - 1, -1, -2), np.array([0, 1, n - 1])]
    models = nb.fit_masks(X, y, rows, THRESHOLDS, [0.5, 1.0], device=dev)
    out = [a for m in models for a in (m.feature_count_, m.class_count_, m.feature_log_prob_, m.class_log_prior_)]
    out += [models[0].predict_joint_log_proba(X), models[3].predict_log_proba(X)]
    out = [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in out]
    bits = nb._Bits(X, THRESHOLDS, dev)
    out += [bits.planes.cpu().numpy(), bits.rowwords.cpu().numpy()]
    w, c = np.stack([m._w for m in models[:4]]), np.stack([m._c for m in models[:4]])
    out += bits.jll(w, c, [0, 0, 1, 1], [None, rows[1], rows[2], None])
    return out


def _padding_is_zero(planes, rowwords, n, d):
    tail_n, tail_d = n % 64, d % 64
    ok = True
    if tail_n:
        ok &= not (planes[:, :, -1].view(np.uint64) >> np.uint64(tail_n)).any()
    if tail_d:
        ok &= not (rowwords[:, :, -1].view(np.uint64) >> np.uint64(tail_d)).any()
    return bool(ok)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_results_do_not_depend_on_the_fill(dev, monkeypatch, n, d, dtype):
    X, y = N.gaussian_problem(n, d, dtype=dtype)
    want = _run(dev, X, y)
    # the unpoisoned run is the restatement's
    B = [N.binarise(X, t) for t in THRESHOLDS]
    planes, rowwords = want[-6], want[-5]
    for t in range(2):
        full = np.zeros((n, -(-d // 64) * 64), dtype=bool)
        full[:, :d] = B[t]
        assert np.array_equal(np.packbits(full, axis=1, bitorder="little").view("<u8"), rowwords[t].view(np.uint64))
        full = np.zeros((d, -(-n // 64) * 64), dtype=bool)
        full[:, :n] = B[t].T
        assert np.array_equal(np.packbits(full, axis=1, bitorder="little").view("<u8"), planes[t].view(np.uint64))
    assert _padding_is_zero(planes, rowwords, n, d)
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, X, y)
            torch.cuda.synchronize()
        assert pa.check() >= 6, "the packed words, the counts and the results did not go through the pools"
        pa.release()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                                                                 b.view(np.int64) if b.dtype == np.float64 else b), \
                f"fill {fill:#04x}: result {i} differs from the unpoisoned run"


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_moated_input_with_an_odd_base_and_a_padded_leading_dimension(dev, monkeypatch, n, d, dtype):
    X, y = N.gaussian_problem(n, d, dtype="float64" if dtype == torch.float64 else "float32")
    want = _run(dev, X, y)
    for fill in FILLS:
        view, check = moated(torch.from_numpy(np.array(X)), fill, ld=d + 7, offset=3, device=dev)
        assert view.stride(0) == d + 7 and view.data_ptr() % 16 != 0
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, view, y)
            torch.cuda.synchronize()
        pa.check()
        pa.release()
        check()
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                                         b.view(np.int64) if b.dtype == np.float64 else b), f"fill {fill:#04x}: result {i} differs"
