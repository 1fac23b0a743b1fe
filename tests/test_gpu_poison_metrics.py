"""GPU: the three paths of ``bbbp_amd.metrics`` with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py), and with
the score and prediction matrices inside a moat at an odd base with a padded leading dimension.

The result words, the partial slabs of the pair kernel and the sums are ``torch.empty``: the kernels have to write every word of them
(no zero-filled output, no atomics) and may read nothing they were not given.  So under the three fills the results must equal those of
an unpoisoned run bit for bit, and no guard band or moat may be touched.  65 rows put one row behind a wave-wide pass, 257 one behind a
pair tile, 64 with three segments leave one segment without rows."""
import numpy as np
import pytest
import torch

import metrics_numpy as R
from bbbp_amd import metrics
from poison import FILLS, moated, poisoned_allocations

pytestmark = pytest.mark.gpu

SHAPES = [(65, 1, 1), (257, 5, 3), (64, 3, 3)]          # (n, M, G)


def _problem(n, M, G, dtype):
    y, pred, scores, groups = R.problem(n, M, G, dtype=np.dtype(dtype), left_out=G > 1)
    rs = np.random.RandomState(n)
    target = rs.randn(n)
    fitted = (target[None, :] + rs.randn(M, n)).astype(dtype)
    return y, pred, scores, groups, target, fitted


def _run(dev, y, pred, scores, groups, target, fitted):
    """Every path once: counts from bytes and from thresholded scores, pair counts, the eight scores, the squared-error sums."""
    cls = metrics.classification_scores(y, pred, scores, groups=groups, device=dev)
    out = [metrics.confusion_counts(y, pred, groups=groups, device=dev), metrics.confusion_counts(y, scores, groups=groups, threshold=0.5, device=dev),
           metrics.auc_pair_counts(y, scores, groups=groups, device=dev), *(cls[k] for k in metrics.KEYS),
           *metrics.squared_error_sums(target, fitted, groups=groups, device=dev)]
    return [R.bits(a) if a.dtype == np.float64 else a for a in out]


def _check_against_the_restatement(got, y, pred, scores, groups, target, fitted):
    cls = R.classification_scores(y, pred, scores, groups)
    want = [R.confusion_counts(y, pred, groups), R.confusion_counts(y, pred, groups), R.pair_counts(y, scores, groups),
            *(R.bits(cls[k]) for k in metrics.KEYS), *(R.bits(a) for a in R.squared_error_sums(target, fitted, groups))]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"result {i} differs from the restatement"


@pytest.mark.parametrize("n,M,G", SHAPES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_results_do_not_depend_on_the_fill(dev, monkeypatch, n, M, G, dtype):
    args = _problem(n, M, G, dtype)
    want = _run(dev, *args)
    _check_against_the_restatement(want, *args)
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, *args)
            torch.cuda.synchronize()
        assert pa.check() >= 6, "the result words, the slabs and the sums did not go through the pools"
        pa.release()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"fill {fill:#04x}: result {i} differs from the unpoisoned run"


@pytest.mark.parametrize("n,M,G", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_moated_inputs_with_an_odd_base_and_a_padded_leading_dimension(dev, monkeypatch, n, M, G, dtype):
    y, pred, scores, groups, target, fitted = _problem(n, M, G, "float64" if dtype == torch.float64 else "float32")
    want = _run(dev, y, pred, scores, groups, target, fitted)
    for fill in FILLS:
        sv, check_s = moated(torch.from_numpy(np.array(scores)), fill, ld=n + 7, offset=3, device=dev)
        fv, check_f = moated(torch.from_numpy(np.array(fitted)), fill, ld=n + 5, offset=1, device=dev)
        pv, check_p = moated(torch.from_numpy(np.array(pred)), fill, ld=n + 9, offset=5, device=dev)
        assert sv.stride(0) == n + 7 and sv.data_ptr() % 16 != 0 and pv.dtype == torch.uint8 and pv.data_ptr() % 4 != 0
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, y, pv, sv, groups, target, fv)
            torch.cuda.synchronize()
        pa.check()
        pa.release()
        check_s()
        check_f()
        check_p()
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"fill {fill:#04x}: result {i} differs"
