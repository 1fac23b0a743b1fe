"""GPU: the three entries of ``csrc/ensemble.hip`` with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py) and with
their sources and destinations inside moats, at odd bases with padded leading dimensions.

The out-of-fold matrix, the averages, the counts and the label bytes are ``torch.empty``: the kernels have to write every cell they own and
nothing else, and may read nothing they were not given.  So under the three fills the results must equal the restatement's bit for bit,
and no guard band or moat may be touched.  65 rows put one row behind a wave, 257 one behind a block of 256 lanes."""
import numpy as np
import pytest
import torch

import ensemble_numpy as R
from bbbp_amd import ensemble
from poison import FILLS, moated, poisoned_allocations

pytestmark = pytest.mark.gpu

ROWS, M = (65, 257), 3


def _same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(R.bits(a), R.bits(b))


def _problem(m):
    """M probability pairs and 0 / 1 predictions per row, three test parts with interleaved row ids, non-dyadic weights."""
    rs = np.random.RandomState(m)
    p1 = rs.uniform(size=(M, m))
    P = np.stack([1.0 - p1, p1], axis=2)
    preds = rs.randint(0, 2, size=(M, m)).astype(np.uint8)
    ids = np.arange(m)
    parts = [ids[np.minimum(ids % 4, 2) == f] for f in range(3)]
    return P, preds, parts, rs.uniform(0.1, 2.0, M)


def _run(dev, P, preds, parts, w, place, meta=None):
    """The three entries once each; ``place(host array)`` puts a source on the device and returns (tensor, the checks to run afterwards)."""
    m, checks, entries = P.shape[1], [], []
    for j in range(M):
        for rows in parts:
            src, check = place(np.ascontiguousarray(P[j][rows]))                 # a learner's [count, 2] probabilities: the meta column is column 1
            checks.append(check)
            entries.append((src, 1, rows, j))
    if meta is None:
        meta = torch.empty((m, M), dtype=torch.float64, device=dev)
    ensemble._meta_scatter(entries, meta, M)
    placed = [place(np.ascontiguousarray(P[j])) for j in range(M)]
    avg, label = ensemble._soft_vote([t for t, _ in placed], w, R.scale(w))
    bytes_ = [place(np.ascontiguousarray(preds[j][:, None])) for j in range(M)]
    counts, hard = ensemble._hard_vote([t for t, _ in bytes_], w)
    torch.cuda.synchronize()
    for check in checks + [c for _, c in placed + bytes_]:
        check()
    return meta, avg, label, counts, hard


def _want(P, preds, parts, w):
    meta = np.full((P.shape[1], M), np.nan)
    for j in range(M):
        for rows in parts:
            meta[rows, j] = P[j][rows, 1]
    return (meta,) + R.soft_vote(list(P), w) + R.hard_vote(preds, w)


@pytest.mark.parametrize("m", ROWS)
def test_results_do_not_depend_on_the_fill(dev, monkeypatch, m):
    P, preds, parts, w = _problem(m)
    want = _want(P, preds, parts, w)
    plain = lambda a: (torch.from_numpy(a).to(dev), lambda: None)  # noqa: E731
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, P, preds, parts, w, plain)
        assert pa.check() >= 5, "the out-of-fold matrix, the averages, the counts and the label bytes did not go through the pools"
        pa.release()
        for i, (a, b) in enumerate(zip(got, want)):
            assert _same(a, b), f"fill {fill:#04x}: result {i} differs from the restatement"
        assert all(np.isin(a.cpu().numpy(), (0, 1)).all() for a in (got[2], got[4])), f"fill {fill:#04x}: a label byte was not written"


@pytest.mark.parametrize("m", ROWS)
def test_moated_sources_and_destination_with_odd_bases_and_padded_leading_dimensions(dev, monkeypatch, m):
    P, preds, parts, w = _problem(m)
    want = _want(P, preds, parts, w)
    for fill in FILLS:
        def place(a, fill=fill):
            return moated(torch.from_numpy(a), fill, ld=a.shape[1] + 3, offset=1, device=dev)
        meta, check_meta = moated((m, M), fill, ld=M + 2, offset=3, device=dev, dtype=torch.float64)
        assert meta.data_ptr() % 16 != 0 and meta.stride(0) == M + 2
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, P, preds, parts, w, place, meta)
        pa.check()
        pa.release()
        check_meta()
        for i, (a, b) in enumerate(zip(got, want)):
            assert _same(a.contiguous(), b), f"fill {fill:#04x}: result {i} differs from the restatement"
