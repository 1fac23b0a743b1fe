"""GPU: SMOTE, TomekLinks and SMOTETomek with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py), and with the
input matrix inside a moat at an odd base with a padded leading dimension.

The result matrix, the search's outputs and workspace and the keep mask are ``torch.empty``: the synthesis kernel has to write every
element of its rows and nothing else, the Tomek kernel every byte of its mask, and neither may read anything it was not given.  So under
the three fills the results must equal those of an unpoisoned run bit for bit, and no guard band or moat may be touched.  65 columns put
one element behind a wave-wide pass, 100 are the workload's."""
import numpy as np
import pytest
import torch

import smote_numpy as S
from bbbp_amd import imbalance
from poison import FILLS, moated, poisoned_allocations

pytestmark = pytest.mark.gpu

K, SEED = 5, 42
# (n, d, n_min, seed).  Seed 59 is the first of 1..59 for which the small set holds a Tomek link with a majority member (one; in 65
# dimensions most seeds give none); seed 11 is the first for which the large set (13 majority members) also has links in its SMOTE output (2).
SHAPES = [(65, 65, 7, 59), (257, 100, 64, 11)]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _run(dev, X, y):
    """Every path once: the three estimators, and the keep mask itself."""
    imb = imbalance
    tl = imb.TomekLinks(device=dev)
    out = [*imb.SMOTE(random_state=SEED, device=dev).fit_resample(X, y), *tl.fit_resample(X, y), tl.sample_indices_,
           *imb.SMOTETomek(random_state=SEED, device=dev).fit_resample(X, y)]
    Xd = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.array(X)).to(dev)
    nn1 = imb._neighbours(imb._fitted(Xd, dev), 1)
    keep = imb._keep_mask(nn1, torch.from_numpy(y.astype(np.int32)).to(dev), torch.tensor([1, 0], dtype=torch.uint8, device=dev))
    return [_bits(a) for a in out + [keep]]


def _problem(shape, dtype):
    X, y = S.problem(*shape, dtype=dtype)
    assert S.gap(X[y == 1], K) > 1 and S.gap(X, 1) > 1
    X_res, y_res = S.smote(X, y, K, SEED)
    assert S.gap(X_res, 1) > 1
    return X, y


def _check_against_the_restatement(got, X, y):
    want = [*S.smote(X, y, K, SEED), *S.tomek(X, y, "auto"), *S.smote_tomek(X, y, K, SEED)]
    want.append((~(S.tomek_members(X, y) & (y == 0))).astype(np.uint8))
    assert want[-1].min() == 0, "no Tomek link in the set: the mask check would be vacuous"
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, _bits(b)), f"result {i} differs from the restatement"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_results_do_not_depend_on_the_fill(dev, monkeypatch, shape, dtype):
    X, y = _problem(shape, dtype)
    want = _run(dev, X, y)
    _check_against_the_restatement(want, X, y)
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = _run(dev, X, y)
            torch.cuda.synchronize()
        assert pa.check() >= 6, "the result matrix, the search's outputs and the keep mask did not go through the pools"
        pa.release()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"fill {fill:#04x}: result {i} differs from the unpoisoned run"
        keep = got[-1]
        assert np.isin(keep, (0, 1)).all() and (fill in (0, 1) or not (keep == fill).any()), f"fill {fill:#04x}: a byte of the keep mask was not written"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_moated_input_with_an_odd_base_and_a_padded_leading_dimension(dev, monkeypatch, shape, dtype):
    X, y = _problem(shape, "float64" if dtype == torch.float64 else "float32")
    d = X.shape[1]
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
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"fill {fill:#04x}: result {i} differs"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_the_synthesis_kernel_reads_and_writes_moated_operands_in_place(dev, shape, dtype):
    """``bbbp_smote_synth`` itself on a class matrix and an output that both sit at an odd base with a padded leading dimension: the
    rows equal the restatement's and nothing outside the output's own elements is written."""
    X, y = _problem(shape, "float64" if dtype == torch.float64 else "float32")
    n, d = X.shape
    record = []
    X_res, _ = S.smote(X, y, K, SEED, record=record)
    (_, rows, _, steps), = record
    Xc = X[y == 1]
    nn = S.class_neighbours(Xc, K)
    rs = np.random.RandomState(SEED)
    idx = rs.randint(0, len(Xc) * K, size=len(rows))
    assert np.array_equal(idx // K, rows)
    for fill in FILLS:
        src, check_src = moated(torch.from_numpy(Xc), fill, ld=d + 7, offset=3, device=dev)
        out, check_out = moated((len(rows), d), fill, ld=d + 5, offset=1, device=dev, dtype=dtype)
        assert src.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
        imbalance._synthesize(src, torch.from_numpy(nn).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(steps).to(dev), out)
        torch.cuda.synchronize()
        check_src()
        check_out()
        assert np.array_equal(_bits(out), _bits(X_res[n:])), f"fill {fill:#04x}"
