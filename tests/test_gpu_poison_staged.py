"""GPU: staged prediction with every ``torch.empty`` served from poisoned, guarded pools (tests/poison.py), and the entry points called
directly on an output inside a moat whose leading dimension exceeds the row count.

The stage matrix and the leaf scratch are ``torch.empty``: the kernels have to write every word they later read or return, may not
depend on what those buffers held, and may not store outside them -- neither behind the last chunk of the last stage nor into the
padded tail ``out[k][n .. ldo)`` of a row.  So under the three fills the matrices equal those of an unpoisoned run bit for bit and no
guard band or moat is touched.  T = 7 at period 3 ends in a short stage; 257 rows at 100 per call end in a chunk of 57."""
import numpy as np
import pytest
import torch

import staged_numpy as S
from bbbp_amd import _lib, boosters, ops
from poison import FILLS, moated, poisoned_allocations

pytestmark = pytest.mark.gpu

D = 9
CASES = [(7, 257, 0, None, 3, 100), (7, 257, 1, 6, 2, None), (40, 65, 0, None, 1, 64)]      # T, n, start, end, period, rows_per_call
BUILD = {"gbt": (S.random_gbt, S.xgb_trees, S.staged_gbt), "oblivious": (S.random_oblivious, S.cat_trees, S.staged_oblivious)}


def run(trees, X, start, end, period, rows_per_call):
    kw = {} if rows_per_call is None else dict(rows_per_call=rows_per_call)
    return S.bits(trees.staged_predict_device(X, start, end, period, **kw).cpu().numpy())


@pytest.mark.parametrize("T,n,start,end,period,rows_per_call", CASES)
@pytest.mark.parametrize("family", list(BUILD))
def test_staged_matrices_do_not_depend_on_the_fill(dev, monkeypatch, family, T, n, start, end, period, rows_per_call):
    make, build, staged_of = BUILD[family]
    model, X = make(T, D, seed=100 + T), S.queries(n, D, seed=n)
    trees = build(model, dev)
    Xd = torch.from_numpy(X).to(dev)
    want = run(trees, Xd, start, end, period, rows_per_call)
    assert np.array_equal(want, S.bits(staged_of(model, X, boosters.stage_ends(T, start, end, period), start)))
    for fill in FILLS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            got = run(trees, Xd, start, end, period, rows_per_call)
            torch.cuda.synchronize()
        assert pa.check() >= 2, "the stage matrix and the leaf scratch did not go through the pools"
        pa.release()
        assert got.shape == want.shape and np.array_equal(got, want), f"fill {fill:#04x}: the matrix differs from the unpoisoned run"


@pytest.mark.parametrize("family", list(BUILD))
def test_padded_output_rows_are_left_alone(dev, family):
    """The C entry points on ``out`` with ``ldo = n + 5`` at an odd base: the stages land in ``out[k][0 .. n)`` and nothing else is written."""
    make, build, staged_of = BUILD[family]
    T, n, start, end, period = 7, 257, 1, 7, 4
    model, X = make(T, D, seed=100 + T), S.queries(n, D, seed=n)
    trees = build(model, dev)
    d, Xd = trees._on_device(), torch.from_numpy(X).to(dev)
    ends = boosters.stage_ends(T, start, end, period)
    want = S.bits(staged_of(model, X, ends, start))
    dtype = torch.float32 if family == "gbt" else torch.float64
    L = _lib.lib()
    for fill in FILLS:
        out, check_out = moated((len(ends), n), fill, ld=n + 5, offset=1, device=dev, dtype=dtype)
        scratch, check_scratch = moated((end - start, n), fill, device=dev, dtype=dtype)
        if family == "gbt":
            rc = L.bbbp_gbt_staged_predict(ops._stream(), Xd.data_ptr(), n, D, d["left"].data_ptr(), d["right"].data_ptr(), d["feature"].data_ptr(),
                                           d["cond"].data_ptr(), d["default_left"].data_ptr(), d["root"].data_ptr(), T, trees.base_score, start, end,
                                           period, scratch.data_ptr(), out.data_ptr(), n + 5)
        else:
            rc = L.bbbp_oblivious_staged_predict(ops._stream(), Xd.data_ptr(), n, D, d["split_feature"].data_ptr(), d["split_border"].data_ptr(),
                                                 d["nan_true"].data_ptr(), d["tree_first_split"].data_ptr(), d["tree_first_leaf"].data_ptr(),
                                                 d["leaf_values"].data_ptr(), T, trees.scale, trees.bias, start, end, period, scratch.data_ptr(),
                                                 out.data_ptr(), n + 5)
        _lib.check(rc, "staged predict")
        torch.cuda.synchronize()
        assert out.stride(0) == n + 5 and np.array_equal(S.bits(out.cpu().numpy()), want), f"fill {fill:#04x}"
        check_out()
        check_scratch()
