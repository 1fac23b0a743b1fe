"""GPU: the float64 tile product (csrc/f64_tile.h) computes bit for bit what it computed before pca.hip and knn.hip shared it.

tests/golden/f64_digests.json holds, group by group and for every case below, the SHA-256 of the raw output bytes of the public call
(decomposition.gemm_f64c, NearestNeighbors.kneighbors, KNeighborsClassifier.predict_proba).  It was recorded with tools/record_f64_digests.py from a build of the
commit BEFORE that refactor (`BBBP_LIB=<that build's libbbbp_hip.so> python tools/record_f64_digests.py`), never from the code under test;
`--check` against that build reproduces it.  The float64 path's outputs do not depend on the slab / slice count or on the run, so equal
digests are the whole statement.  Shapes are the smallest at which the shared code takes each of its paths: ragged tiles in both directions,
K of 1 / 15 / 16 / 17 / 37 (no prefetch, ragged last chunk, exactly one chunk, one chunk and an element, three chunks), K = 533 cut into 1,
3, 13 and 34 slabs and K = 17 cut into 3 (34 slabs of one chunk each; with 13, and with 3 at K = 17, the last slab owns no chunk and the
product takes its empty-range exit), operands that are views of wider pools.  Inputs are exact in float32, so every dtype pair sees the
same numbers."""
import functools
import hashlib
import itertools
import json
import os

import numpy as np
import pytest
import torch

from bbbp_amd.decomposition import gemm_f64c
from bbbp_amd.neighbors import KNeighborsClassifier, NearestNeighbors

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f64_digests.json")
DT = {"f32": torch.float32, "f64": torch.float64}
PAIRS = (("f32", "f32"), ("f64", "f64"), ("f32", "f64"), ("f64", "f32"))
# (K, split_k).  split_k = 3 at K = 17 leaves slab 2 of 3 without a chunk (2 chunks, 1 per slab); 13 at K = 533 leaves slab 12 without one
# (34 chunks, 3 per slab); 34 gives every slab exactly one chunk.
GEMM_M, GEMM_N, GEMM_KS = 65, 63, ((1, 0), (15, 0), (16, 0), (17, 0), (17, 3), (37, 0), (533, 1), (533, 3), (533, 13), (533, 34))
SYM_M, SYM_K, SYM_SPLITS = 130, 37, (1, 2)
KNN_MS, KNN_DS, KNN_KS, KNN_SLICES = (1, 65), (1, 16, 17, 167), (1, 7, 32), (1, 3)
POOL_K, POOL_D = 600, 200         # pool widths: leading dimensions differ from K / d
GROUPS = ("gemm-NT", "gemm-TN", "symmetric", "knn-n65", "knn-n333", "knn-self", "proba")


@functools.lru_cache(maxsize=None)
def _pool():
    """Device pools drawn once from numpy.random.default_rng, rounded to float32 first: {(name, dtype): tensor}."""
    rng = np.random.default_rng(20240607)
    host = {"nt": rng.standard_normal((2, SYM_M, POOL_K)) + 2.0, "tn": rng.standard_normal((2, POOL_K, SYM_M)) + 2.0,
            "q": 3.0 * rng.standard_normal((65, POOL_D)) + 1.0, "t": 3.0 * rng.standard_normal((333, POOL_D)) + 1.0}
    out = {}
    for name, v in host.items():
        v32 = v.astype(np.float32)
        out[name, "f32"], out[name, "f64"] = torch.from_numpy(v32).cuda(), torch.from_numpy(v32.astype(np.float64)).cuda()
    out["shift"] = torch.from_numpy(rng.standard_normal((2, POOL_K)).astype(np.float32).astype(np.float64) + 2.0).cuda()
    out["scale"] = torch.from_numpy(rng.standard_normal(SYM_M).astype(np.float32).astype(np.float64) + 2.0).cuda()
    out["labels"] = rng.integers(0, 3, 333)
    return out


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def _operand(layout, which, dt, rows, K):
    return _pool()["nt", dt][which, :rows, :K] if layout == "NT" else _pool()["tn", dt][which, :K, :rows]


def _shift(layout, which, rows, K):
    return _pool()["shift"][which, :(K if layout == "NT" else rows)].contiguous()


def _gemm(layout):
    out = {}
    for (adt, bdt), odt, shift, (K, split) in itertools.product(PAIRS, ("f32", "f64"), (0, 1), GEMM_KS):
        A, B = _operand(layout, 0, adt, GEMM_M, K), _operand(layout, 1, bdt, GEMM_N, K)
        sa, sb = (_shift(layout, 0, GEMM_M, K), _shift(layout, 1, GEMM_N, K)) if shift else (None, None)
        C = gemm_f64c(A, B, layout=layout, a_shift=sa, b_shift=sb, row_scale=_pool()["scale"][:GEMM_M].contiguous(), out_dtype=DT[odt],
                      split_k=split)
        out[f"gemm-{layout}-{adt}x{bdt}-out{odt}-shift{shift}-K{K}-split{split}"] = _sha(C)
    return out


def _symmetric():
    out = {}
    for layout, dt, split in itertools.product(("NT", "TN"), ("f32", "f64"), SYM_SPLITS):
        A, s = _operand(layout, 0, dt, SYM_M, SYM_K), _shift(layout, 0, SYM_M, SYM_K)
        C = gemm_f64c(A, A, layout=layout, a_shift=s, b_shift=s, symmetric=True, split_k=split)
        assert torch.equal(C, C.T), f"symmetric {layout} {dt} split {split}: not bitwise symmetric"
        out[f"symmetric-{layout}-{dt}-split{split}"] = _sha(C)
    return out


def _knn(n, exclude_self):
    out = {}
    for d, (qdt, tdt) in itertools.product(KNN_DS, PAIRS):
        if exclude_self and qdt != tdt:
            continue
        T = _pool()["t", tdt][:n, :d]
        assert T.stride(0) == POOL_D
        nn = NearestNeighbors().fit(T)
        for m, k, slices in itertools.product((n,) if exclude_self else KNN_MS, KNN_KS, KNN_SLICES):
            if k > (n - 1 if exclude_self else n):
                continue
            if exclude_self:
                dist, ind = map(torch.from_numpy, nn.kneighbors(None, k, slices=slices))
            else:
                dist, ind = nn.kneighbors(_pool()["q", qdt][:m, :d], k, slices=slices)
            cid = f"knn-{'self' if exclude_self else 'm%d' % m}-n{n}-d{d}-k{k}-{qdt}x{tdt}-slices{slices}"
            out[cid + "-dist"], out[cid + "-ind"] = _sha(dist), _sha(ind)
    return out


def _proba():
    out = {}
    for weights in ("uniform", "distance"):
        clf = KNeighborsClassifier(7, weights=weights).fit(_pool()["t", "f64"][:333, :17], _pool()["labels"])
        out[f"proba-m65-n333-d17-k7-{weights}"] = _sha(clf.predict_proba(_pool()["q", "f64"][:65, :17]))
    return out


def compute_digests(group):
    """{case id: SHA-256 of the output bytes} of one group, with whatever library bbbp_amd._lib has loaded."""
    if group.startswith("gemm-"):
        return _gemm(group[5:])
    if group.startswith("knn-n"):
        return _knn(int(group[5:]), False)
    return {"symmetric": _symmetric, "knn-self": lambda: _knn(333, True), "proba": _proba}[group]()


@pytest.mark.parametrize("group", GROUPS)
def test_outputs_are_bit_identical_to_the_recorded_build(dev, group):
    got = compute_digests(group)
    with open(DIGESTS) as f:
        want = json.load(f)[group]
    assert sorted(got) == sorted(want), f"{group}: the case list differs from the recorded one"
    differ = [k for k in got if got[k] != want[k]]
    assert not differ, f"{group}: {len(differ)} of {len(got)} outputs differ from the recorded build, first: {differ[:5]}"
