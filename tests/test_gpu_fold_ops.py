"""GPU: the kernels of csrc/fold.hip (outproj_fold_kernel, outproj_unfold_kernel) and csrc/encoder.hip: ln_param_grad_multi_kernel called
directly (ops.outproj_fold_fwd / outproj_fold_bwd / ln_param_grad) and held element-wise to the float64 oracle of tests/encoder_oracle.py.

Bounds.  Products: the form of test_gemm_layouts, |err| <= 2e-6 * (|A| @ |B|) per element (plus |bo| * 2^-23 where bo is added).  Column
sums (dbo, dgamma, dbeta): derived, not tuned -- a thread adds ceil(rows / lanes) terms in sequence and one thread then adds the `lanes`
partial sums in a fixed order (16 for dbo, 32 for the LayerNorm sums), so |err| <= (depth + 4) * 2^-24 * sum |terms| with depth that chain
length; the 4 covers forming dy * (z - mean) * rstd.  Every test prints the largest observed ratio to its bound."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import encoder_oracle as E
from bbbp_amd import _lib, ops
from poison import moated, poisoned_allocations

pytestmark = pytest.mark.gpu

NAN = 0xFF
GEMM_BOUND = 2e-6
U = 2.0 ** -24


def T(a, dev):
    return torch.tensor(a).to(dev)             # a copy: the cached references are read-only


def N(t):
    return t.detach().cpu().numpy()


def freeze(r):
    for v in vars(r).values():
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return r


def held(got, want, bound, what):
    """Every element finite and within ``bound``; returns (and prints) the largest ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, f"{what}: shapes {got.shape} {want.shape} {bound.shape}"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements are not finite"
    ratio = float((np.abs(got - want) / (bound + 1e-30)).max())
    print(f"[bound] {what}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: max err / bound = {ratio:.3f}"
    return ratio


def sum_bound(terms, lanes):
    """(depth + 4) * 2^-24 * sum |terms| over axis 0 for a column sum done as `lanes` strided sequential chains plus a chain over the partials."""
    depth = -(-terms.shape[0] // lanes) + lanes
    return (depth + 4) * U * np.abs(terms).sum(axis=0)


# ---- fold forward -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fold_reference(F, layers):
    win, bin_, wo, bo = E.fold_inputs(F, layers)
    r = SimpleNamespace(F=F, layers=layers, win=win, bin=bin_, wo=wo, bo=bo, with_bo=[], without=[], wbound=[], bbound=[])
    for l in range(layers):
        r.with_bo.append(E.fold(win[l], bin_[l], wo[l], bo[l]))
        r.without.append(E.fold(win[l], bin_[l], wo[l], None))
        awo = np.abs(wo[l].astype(np.float64))
        r.wbound.append(GEMM_BOUND * (awo @ np.abs(win[l][2 * F:].astype(np.float64))))
        r.bbound.append(GEMM_BOUND * (awo @ np.abs(bin_[l][2 * F:].astype(np.float64))))
    for lst in (r.with_bo, r.without):
        for tup in lst:
            for a in tup:
                a.setflags(write=False)
    return freeze(r)


def check_fold(r, o, with_bo, what):
    F = r.F
    worst = 0.0
    for l in range(r.layers):
        wf, bf, wvt = (N(o[n][l]) for n in ("wf", "bf", "wvt"))
        want_wf, want_bf, want_wvt = (r.with_bo if with_bo else r.without)[l]
        # the copied parts, bit for bit
        assert np.array_equal(wf[:2 * F].view(np.uint32), r.win[l][:2 * F].view(np.uint32)), f"{what} layer {l}: Wq; Wk"
        assert np.array_equal(bf[:2 * F].view(np.uint32), r.bin[l][:2 * F].view(np.uint32)), f"{what} layer {l}: bq; bk"
        want_t = np.ascontiguousarray(np.concatenate([r.win[l][2 * F:], r.bin[l][2 * F:, None]], axis=1).T)
        assert np.array_equal(wvt.view(np.uint32), want_t.view(np.uint32)), f"{what} layer {l}: [Wv | bv]^T"
        assert np.array_equal(want_wvt, want_t.astype(np.float64))
        worst = max(worst, held(wf[2 * F:], want_wf[2 * F:], r.wbound[l], f"{what} layer {l}: W' = Wo Wv"))
        bb = r.bbound[l] + (np.abs(r.bo[l].astype(np.float64)) * 2.0 ** -23 if with_bo else 0.0)
        worst = max(worst, held(bf[2 * F:], want_bf[2 * F:], bb, f"{what} layer {l}: b' = Wo bv" + (" + bo" if with_bo else "")))
    return worst


@pytest.mark.parametrize("with_bo", [True, False], ids=["bo", "no-bo"])
@pytest.mark.parametrize("F,layers", E.FOLD_LAYERS)
def test_fold_forward_against_float64(dev, F, layers, with_bo):
    """F = 1 .. 5: a single ragged row tile; 63 / 64 / 65: the bias column c = F as the last lane of the first column tile, alone in a second
    one, and beside one more column; 255: the widest supported (K + KB = 262 LDS words per row); 6 and 32 layers: blockIdx.y and every slot of
    the pointer table.  Two calls give equal bits."""
    assert _lib.lib().bbbp_outproj_fold_supported(F, 1, layers) == 1
    r = fold_reference(F, layers)
    args = [[T(a, dev) for a in lst] for lst in (r.win, r.bin, r.wo)]
    bo = [T(a, dev) for a in r.bo] if with_bo else None
    o = ops.outproj_fold_fwd(*args, bo)
    assert [len(o[n]) for n in ("wf", "bf", "wvt")] == [layers] * 3
    check_fold(r, o, with_bo, f"fold F={F} layers={layers}")
    again = ops.outproj_fold_fwd(*args, bo)
    for n in ("wf", "bf", "wvt"):
        for a, b in zip(o[n], again[n]):
            assert torch.equal(a, b), n


def test_fold_forward_refuses_what_it_does_not_support(dev):
    for F, layers in ((256, 1), (5, 33)):
        win, bin_, wo = ([torch.zeros(s, device=dev) for _ in range(layers)] for s in ((3 * F, F), (3 * F,), (F, F)))
        with pytest.raises(RuntimeError, match="not supported"):
            ops.outproj_fold_fwd(win, bin_, wo)
    with pytest.raises(RuntimeError, match="not supported"):
        ops.outproj_fold_bwd(*(torch.zeros(s, device=dev) for s in ((256, 256), (256,), (256, 256), (257, 256), (4, 256))))
    torch.cuda.synchronize()


# ---- fold backward ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unfold_reference(F, B):
    tdw, tdb, wo, wvt, dz = E.unfold_inputs(F, B)
    r = SimpleNamespace(F=F, B=B, tdw=tdw, tdb=tdb, wo=wo, wvt=wvt, dz=dz)
    r.g_outw, r.g_outb, r.g_inw_v, r.g_inb_v = E.unfold(tdw, tdb, wo, wvt, dz)
    td = np.abs(np.concatenate([tdw, tdb[:, None]], axis=1).astype(np.float64))              # [dW' | db']: [F, F + 1]
    awo_t = np.abs(wo.astype(np.float64)).T
    r.b_outw = GEMM_BOUND * (td @ np.abs(wvt.astype(np.float64)))                             # K = F + 1
    r.b_inw_v, r.b_inb_v = GEMM_BOUND * (awo_t @ td[:, :F]), GEMM_BOUND * (awo_t @ td[:, F])  # K = F
    r.b_outb = sum_bound(dz.astype(np.float64), 16)
    return freeze(r)


def check_unfold(r, o, what):
    ratios = [held(N(o[n]), getattr(r, n), getattr(r, "b_" + n[2:]), f"{what} {n}") for n in ("g_outw", "g_inw_v", "g_inb_v")]
    return max(ratios), held(N(o["g_outb"]), r.g_outb, r.b_outb, f"{what} g_outb (column sums)")


@pytest.mark.parametrize("pad", [0, 3], ids=["lddz=F", "lddz=F+3"])
@pytest.mark.parametrize("B", E.UNFOLD_BS)
@pytest.mark.parametrize("F", E.FOLD_FS)
def test_fold_backward_against_float64(dev, F, B, pad):
    """dWo = [dW' | db'] [Wv | bv]^T (K = F + 1), d[Wv | bv] = Wo^T [dW' | db'] (K = F, U read k-major), dbo = column sums of dz over 16 row
    groups: B = 1 (fifteen idle groups), 15 / 16 / 17 (one term short of, exactly, one past a full round), 100; dz dense and with padded rows."""
    r = unfold_reference(F, B)
    dz = torch.full((B, F + pad), float("nan"), device=dev)
    dz[:, :F] = T(r.dz, dev)
    ins = [T(getattr(r, n), dev) for n in ("tdw", "tdb", "wo", "wvt")]
    o = ops.outproj_fold_bwd(*ins, dz[:, :F])
    check_unfold(r, o, f"unfold F={F} B={B} lddz=F+{pad}")
    again = ops.outproj_fold_bwd(*ins, dz[:, :F])
    assert all(torch.equal(o[n], again[n]) for n in o)


# ---- LayerNorm parameter gradients ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_reference(n, rows, cols):
    ins = E.ln_grad_inputs(n, rows, cols)
    r = SimpleNamespace(n=n, rows=rows, cols=cols, ins=[list(t) for t in ins], want=[], bound=[])
    for dy, z, mean, rstd in ins:
        r.want.append(E.ln_param_grad(dy, z, mean, rstd))
        dy64 = dy.astype(np.float64)
        terms = dy64 * (z.astype(np.float64) - mean.astype(np.float64)[:, None]) * rstd.astype(np.float64)[:, None]
        r.bound.append((sum_bound(terms, 32), sum_bound(dy64, 32)))
    for lst in (r.ins, r.want, r.bound):
        for tup in lst:
            for a in tup:
                a.setflags(write=False)
    return r


def check_ln(r, o, what):
    worst = 0.0
    for i in range(r.n):
        worst = max(worst, held(N(o["dgamma"][i]), r.want[i][0], r.bound[i][0], f"{what} dgamma[{i}]"),
                    held(N(o["dbeta"][i]), r.want[i][1], r.bound[i][1], f"{what} dbeta[{i}]"))
    return worst


@pytest.mark.parametrize("n,rows,cols", E.LN_GRAD_CASES)
def test_ln_param_grad_against_float64(dev, n, rows, cols):
    """n = 1, 2, 12: one launch; 13: a second launch of one norm (slots 1 .. 11 of its table repeat norm 12); 25: three launches.  Every norm
    has its own tensors, so a pointer from the wrong slot gives another norm's sums.  rows 31 / 32 / 33: the 32 row lanes; cols 15 / 16 /
    17: the 16-column work-group."""
    r = ln_reference(n, rows, cols)
    lists = [[T(t[j], dev) for t in r.ins] for j in range(4)]
    o = ops.ln_param_grad(*lists)
    worst = check_ln(r, o, f"ln_param_grad n={n} rows={rows} cols={cols}")
    print(f"[bound] ln_param_grad n={n} rows={rows} cols={cols}: worst ratio {worst:.3f} of (ceil(rows/32) + 32 + 4) * 2^-24 * sum|terms|")
    again = ops.ln_param_grad(*lists)
    for k in ("dgamma", "dbeta"):
        assert all(torch.equal(a, b) for a, b in zip(o[k], again[k]))


# ---- under poison -----------------------------------------------------------------------------------------------------------------------------
class Pools:
    """Operands in moated pools with base offset 1: inputs between bands of ``fill``, outputs as NaN between NaN."""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.checks = dev, fill, []

    def put(self, a, ld=None):
        v, check = moated(torch.from_numpy(np.array(a)), self.fill, ld=ld, offset=1, device=self.dev)
        self.checks.append(check)
        return v

    def out(self, *shape, ld=None):
        v, check = moated(shape, NAN, ld=ld, offset=1, device=self.dev)
        self.checks.append(check)
        assert bool(v.isnan().all())
        return v

    def check(self):
        for c in self.checks:
            c()


@pytest.mark.parametrize("fill", [NAN, 0x7B], ids=["nan", "inputs-0x7b"])
def test_fold_forward_under_poison(dev, monkeypatch, fill):
    """F = 167, two layers, bo given: the K + KB LDS words past K, the rows past F of the last row tile and the lanes past F + 1 of the last
    column tile may not come from the caller's memory.  The second run puts the inputs between bands of 0x7B (1.3e36): a value computed
    from a stray load does not look like the outputs' NaN moat (see test_gemm_family_under_poison)."""
    F, layers = 167, 2
    r = fold_reference(F, layers)
    P = Pools(dev, fill)
    win, bin_, wo, bo = ([P.put(a) for a in lst] for lst in (r.win, r.bin, r.wo, r.bo))
    out = {"wf": [P.out(3 * F, F) for _ in range(layers)], "bf": [P.out(3 * F) for _ in range(layers)], "wvt": [P.out(F + 1, F) for _ in range(layers)]}
    with poisoned_allocations(monkeypatch, NAN) as pa:
        o = ops.outproj_fold_fwd(win, bin_, wo, bo, out=out)
    assert len(pa.pools) == 0 and all(o[n][l] is out[n][l] for n in out for l in range(layers))
    check_fold(r, o, True, f"poisoned fold F={F}")
    P.check()


@pytest.mark.parametrize("fill", [NAN, 0x7B], ids=["nan", "inputs-0x7b"])
def test_fold_backward_under_poison(dev, monkeypatch, fill):
    """F = 167, B = 37, dz with row stride F + 3."""
    F, B = 167, 37
    r = unfold_reference(F, B)
    P = Pools(dev, fill)
    ins = [P.put(getattr(r, n)) for n in ("tdw", "tdb", "wo", "wvt")]
    dz = P.put(r.dz, ld=F + 3)
    out = {"g_outw": P.out(F, F), "g_outb": P.out(F), "g_inw_v": P.out(F, F), "g_inb_v": P.out(F)}
    with poisoned_allocations(monkeypatch, NAN) as pa:
        o = ops.outproj_fold_bwd(*ins, dz, out=out)
    assert len(pa.pools) == 0 and all(o[n] is out[n] for n in out)
    check_unfold(r, o, f"poisoned unfold F={F} B={B}")
    P.check()


@pytest.mark.parametrize("fill", [NAN, 0x7B], ids=["nan", "inputs-0x7b"])
def test_ln_param_grad_under_poison(dev, monkeypatch, fill):
    """13 norms (two launches) of 33 x 17: ragged in rows and columns."""
    n, rows, cols = 13, 33, 17
    r = ln_reference(n, rows, cols)
    P = Pools(dev, fill)
    lists = [[P.put(t[j]) for t in r.ins] for j in range(4)]
    out = {"dgamma": [P.out(cols) for _ in range(n)], "dbeta": [P.out(cols) for _ in range(n)]}
    with poisoned_allocations(monkeypatch, NAN) as pa:
        o = ops.ln_param_grad(*lists, out=out)
    assert len(pa.pools) == 0 and all(o[k][i] is out[k][i] for k in out for i in range(n))
    check_ln(r, o, f"poisoned ln_param_grad n={n}")
    P.check()
