"""GPU: the row-fused stretches of csrc/encoder.hip (enc_row_fwd_kernel / enc_row_bwd_kernel) called directly (ops.encoder_rows_fwd /
encoder_rows_bwd) and compared element-wise with the float64 oracle of tests/encoder_oracle.py, whose dropout masks are the exact Philox
stream of tests/rowops_oracle.py -- not another kernel's.

Shapes: B = 1 / 16 / 17 / 37 (one row, a full block, a block plus one row, three blocks with a ragged last one); F = 4 and 15 (every product
is only the clamped tail chunk), 16 / 17, 64, 167, 192 (the widest: LDS rows of exactly MAXF); DFF = 16, 18 and 70 (DFF % 4 != 0: the scalar
epilogue of the last lanes), 272 (17 column tiles: the 16-tile wave pass wraps), and 2048 with F = 167 at B = 37, the real widths.  Every
output of every case is held to the project's float32-against-float64 tolerance.  The backward cases take the float32 casts of the
oracle's forward as their saved activations and the oracle evaluates the backward in float64 from those casts: both sides see the same
gates."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import encoder_oracle as E
from bbbp_amd import _lib, ops
from helpers import assert_close, assert_close_or_as_accurate_as_fp32
from poison import moated, poisoned_allocations

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol_frac=2e-5)          # float32 kernels against float64, as tests/test_gpu_attention.py
NAN = 0xFF
WORST = {}                                     # op -> largest err / tolerance seen in this session (printed per case)


def T(a, dev):
    return torch.tensor(a).to(dev)             # a copy: the cached references are read-only


def N(t):
    return t.detach().cpu().numpy()


def ratio(got, want, rtol, atol_frac):
    want = np.asarray(want, dtype=np.float64)
    tol = rtol * np.abs(want) + atol_frac * float(np.abs(want).max()) + 1e-30
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / tol).max())


def close(op, got, want, what):
    """assert_close at TOL, after printing the observed err / tolerance (the summary's figures)."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements are not finite"
    r = ratio(got, want, **TOL)
    WORST[op] = max(WORST.get(op, 0.0), r)
    print(f"[tol] {what}: max err / tol = {r:.3f} (worst {op} so far {WORST[op]:.3f})")
    assert_close(got, want, what=what, **TOL)


@functools.lru_cache(maxsize=None)
def reference(B, F, DFF, kind="none", p=0.0, seeds=E.ROW_SEEDS, base=None, shifted=False, f32=False):
    """Inputs and float64 results of one case, forward and backward (computed once, shared, read-only)."""
    ctx, xin, w, dyout, up = E.row_inputs(B, F, DFF, shifted=shifted)
    nxt = E.next_projection(kind, F)
    r = SimpleNamespace(B=B, F=F, DFF=DFF, kind=kind, p=p, seeds=seeds, base=base, ctx=ctx, xin=xin, w=w, dyout=dyout, up=up, nxt=nxt,
                        what=f"B={B} F={F} DFF={DFF} next={kind} p={p}" + (" shifted" if shifted else ""))
    r.fwd = E.rows_fwd(ctx, xin, w, p=p, seeds=seeds, base=base, next=nxt)
    r.fwd32 = E.rows_fwd(ctx, xin, w, p=p, seeds=seeds, base=base, next=nxt, dtype=np.float32) if f32 else None
    r.saved = {n: r.fwd[n].astype(np.float32) for n in E.SAVED_NAMES}
    kw = dict(p=p, seeds=(seeds[0], seeds[2]), base=base)
    r.bwd = E.rows_bwd(r.saved, w, dyout=dyout, **kw)
    r.bwd0 = E.rows_bwd(r.saved, w, up=up, **kw)
    for d in (w, up, r.saved, r.fwd, r.bwd, r.bwd0, nxt or {}, r.fwd32 or {}):
        for v in d.values():
            for a in (v if isinstance(v, tuple) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    for a in (ctx, xin, dyout):
        a.setflags(write=False)
    return r


def run_fwd(dev, r, out=None, wide=None):
    """ops.encoder_rows_fwd on a case's inputs.  The fingerprint_fc form of the next projection writes the left half of a [B, 256] buffer
    (``wide``, or a new NaN-filled one), whose right half must stay as it was."""
    w = {k: T(v, dev) for k, v in r.w.items()}
    nxt = None
    if r.nxt is not None:
        nxt = dict(wn=T(r.nxt["wn"], dev), bn=T(r.nxt["bn"], dev), act=r.nxt["act"])
        if r.kind == "fc":
            wide = torch.full((r.B, 256), float("nan"), device=dev) if wide is None else wide
            nxt["outn"] = wide[:, :128]
    o = ops.encoder_rows_fwd(T(r.ctx, dev), T(r.xin, dev), w, p=r.p, seeds=r.seeds, nxt=nxt, out=out)
    if r.kind == "fc":
        assert o["outn"].data_ptr() == wide.data_ptr() and bool(wide[:, 128:].isnan().all()), f"{r.what}: the right half of the wide buffer was written"
    return o


def check_fwd(r, o):
    for n in E.FWD_NAMES + (("outn",) if r.nxt is not None else ()):
        close("rows_fwd", N(o[n]), r.fwd[n], f"{r.what} {n}")
    assert (o["outn"] is None) == (r.nxt is None)
    if r.p > 0:
        hff, k2 = N(o["hff"]), r.fwd["masks"][1]
        assert not hff[k2 == 0].any(), f"{r.what}: hff is not 0 at {int((hff[k2 == 0] != 0).sum())} dropped elements"
        alive = (k2 != 0) & (r.fwd["pre"] > 1e-3)
        assert hff[alive].all(), f"{r.what}: hff is 0 at {int((hff[alive] == 0).sum())} kept, active elements"
        assert 0.5 * r.p < (k2 == 0).mean() < 1.5 * r.p or k2.size < 2000


def run_bwd(dev, r, stage0, out=None):
    saved = {k: T(v, dev) for k, v in r.saved.items()}
    w = {k: T(r.w[k], dev) for k in ("g1", "g2", "w1", "w2", "wo")}
    kw = dict(p=r.p, seeds=(r.seeds[0], r.seeds[2]), out=out)
    if stage0:
        return ops.encoder_rows_bwd(saved, w, up={k: T(v, dev) for k, v in r.up.items()}, **kw)
    dyout = T(r.dyout, dev)
    o = ops.encoder_rows_bwd(saved, w, dyout=dyout, **kw)
    assert o["dyout"] is dyout and np.array_equal(N(dyout), r.dyout)                    # read, not written
    return o


def check_bwd(r, o, stage0):
    want = r.bwd0 if stage0 else r.bwd
    for n in E.BWD_NAMES:
        close("rows_bwd", N(o[n]), want[n], f"{r.what} stage0={int(stage0)} {n}")


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------------
GRID = [(F, DFF) for F in E.ROW_FS for DFF in E.ROW_DFFS]


@pytest.mark.parametrize("F,DFF", GRID)
def test_row_forward_against_float64(dev, F, DFF):
    """Every B x next projection x p of one (F, DFF): 24 launches, each output of each against the oracle; with dropout, hff is exactly 0 where
    the oracle's stream drops it and non-zero where it keeps an active unit, and z1 / z2 carry the oracle's masks of sites 1 and 3."""
    assert _lib.lib().bbbp_encoder_rows_supported(F, 1, DFF) == 1
    for B in E.ROW_BS:
        for kind in E.NEXT_KINDS:
            for p in E.ROW_PS:
                r = reference(B, F, DFF, kind, p)
                check_fwd(r, run_fwd(dev, r))


@pytest.mark.parametrize("F,DFF", GRID)
def test_row_backward_against_float64(dev, F, DFF):
    """Every B x (dyout read | stage 0 from the layer above) x p of one (F, DFF): all eight outputs, every element."""
    for B in E.ROW_BS:
        for p in E.ROW_PS:
            r = reference(B, F, DFF, "none", p)
            for stage0 in (False, True):
                check_bwd(r, run_bwd(dev, r, stage0), stage0)


@pytest.mark.parametrize("kind", E.NEXT_KINDS)
@pytest.mark.parametrize("p", E.ROW_PS)
def test_rows_at_the_real_widths_against_float64(dev, kind, p):
    """F = 167, DFF = 2048, B = 37: 128 column tiles of linear1, a 2048-deep K of linear2 read back from global memory."""
    r = reference(37, 167, 2048, kind, p)
    check_fwd(r, run_fwd(dev, r))
    for stage0 in (False, True):
        check_bwd(r, run_bwd(dev, r, stage0), stage0)


# ---- dropout streams --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,DFF", [(37, 167, 70), (17, 16, 18)])
def test_dropout_with_seeds_above_2_to_32(dev, B, F, DFF):
    """The upper key word of the three streams; F = 167: rows start anywhere in a Philox block (dropout_scale4 stitches two blocks)."""
    r = reference(B, F, DFF, "in_proj", 0.1, seeds=E.HIGH_SEEDS)
    low = reference(B, F, DFF, "in_proj", 0.1)
    assert not np.array_equal(r.fwd["masks"][1], low.fwd["masks"][1])
    check_fwd(r, run_fwd(dev, r))
    for stage0 in (False, True):
        check_bwd(r, run_bwd(dev, r, stage0), stage0)


def test_dropout_under_a_seed_base(dev):
    B, F, DFF = 37, 167, 70
    r = reference(B, F, DFF, "fc", 0.1, seeds=E.HIGH_SEEDS, base=E.SEED_BASE)
    base_t = torch.full((1,), E.SEED_BASE, dtype=torch.int64, device=dev)
    ops.set_seed_base(base_t.data_ptr())
    try:
        fwd = run_fwd(dev, r)
        bwd = [run_bwd(dev, r, stage0) for stage0 in (False, True)]
        torch.cuda.synchronize()
    finally:
        ops.set_seed_base(0)
    check_fwd(r, fwd)
    for stage0, o in zip((False, True), bwd):
        check_bwd(r, o, stage0)
    plain = reference(B, F, DFF, "fc", 0.1, seeds=E.HIGH_SEEDS)                 # restored: no base
    assert not np.array_equal(plain.fwd["masks"][0], r.fwd["masks"][0])
    check_fwd(plain, run_fwd(dev, plain))


# ---- rows whose mean dwarfs their spread ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", E.ROW_PS)
def test_rows_with_a_mean_far_above_their_spread(dev, p):
    """A third of the rows of x carry +30 (as test_layernorm_absorbed_by_the_consuming_linear): LayerNorm1 subtracts a mean thirty times the
    spread.  Held to what float32 gives on the same input: within the float64 tolerance, or no worse than 2 x the oracle's float32
    evaluation."""
    r = reference(37, 167, 272, "in_proj", p, shifted=True, f32=True)
    o = run_fwd(dev, r)
    for n in E.FWD_NAMES + ("outn",):
        got, want, want32 = N(o[n]).astype(np.float64), r.fwd[n], r.fwd32[n]
        err, ref = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
        print(f"[fp32-yardstick] {r.what} {n}: kernel {err:.3e} float32 {ref:.3e} scale {np.abs(want).max():.3e}")
        assert np.isfinite(got).all()
        assert_close_or_as_accurate_as_fp32(got, want, want32, what=f"{r.what} {n}")


# ---- two calls, and the launch-per-op chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,DFF,p", [(37, 167, 272, 0.1), (17, 15, 18, 0.0)])
def test_two_calls_are_bit_identical(dev, B, F, DFF, p):
    r = reference(B, F, DFF, "in_proj", p)
    a, b = run_fwd(dev, r), run_fwd(dev, r)
    assert all(torch.equal(a[n], b[n]) for n in E.FWD_NAMES + ("outn",))
    for stage0 in (False, True):
        a, b = run_bwd(dev, r, stage0), run_bwd(dev, r, stage0)
        assert all(torch.equal(a[n], b[n]) for n in E.BWD_NAMES)


def chain_close(got, want, what):
    """The bound test_fused_encoder_rows_match_the_launch_per_op_schedule holds the two schedules to at B <= 64."""
    got, want = got.double(), want.double()
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"[chain] {what}: max err {err:.3e} = {err / (1e-4 * scale + 1e-12):.3f} of 1e-4 x max {scale:.3e}")
    assert err <= 1e-4 * scale + 1e-12, (what, err, scale)


def test_row_forward_agrees_with_the_launch_per_op_chain(dev):
    """F = 167, DFF = 2048, B = 37, p = 0.1: the same stretch as ops.gemm / layernorm_fwd / dropout launches.  Both draw the same streams: hff
    has the same zeros, and every tensor agrees to summation-order rounding."""
    r = reference(37, 167, 2048, "in_proj", 0.1)
    o = run_fwd(dev, r)
    w = {k: T(v, dev) for k, v in r.w.items()}
    s1, s2, s3 = r.seeds
    sa = ops.gemm(T(r.ctx, dev), w["wo"], trans_b=True, bias=w["bo"])
    y1, z1, mean1, rstd1 = ops.layernorm_fwd(sa, T(r.xin, dev), w["g1"], w["be1"], dropout_p=r.p, seed=s1)
    hff = ops.dropout(ops.gemm(y1, w["w1"], trans_b=True, bias=w["b1"], act="relu"), r.p, s2)
    ff = ops.gemm(hff, w["w2"], trans_b=True, bias=w["b2"])
    y2, z2, mean2, rstd2 = ops.layernorm_fwd(ff, y1, w["g2"], w["be2"], dropout_p=r.p, seed=s3)
    outn = ops.gemm(y2, T(r.nxt["wn"], dev), trans_b=True, bias=T(r.nxt["bn"], dev))
    assert torch.equal(o["hff"] == 0, hff == 0), f"{int(((o['hff'] == 0) != (hff == 0)).sum())} elements of hff are zero in one schedule only"
    for n, t in (("z1", z1), ("y1", y1), ("hff", hff), ("z2", z2), ("y2", y2), ("mean1", mean1), ("rstd1", rstd1), ("mean2", mean2),
                 ("rstd2", rstd2), ("outn", outn)):
        chain_close(o[n], t, f"forward {n}")


def test_row_backward_agrees_with_the_launch_per_op_chain(dev):
    """The same shape backward, through stage 0: ops.gemm (with the hff gate) / layernorm_bwd launches on the same saved activations."""
    r = reference(37, 167, 2048, "in_proj", 0.1)
    o = run_bwd(dev, r, True)
    s = {k: T(v, dev) for k, v in r.saved.items()}
    w = {k: T(r.w[k], dev) for k in ("g1", "g2", "w1", "w2", "wo")}
    s1, _, s3 = r.seeds
    inv_keep = float(np.float32(1) / (np.float32(1) - np.float32(r.p)))
    dyout = ops.gemm(T(r.up["dqkv_up"], dev), T(r.up["win_up"], dev), residual=T(r.up["dz1_up"], dev))
    dz2, dff, _, _ = ops.layernorm_bwd(dyout, s["z2"], w["g2"], s["mean2"], s["rstd2"], r.p, s3)
    dhff = ops.gemm(dff, w["w2"], gate=s["hff"], gate_scale=inv_keep)
    dy1 = ops.gemm(dhff, w["w1"], residual=dz2)
    dz1, dsa, _, _ = ops.layernorm_bwd(dy1, s["z1"], w["g1"], s["mean1"], s["rstd1"], r.p, s1)
    dctx = ops.gemm(dsa, w["wo"])
    assert torch.equal(o["dhff"] == 0, dhff == 0) and torch.equal(o["dff"] == 0, dff == 0) and torch.equal(o["dsa"] == 0, dsa == 0)
    for n, t in (("dyout", dyout), ("dz2", dz2), ("dff", dff), ("dhff", dhff), ("dy1", dy1), ("dz1", dz1), ("dsa", dsa), ("dctx", dctx)):
        chain_close(o[n], t, f"backward {n}")


# ---- refusals through the front end -----------------------------------------------------------------------------------------------------------
def test_unsupported_widths_are_refused(dev):
    for F, DFF in ((3, 16), (193, 16), (16, 15)):
        ctx = torch.zeros(4, F, device=dev)
        w = {k: torch.zeros(s, device=dev) for k, s in ops._encoder_rows_shapes(F, DFF).items()}
        with pytest.raises(RuntimeError, match="not supported"):
            ops.encoder_rows_fwd(ctx, ctx, w)
        saved = dict(z1=ctx, z2=ctx, hff=torch.zeros(4, DFF, device=dev), mean1=ctx[:, 0], rstd1=ctx[:, 0], mean2=ctx[:, 0], rstd2=ctx[:, 0])
        with pytest.raises(RuntimeError, match="not supported"):
            ops.encoder_rows_bwd(saved, w, dyout=ctx)
    torch.cuda.synchronize()


# ---- under poison -----------------------------------------------------------------------------------------------------------------------------
class Pools:
    """Operands in moated pools with base offset 1: inputs between bands of ``fill``, outputs as NaN between NaN."""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.checks = dev, fill, []

    def put(self, a):
        v, check = moated(torch.from_numpy(np.array(a)), self.fill, offset=1, device=self.dev)
        self.checks.append(check)
        return v

    def out(self, *shape):
        v, check = moated(shape, NAN, offset=1, device=self.dev)
        self.checks.append(check)
        assert bool(v.isnan().all())
        return v

    def check(self):
        for c in self.checks:
            c()


POISON_CASE = (37, 167, 70)                    # odd F, ragged B, DFF % 4 != 0


@pytest.mark.parametrize("fill", [NAN, 0x7B], ids=["nan", "inputs-0x7b"])
def test_row_forward_under_poison(dev, monkeypatch, fill):
    """Every input and parameter in its own moated pool at an odd base, every output NaN between NaN moats, the next projection into the left
    half of a moated [B, 256] buffer: the clamped loads of rows >= B, of k >= K and of columns >= N may not reach a result, no store may
    leave an extent, and the op allocates nothing.  Second run: inputs between bands of 0x7B (see test_gemm_family_under_poison)."""
    B, F, DFF = POISON_CASE
    r = reference(B, F, DFF, "fc", 0.1)
    P = Pools(dev, fill)
    w = {k: P.put(v) for k, v in r.w.items()}
    nxt = dict(wn=P.put(r.nxt["wn"]), bn=P.put(r.nxt["bn"]), act="relu")
    wide = P.out(B, 256)
    nxt["outn"] = wide[:, :128]
    shapes = {"z1": (B, F), "y1": (B, F), "hff": (B, DFF), "z2": (B, F), "y2": (B, F), "mean1": (B,), "rstd1": (B,), "mean2": (B,), "rstd2": (B,)}
    out = {n: P.out(*s) for n, s in shapes.items()}
    with poisoned_allocations(monkeypatch, NAN) as pa:
        o = ops.encoder_rows_fwd(P.put(r.ctx), P.put(r.xin), w, p=r.p, seeds=r.seeds, nxt=nxt, out=out)
    assert len(pa.pools) == 0 and all(o[n] is out[n] for n in out)
    assert bool(wide[:, 128:].isnan().all()), "the right half of the wide buffer was written"
    check_fwd(r, o)
    P.check()


@pytest.mark.parametrize("stage0", [False, True], ids=["dyout", "stage0"])
@pytest.mark.parametrize("fill", [NAN, 0x7B], ids=["nan", "inputs-0x7b"])
def test_row_backward_under_poison(dev, monkeypatch, fill, stage0):
    B, F, DFF = POISON_CASE
    r = reference(B, F, DFF, "none", 0.1)
    P = Pools(dev, fill)
    saved = {k: P.put(v) for k, v in r.saved.items()}
    w = {k: P.put(r.w[k]) for k in ("g1", "g2", "w1", "w2", "wo")}
    shapes = {"dz2": (B, F), "dff": (B, F), "dhff": (B, DFF), "dy1": (B, F), "dz1": (B, F), "dsa": (B, F), "dctx": (B, F)}
    if stage0:
        shapes = {"dyout": (B, F), **shapes}
    out = {n: P.out(*s) for n, s in shapes.items()}
    kw = dict(up={k: P.put(v) for k, v in r.up.items()}) if stage0 else dict(dyout=P.put(r.dyout))
    with poisoned_allocations(monkeypatch, NAN) as pa:
        o = ops.encoder_rows_bwd(saved, w, p=r.p, seeds=(r.seeds[0], r.seeds[2]), out=out, **kw)
    assert len(pa.pools) == 0 and all(o[n] is out[n] for n in out)
    check_bwd(r, o, stage0)
    P.check()
