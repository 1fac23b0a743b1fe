"""GPU: every conv stage in every kernel form (tests/conv_cells.py: the table of csrc/conv.hip's conv_choice) against the float64 oracle of
tests/conv_oracle.py, element by element: |got - want| <= C * scale + 1e-30 with scale the same computation on absolute values.

Every case sets the mask and the two preferences, asserts through bbbp_conv_kernel_form that the call will run the form the case is named
for, runs, restores, and only then compares.  The gradients are fed float64's own pooling decisions, so they do not depend on the forward
under test; the forward's own decisions may differ from float64's only at near-ties (conv_oracle.Problem.check_decisions), and its values
are compared under the decisions it took.  Each line ``conv-ratio ...`` printed (-s) is the worst |error| / scale of one result."""
import functools

import pytest
import torch

from bbbp_amd import _lib, ops
import conv_cells as cc
import conv_oracle as co

pytestmark = pytest.mark.gpu

def _c(cell, kind):
    """The constant of the bound: conv_oracle.C but for the cases listed, with their reason, in conv_oracle.C_MOVED."""
    return co.C_MOVED.get((cc.FORM_NAMES[cell.form], cc.OP_NAMES[cell.op], cell.stage, kind), co.C)


def _cases(op, flat=False):
    """(cell, B, kind) of one op, problems of one (stage, kind, B) next to each other so that the oracle cache serves them."""
    out = []
    for c in cc.cells(op):
        rows = [(1, "plain"), (c.big, "plain")] + ([(2, "wide")] if cc.wants_wide(c) else [])
        if flat:
            rows = [(2, "flat")] if c.stage.startswith("W") else []
        out += [(c, B, kind) for B, kind in rows]
    out.sort(key=lambda r: (r[0].stage, r[2], r[1]))
    return [pytest.param(*r, id=f"{cc.cell_id(r[0])}-B{r[1]}-{r[2]}") for r in out]


def _purpose(dev, cell, B, kind):
    """The larger plain batch is there for a ragged share of work items per work-group: check it against this device's CU count."""
    if kind != "plain" or B == 1:
        return
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    nwork, grid = cc.geometry(cell, B, cus)
    if (cell.op, cell.stage) == (cc.WGRAD, "W3"):
        return                                           # 16 B strips over 16 groups: never ragged
    if B == cc.CAP:
        assert nwork > grid                              # ragged only beyond the cap: more than one item per group is what is left
    elif not cc.ragged(cell, B, cus):
        pytest.skip(f"{cc.cell_id(cell)}: B = {B} gives {nwork} work items over {grid} work-groups on {cus} CUs, not the ragged share it was chosen for on 256")


def _dev(dev, *ts):
    return [t.to(dev) for t in ts]


def _compare(cell, B, kind, results, c=None):
    """results: {name: (got, want, scale)}.  Prints every ratio, then asserts every bound."""
    c = _c(cell, kind) if c is None else c
    out = {name: co.within(got, want, scale, c) for name, (got, want, scale) in results.items()}
    print(f"conv-ratio {cc.cell_id(cell)} B={B} {kind} " + " ".join(f"{n}={r:.3e}" for n, (_, r) in out.items()))
    for name, (ok, r) in out.items():
        assert ok, f"{cc.cell_id(cell)} B={B} {kind}: {name} off by {r:.3e} x scale (bound {c:.1e})"


def _forward(dev, cell, B, kind):
    p = co.problem(cell.stage, B, kind)
    x, w, b = _dev(dev, p.x, p.w, p.b)
    with cc.selected(_lib.lib(), cell):
        y, m = ops.conv3x3_relu_pool_fwd(x, w, b)
        y1, m1 = ops.conv3x3_relu_pool_fwd(x, w, b, keep_mask=False)
    assert m1 is None and torch.equal(y, y1)             # the forward-only call: the same bits
    m = m.cpu()
    share = p.check_decisions(m, cc.cell_id(cell))
    want, scale = p.forward(m)
    print(f"conv-decisions {cc.cell_id(cell)} B={B} {kind} differ at {share:.2e}")
    _compare(cell, B, kind, {"y": (y, want, scale)})
    assert not bool(y.cpu()[m == 4].any())               # ReLU inactive: exactly zero
    return p, m


@pytest.mark.parametrize("cell,B,kind", _cases(cc.FWD))
def test_forward(dev, cell, B, kind):
    _purpose(dev, cell, B, kind)
    _forward(dev, cell, B, kind)


@pytest.mark.parametrize("cell,B,kind", _cases(cc.FWD, flat=True))
def test_forward_flat_images(dev, cell, B, kind):
    """An image with a flat band across the left and right borders and an all-ones image: inside the flat region the four pre-activations
    of a window come from identical inputs, so the first-maximum rule leaves 0, or 4 where the value is not positive."""
    p, m = _forward(dev, cell, B, kind)
    _, rows = co.flat_rows(p.hw)
    assert set(m[0, :, rows, 1:-1].unique().tolist()) <= {0, 4}
    assert set(m[1:, :, 1:-1, 1:-1].unique().tolist()) <= {0, 4}


def _data_gradient(dev, cell, B, kind, mask, ref):
    p = co.problem(cell.stage, B, kind)
    gy, w, m = _dev(dev, p.gy, p.w, mask)
    with cc.selected(_lib.lib(), cell):
        dx = ops.conv3x3_relu_pool_bwd_data(gy, m, w)
    return {"dx": (dx, *ref["dx"])}


def _weight_gradient(dev, cell, B, kind, mask, ref):
    p = co.problem(cell.stage, B, kind)
    x, gy, m = _dev(dev, p.x, p.gy, mask)
    with cc.selected(_lib.lib(), cell):
        dw, db = ops.conv3x3_relu_pool_bwd_weight(x, gy, m)
    return {"dw": (dw, *ref["dw"]), "db": (db, *ref["db"])}


@pytest.mark.parametrize("cell,B,kind", _cases(cc.DGRAD))
def test_data_gradient(dev, cell, B, kind):
    _purpose(dev, cell, B, kind)
    p = co.problem(cell.stage, B, kind)
    _compare(cell, B, kind, _data_gradient(dev, cell, B, kind, p.decisions, p.backward()))


@pytest.mark.parametrize("cell,B,kind", _cases(cc.WGRAD))
def test_weight_gradient(dev, cell, B, kind):
    """B = 1 on W3 leaves the structured-sparse kernels 8 stages for 16 groups: half the groups write an all-zero slab, and it is summed."""
    _purpose(dev, cell, B, kind)
    p = co.problem(cell.stage, B, kind)
    _compare(cell, B, kind, _weight_gradient(dev, cell, B, kind, p.decisions, p.backward()))


@functools.lru_cache(maxsize=2)
def _synthetic(stage, name):
    p = co.problem(stage, 2, "plain")
    m = co.synthetic_mask(name, tuple(p.gy.shape))
    return m, p.backward(m)


def _synthetic_cases(op):
    rows = sorted(((c, name) for c in cc.cells(op) for name in co.SYNTHETIC), key=lambda r: (r[0].stage, r[1]))
    return [pytest.param(c, name, id=f"{cc.cell_id(c)}-{name}") for c, name in rows]


@pytest.mark.parametrize("cell,name", _synthetic_cases(cc.DGRAD))
def test_data_gradient_synthetic_masks(dev, cell, name):
    """Masks no forward produces: a random forward gives 0..3 about evenly and almost no 4."""
    m, ref = _synthetic(cell.stage, name)
    res = _data_gradient(dev, cell, 2, "plain", m, ref)
    _compare(cell, 2, name, res, _c(cell, "plain"))
    if name == "const4":
        assert not bool(res["dx"][0].any())


@pytest.mark.parametrize("cell,name", _synthetic_cases(cc.WGRAD))
def test_weight_gradient_synthetic_masks(dev, cell, name):
    """The structured-sparse forms build their 2:4 index from the mask: constant positions, and 4 everywhere (no nonzero at all)."""
    m, ref = _synthetic(cell.stage, name)
    res = _weight_gradient(dev, cell, 2, "plain", m, ref)
    _compare(cell, 2, name, res, _c(cell, "plain"))
    if name == "const4":
        assert not bool(res["dw"][0].any()) and not bool(res["db"][0].any())


# ---- the C ABI directly -------------------------------------------------------------------------------------------------------------

SENTINEL = -7.25


def _abi(dev, stage, B):
    """Device buffers of one stage, the outputs filled with a sentinel, and the full workspace; B = 0 gets one image's worth of memory."""
    cin, cout, hw = co.STAGES[stage]
    n = max(B, 1)
    f = lambda *s: torch.randn(*s, device=dev)
    t = dict(x=f(n, cin, hw, hw), w=f(cout, cin, 3, 3) * 0.2, b=f(cout) * 0.1, gy=f(n, cout, hw // 2, hw // 2),
             m=torch.randint(0, 5, (n, cout, hw // 2, hw // 2), device=dev, dtype=torch.uint8),
             y=torch.full((n, cout, hw // 2, hw // 2), SENTINEL, device=dev), ym=torch.full((n, cout, hw // 2, hw // 2), 9, device=dev, dtype=torch.uint8),
             dx=torch.full((n, cin, hw, hw), SENTINEL, device=dev), dw=torch.full((cout, cin, 3, 3), SENTINEL, device=dev),
             db=torch.full((cout,), SENTINEL, device=dev))
    wsb = _lib.lib().bbbp_conv3x3_workspace_bytes(B, cin, cout, hw, hw)
    t["ws"] = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    return t, wsb


def _call(op, stage, B, t, wsb, null=None):
    """One entry point on the current stream; ``null`` names the argument passed as a null pointer."""
    L = _lib.lib()
    cin, cout, hw = co.STAGES[stage]
    st = torch.cuda.current_stream().cuda_stream
    a = {k: (None if k == null else v.data_ptr()) for k, v in t.items()}
    if op == cc.FWD:
        return L.bbbp_conv3x3_relu_pool_fwd(st, a["x"], a["w"], a["b"], a["y"], a["ym"], B, cin, cout, hw, hw, a["ws"], wsb)
    if op == cc.DGRAD:
        return L.bbbp_conv3x3_relu_pool_bwd_data(st, a["gy"], a["m"], a["w"], a["dx"], B, cin, cout, hw, hw, a["ws"], wsb)
    return L.bbbp_conv3x3_relu_pool_bwd_weight(st, a["x"], a["gy"], a["m"], a["dw"], a["db"], B, cin, cout, hw, hw, a["ws"], wsb)


OUTPUTS = {cc.FWD: ("y", "ym"), cc.DGRAD: ("dx",), cc.WGRAD: ("dw", "db")}
INPUTS = {cc.FWD: ("x", "w", "b", "y", "ws"), cc.DGRAD: ("gy", "m", "w", "dx", "ws"), cc.WGRAD: ("x", "gy", "m", "dw", "db", "ws")}


def _untouched(t, op):
    torch.cuda.synchronize()
    return all(bool((t[k] == (9 if k == "ym" else SENTINEL)).all()) for k in OUTPUTS[op])


def _ops_of(stage):
    return [op for op in (cc.FWD, cc.DGRAD, cc.WGRAD) if (op, stage) not in cc.UNSUPPORTED]


@pytest.mark.parametrize("stage", list(co.STAGES))
def test_abi_empty_batch(dev, stage):
    """B = 0: OK from all three ops, nothing written to y / mask / dx, dw and db zero-filled."""
    t, wsb = _abi(dev, stage, 0)
    for op in _ops_of(stage):
        assert _call(op, stage, 0, t, wsb) == 0, _lib.lib().bbbp_last_error()
        if op != cc.WGRAD:
            assert _untouched(t, op)
    torch.cuda.synchronize()
    assert not bool(t["dw"].any()) and not bool(t["db"].any())


@pytest.mark.parametrize("stage", list(co.STAGES))
def test_abi_null_pointer(dev, stage):
    """Every required pointer, one at a time (the forward's mask alone may be null): an error, a message, and nothing launched."""
    L = _lib.lib()
    t, wsb = _abi(dev, stage, 1)
    for op in _ops_of(stage):
        for name in INPUTS[op]:
            assert _call(op, stage, 1, t, wsb, null=name) != 0, (op, name)
            assert b"null pointer" in L.bbbp_last_error()
            assert _untouched(t, op), (op, name)


def _need(op, stage, B, cus):
    """Bytes of workspace the f32 form of the op takes (csrc/conv.hip): the re-laid filters [9][cin, 3 padded to 4][cout] of the forward and
    the data gradient; one slab [64][288] + [64] (3-channel stages: [32][32] + [32]) per work-group of the weight gradient's grid."""
    cin, cout, hw = co.STAGES[stage]
    if op != cc.WGRAD:
        return 9 * max(cin, 4) * cout * 4
    _, groups = cc.geometry(cc.Cell(op, stage, 0, 0, 0, cc.F32, 0), B, cus)
    return groups * (cout // 32) * (1024 + 32) * 4 if cin == 3 else groups * (cin // 32) * (cout // 64) * (64 * 288 + 64) * 4


@pytest.mark.parametrize("stage,B", [("S1", 8), ("S2", 1), ("W3", 1)])
def test_abi_short_workspace(dev, stage, B):
    """One byte less than the op needs: rejected by the argument check in conv.hip with a message, before anything is launched -- the
    buffer behind the pointer is the full bbbp_conv3x3_workspace_bytes all the same.  That size is the stage's maximum over the three ops
    and over any weight-gradient grid (512 slabs), and each entry point checks its own share of it (the engine hands all of them one
    scratch area): the filters of the forward and the data gradient, the slabs of this call's grid.  So the byte an op misses is the last
    byte of ITS share -- which is the whole size for the weight gradient of S1 from B = 8 on 256 CUs (512 work-groups; asserted where it
    applies).  With exactly its share the op runs and gives the bits of the plain call."""
    L = _lib.lib()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    old = L.bbbp_get_conv_winograd()
    L.bbbp_set_conv_winograd(0)
    try:
        t, wsb = _abi(dev, stage, B)
        for op in _ops_of(stage):
            assert L.bbbp_conv_kernel_form(op, *co.STAGES[stage]) == cc.F32
            need = _need(op, stage, B, cus)
            assert need <= wsb
            if op == cc.WGRAD and stage == "S1" and cus * 2 >= 512:
                assert need == wsb                       # one byte short of bbbp_conv3x3_workspace_bytes itself
            assert _call(op, stage, B, t, need - 1) != 0
            assert b"workspace" in L.bbbp_last_error()
            assert _untouched(t, op)
            assert _call(op, stage, B, t, need) == 0, L.bbbp_last_error()
            torch.cuda.synchronize()
            exact = [t[k].clone() for k in OUTPUTS[op]]
            assert _call(op, stage, B, t, wsb) == 0, L.bbbp_last_error()
            torch.cuda.synchronize()
            assert all(torch.equal(e, t[k]) for e, k in zip(exact, OUTPUTS[op]))
    finally:
        L.bbbp_set_conv_winograd(old)


# ---- the front end's checks (ops.py) ------------------------------------------------------------------------------------------------
# Every wrong operand is LARGER than the right one (one more image, one more channel; the strided ones are slices of a larger buffer), so a
# call that slipped past a missing check would still read only memory it was given.

def _front_end(dev):
    cin, cout, hw = co.STAGES["S2"]
    B = 2
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, device=dev, dtype=dtype)
    return dict(B=B, cin=cin, cout=cout, hw=hw, z=z, x=z(B, cin, hw, hw), w=z(cout, cin, 3, 3), gy=z(B, cout, hw // 2, hw // 2),
                m=z(B, cout, hw // 2, hw // 2, dtype=torch.uint8))


def _raises(fn, *shapes):
    with pytest.raises(RuntimeError) as e:
        fn()
    for s in shapes:
        assert str(tuple(s)) in str(e.value), (str(e.value), tuple(s))


def test_bwd_weight_rejects_mismatched_operands(dev):
    f = _front_end(dev)
    B, cin, cout, hw, z, x, gy, m = (f[k] for k in ("B", "cin", "cout", "hw", "z", "x", "gy", "m"))
    bw = ops.conv3x3_relu_pool_bwd_weight
    dw, db = bw(x, gy, m)                                                            # the right operands pass
    assert tuple(dw.shape) == (cout, cin, 3, 3) and tuple(db.shape) == (cout,)
    xs = z(B, cin + 1, hw, hw)[:, :cin]                                              # a channel slice: right shape, wrong strides
    assert tuple(xs.shape) == tuple(x.shape) and not xs.is_contiguous()
    _raises(lambda: bw(xs, gy, m), xs.shape)
    ms = z(B, cout + 1, hw // 2, hw // 2, dtype=torch.uint8)[:, :cout]
    _raises(lambda: bw(x, gy, ms), ms.shape)
    m1 = z(B + 1, cout, hw // 2, hw // 2, dtype=torch.uint8)                         # one more image of decisions than of gradients
    _raises(lambda: bw(x, gy, m1), m1.shape, gy.shape)
    gy1 = z(B + 1, cout, hw // 2, hw // 2)                                           # gy and mask agree, x has one image fewer
    _raises(lambda: bw(x, gy1, m1), gy1.shape, x.shape)
    gy2, m2 = z(B, cout, hw // 2 + 1, hw // 2), z(B, cout, hw // 2 + 1, hw // 2, dtype=torch.uint8)      # one more pooled row
    _raises(lambda: bw(x, gy2, m2), gy2.shape, x.shape)
    xo = z(B, cin, hw + 1, hw)                                                       # odd height
    _raises(lambda: bw(xo, gy, m), xo.shape)
    xo = z(B, cin, hw, hw + 1)                                                       # odd width
    _raises(lambda: bw(xo, gy, m), xo.shape)
    bw(x, gy.transpose(2, 3), m)                                                     # gy keeps its .contiguous()


def test_bwd_data_rejects_mismatched_operands(dev):
    f = _front_end(dev)
    B, cin, cout, hw, z, w, gy, m = (f[k] for k in ("B", "cin", "cout", "hw", "z", "w", "gy", "m"))
    bd = ops.conv3x3_relu_pool_bwd_data
    assert tuple(bd(gy, m, w).shape) == (B, cin, hw, hw)
    ms = z(B, cout + 1, hw // 2, hw // 2, dtype=torch.uint8)[:, :cout]
    _raises(lambda: bd(gy, ms, w), ms.shape)
    ws = z(cout, cin + 1, 3, 3)[:, :cin]
    assert tuple(ws.shape) == tuple(w.shape) and not ws.is_contiguous()
    _raises(lambda: bd(gy, m, ws), ws.shape)
    m1 = z(B + 1, cout, hw // 2, hw // 2, dtype=torch.uint8)
    _raises(lambda: bd(gy, m1, w), m1.shape, gy.shape)
    w1 = z(cout + 1, cin, 3, 3)                                                      # one more output channel than gy has
    _raises(lambda: bd(gy, m, w1), w1.shape, gy.shape)
    w2 = z(cout, cin, 3, 4)
    _raises(lambda: bd(gy, m, w2), w2.shape)
    bd(gy.transpose(2, 3), m, w)
