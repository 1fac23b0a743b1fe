"""GPU: every GEMM kernel family of csrc/gemm.hip under poison.  Operands, outputs and epilogue inputs sit in NaN-filled pools with padded
leading dimensions and (second run) odd bases; the split-K slab comes from a NaN-filled, guarded allocation.  A load that is not clamped and
selected, a slab entry nobody wrote or a skipped tile turns the result into NaN; a store outside the extent breaks a moat or a guard.
Shapes: ragged in M and N, and (all but the K = 96 row) a K that ends in a partial stage; each case asserts the family it is meant for."""
import functools

import pytest
import torch

from bbbp_amd import _lib, ops
from helpers import assert_close
from poison import moated, poisoned_allocations

pytestmark = pytest.mark.gpu

NAN = 0xFF
DIRECT, B3_SMALL, B3, F32_128, SHORT_K, F32_64, B3_RESIDENT = 0, 1, 2, 3, 4, 5, 6      # bbbp_gemm_kernel_form (include/bbbp_hip.h)
LAYOUTS = {"nt": (0, 1), "nn": (0, 0), "tn": (1, 0)}
ALL = [(lay, knob) for knob in (0, 1) for lay in LAYOUTS]


def _cases():
    rows = [  # what the row is for, (M, N, K, batch), [(layout, knob)], family
        ("direct-ks1", (40, 24, 33, 1), ALL, DIRECT),
        ("direct-kslices", (3, 5, 700, 1), ALL, DIRECT),
        ("direct-wave32", (1000, 1040, 16, 1), ALL, DIRECT),
        ("f32tile64-batched", (70, 40, 9, 8), ALL, F32_64),
        ("f32tile64-splitk-scalar-reduce", (33, 65, 8200, 1), ALL, F32_64),
        ("f32tile128-splitk", (130, 140, 8200, 1), [(lay, 0) for lay in LAYOUTS] + [("tn", 1)], F32_128),
        ("f32tile128-nonvector", (131, 142, 8200, 1), [("nn", 1), ("tn", 1)], F32_128),
        ("b3-splitk-tail", (130, 140, 8200, 1), [("nt", 1), ("nn", 1)], B3),
        ("b3-splitk-tail", (132, 140, 8200, 1), [("tn", 1)], B3),
        ("b3small", (500, 6100, 518, 1), [("nt", 1), ("nn", 1)], B3_SMALL),
        ("b3resident", (300, 32768, 96, 1), [("nn", 1)], B3_RESIDENT),
        ("shortk", (130, 132000, 28, 1), [("nt", 0), ("nn", 0), ("nt", 1), ("nn", 1)], SHORT_K),
        ("shortk", (384, 49152, 128, 1), [(lay, 0) for lay in LAYOUTS], SHORT_K),
    ]
    out = []
    for name, shape, combos, form in rows:
        for lay, knob in combos:
            out.append(pytest.param(shape, lay, knob, form, id=f"{name}-{'x'.join(map(str, shape))}-{lay}-knob{knob}"))
    return out


@pytest.fixture
def split_bf16_knob():
    L = _lib.lib()
    old = L.bbbp_set_gemm_split_bf16(1)
    L.bbbp_set_gemm_split_bf16(old)

    def set_(v):
        L.bbbp_set_gemm_split_bf16(v)
    yield set_
    L.bbbp_set_gemm_split_bf16(old)


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=2)
def _problem(M, N, K, batch, dev):
    """Host operands and the float64 reference of out = gate(relu(a b + bias)) + residual, on the device (the large rows compare there)."""
    lead = (batch,) if batch > 1 else ()
    a, b = _rnd(*lead, M, K, seed=M + K), _rnd(*lead, K, N, seed=N + 7)
    bias, res, gate = _rnd(N, seed=3), _rnd(*lead, M, N, seed=4), _rnd(*lead, M, N, seed=9)
    ad, bd = a.to(dev).double(), b.to(dev).double()
    want = torch.relu(ad @ bd + bias.to(dev).double()) * (gate.to(dev) > 0) + res.to(dev).double()
    scale = ad.abs() @ bd.abs() + 1.0
    return a, b, bias, res, gate, want, scale


def _pool(t, aligned, dev, fill=NAN):
    """Aligned pools: ld rounded up to a multiple of 4, plus 4, base 16-byte aligned.  Odd pools: ld = extent + 3, base offset 1."""
    shape = tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(t)
    if len(shape) != 2:                    # bias; batched operands, which the front end takes contiguous
        return moated(t, fill, offset=0 if aligned else 1, device=dev)
    ld = -(-shape[1] // 4) * 4 + 4 if aligned else shape[1] + 3
    return moated(t, fill, ld=ld, offset=0 if aligned else 1, device=dev)


@pytest.mark.parametrize("pools", ["aligned", "odd", "odd-inputs-0x7b"])
@pytest.mark.parametrize("shape,layout,knob,form", _cases())
def test_gemm_family_under_poison(dev, monkeypatch, split_bf16_knob, shape, layout, knob, form, pools):
    """``odd-inputs-0x7b``: the odd pools again with the inputs between bands of 0x7B (1.3e36) and the output between NaN.  A NaN read from
    an input's moat and stored outside the output's extent arrives with its payload intact -- 0xFFFFFFFF, the moat's own bytes -- so with
    one fill everywhere a store computed from a stray load would go unseen; a value computed from 1.3e36 does not look like the moat."""
    M, N, K, batch = shape
    ta, tb = LAYOUTS[layout]
    split_bf16_knob(knob)
    assert _lib.lib().bbbp_gemm_kernel_form(ta, tb, M, N, K, batch) == form
    a, b, bias, res, gate, want, scale = _problem(M, N, K, batch, dev)
    aligned = pools == "aligned"
    checks = []

    def put(t, fill=0x7B if pools == "odd-inputs-0x7b" else NAN):
        v, check = _pool(t, aligned, dev, fill)
        checks.append(check)
        return v
    A = put(a.transpose(-1, -2).contiguous() if ta else a)
    B = put(b.transpose(-1, -2).contiguous() if tb else b)
    C = put(tuple(want.shape), NAN)        # the output's own region starts as NaN too
    assert C.isnan().all()
    bias_d, res_d, gate_d = put(bias), put(res), put(gate)
    with poisoned_allocations(monkeypatch, NAN) as pa:
        got = ops.gemm(A, B, trans_a=bool(ta), trans_b=bool(tb), bias=bias_d, residual=res_d, act="relu", out=C, gate=gate_d)
    assert got is C
    assert len(pa.pools) == 1              # the workspace
    assert bool(C.isfinite().all()), f"{int((~C.isfinite()).sum())} of {C.numel()} output elements are not finite"
    err = (C.double() - want).abs()
    assert bool((err <= 2e-6 * scale).all()), f"max err ratio {float((err / scale).max()):.3e}"
    pa.check()
    for check in checks:
        check()


def test_batched_products_with_the_engines_strides(dev, monkeypatch):
    """Heads as column slices of one [B, 3F] buffer (lda = ldb = 3F, batch stride = head_dim): Q K^T (NT) into a strided score buffer, P V
    (NN) into the column slices of the context.  bbbp_gemm_desc directly: the torch front end only builds dense batches."""
    L = _lib.lib()
    Bn, NH, D = 70, 8, 8
    F = NH * D
    assert L.bbbp_gemm_kernel_form(0, 1, Bn, Bn, D, NH) == F32_64 and L.bbbp_gemm_kernel_form(0, 0, Bn, D, Bn, NH) == F32_64
    qkv_h = _rnd(Bn, 3 * F, seed=51)
    for aligned in (True, False):
        ldq = 3 * F + (4 if aligned else 3)
        qkv, check_qkv = moated(qkv_h, NAN, ld=ldq, offset=0 if aligned else 1, device=dev)
        lds = Bn + (2 if aligned else 3)
        scores, check_s = moated((NH * Bn, Bn), NAN, ld=lds, offset=0 if aligned else 1, device=dev)      # head h: rows h * Bn ...
        ldc = F + (4 if aligned else 3)
        ctx, check_c = moated((Bn, F), NAN, ld=ldc, offset=0 if aligned else 1, device=dev)
        q, k, v = qkv[:, :F], qkv[:, F:2 * F], qkv[:, 2 * F:]
        d1 = _lib.GemmDesc(0, 1, Bn, Bn, D, 0.25, q.data_ptr(), ldq, k.data_ptr(), ldq, scores.data_ptr(), lds, None, None, 0, 0, None, 0, 1.0,
                           NH, D, D, Bn * lds, 0, 0, 0, None, 0.0, 0)
        d2 = _lib.GemmDesc(0, 0, Bn, D, Bn, 1.0, scores.data_ptr(), lds, v.data_ptr(), ldq, ctx.data_ptr(), ldc, None, None, 0, 0, None, 0, 1.0,
                           NH, Bn * lds, D, D, 0, 0, 0, None, 0.0, 0)
        with poisoned_allocations(monkeypatch, NAN) as pa:
            wsb = max(L.bbbp_gemm_workspace_bytes(Bn, Bn, D, NH), L.bbbp_gemm_workspace_bytes(Bn, D, Bn, NH))
            ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
            arr = (_lib.GemmDesc * 2)(d1, d2)
            _lib.check(L.bbbp_gemm_f32_grouped(torch.cuda.current_stream().cuda_stream, arr, 2, ws.data_ptr(), wsb), "bbbp_gemm_f32_grouped")
        qh, kh, vh = (t.double().view(Bn, NH, D).transpose(0, 1) for t in (qkv_h[:, :F], qkv_h[:, F:2 * F], qkv_h[:, 2 * F:]))
        want_s = 0.25 * qh @ kh.transpose(1, 2)
        got_s = scores.cpu().view(NH, Bn, Bn)
        assert got_s.isfinite().all()
        assert ((got_s.double() - want_s).abs() <= 2e-6 * 0.25 * (qh.abs() @ kh.abs().transpose(1, 2)) + 1e-30).all()
        want_c = (got_s.double() @ vh).transpose(0, 1).reshape(Bn, F)                                       # of the scores the kernel read
        got_c = ctx.cpu()
        assert got_c.isfinite().all()
        assert ((got_c.double() - want_c).abs() <= 2e-6 * (got_s.double().abs() @ vh.abs()).transpose(0, 1).reshape(Bn, F) + 1e-30).all()
        pa.check(); check_qkv(); check_s(); check_c()


@pytest.mark.parametrize("pair", ["tn|nt", "nn|tn", "tn|tn"])
def test_grouped_pair_with_unequal_grids(dev, monkeypatch, pair):
    """Two small products in one launch (gemm_direct_pair_kernel): the grid covers the larger of the two in each dimension, so most
    work-groups of either problem's z range lie outside that problem's own grid and must leave its output -- and its moat -- alone."""
    L = _lib.lib()
    shapes = ((40, 700, 24), (700, 8, 24))
    lays = pair.split("|")
    for (M, N, K), lay in zip(shapes, lays):
        assert L.bbbp_gemm_kernel_form(*LAYOUTS[lay], M, N, K, 1) == DIRECT and L.bbbp_gemm_folds_asum(M, N, K, 1) == 1
        assert -(-M // 16) * -(-N // 16) <= 4096 and K <= 12 * 16           # 16 x 16 wave tiles, no K slices: four waves of one tile each
    problems, wants, checks = [], [], []
    for i, ((M, N, K), lay) in enumerate(zip(shapes, lays)):
        ta, tb = LAYOUTS[lay]
        a, b, res = _rnd(M, K, seed=60 + i), _rnd(K, N, seed=70 + i), _rnd(M, N, seed=80 + i)
        A, ca = moated(a.t().contiguous() if ta else a, NAN, ld=(M if ta else K) + 3, offset=1, device=dev)
        Bm, cb = moated(b.t().contiguous() if tb else b, NAN, ld=(K if tb else N) + 3, offset=1, device=dev)
        C, cc = moated((M, N), NAN, ld=N + 3, offset=1, device=dev)
        R, cr = moated(res, NAN, ld=N + 3, offset=1, device=dev)
        checks += [ca, cb, cc, cr]
        problems.append(dict(a=A, b=Bm, trans_a=bool(ta), trans_b=bool(tb), residual=R, out=C))
        wants.append((a.double() @ b.double() + res.double(), a.double().abs() @ b.double().abs() + 1.0))
    with poisoned_allocations(monkeypatch, NAN) as pa:
        outs = ops.gemm_grouped(problems)
    for got, (want, scale) in zip(outs, wants):
        assert got.isfinite().all()
        assert ((got.cpu().double() - want).abs() <= 2e-6 * scale).all()
    pa.check()
    for check in checks:
        check()


@pytest.mark.parametrize("M,N,K", [(37, 16, 16), (37, 5, 5), (700, 16, 24)])
def test_bias_gradient_column_of_the_weight_gradient(dev, monkeypatch, M, N, K):
    """linear_weight_bias_grad: db rides as a virtual all-ones column at index K of x (bbbp_gemm_desc.asum) -- at K = 16 that column opens
    a wave tile of its own, at K = 5 it shares one; dW and db come from guarded NaN allocations, dy and x sit in padded NaN pools."""
    assert _lib.lib().bbbp_gemm_folds_asum(N, K, M, 1) == 1
    dy_h, x_h = _rnd(M, N, seed=M + N), _rnd(M, K, seed=M + K + 1)
    for aligned in (True, False):
        dy, c1 = _pool(dy_h, aligned, dev)
        x, c2 = _pool(x_h, aligned, dev)
        with poisoned_allocations(monkeypatch, NAN) as pa:
            dw, db = ops.linear_weight_bias_grad(dy, x)
        assert len(pa.pools) == 3 and dw.isfinite().all() and db.isfinite().all()
        assert_close(dw.cpu().numpy(), (dy_h.double().t() @ x_h.double()).numpy(), rtol=1e-5, atol_frac=2e-6, what="dW")
        assert_close(db.cpu().numpy(), dy_h.double().sum(dim=0).numpy(), rtol=1e-5, atol_frac=2e-6, what="db")
        pa.check(); c1(); c2()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("M,N,K", [(37, 64, 300), (5, 256, 16), (16, 1, 7)])
def test_linear_layernorm_with_padded_leading_dimensions(dev, monkeypatch, M, N, K):
    """bbbp_linear_layernorm_fwd at the C ABI with ld > extent on x, residual, z and y.  Tolerances: those of
    test_linear_layernorm_fused_matches_gemm_then_layernorm (against the two-launch schedule, and y against float64)."""
    x_h, w_h, b_h = _rnd(M, K, seed=31), _rnd(N, K, seed=32) * 0.2, _rnd(N, seed=33)
    res_h, gam_h, bet_h = _rnd(M, N, seed=34), 1 + 0.1 * _rnd(N, seed=35), _rnd(N, seed=36)
    y0, z0, m0, r0 = ops.layernorm_fwd(ops.gemm(x_h.to(dev), w_h.to(dev), trans_b=True, bias=b_h.to(dev)), res_h.to(dev), gam_h.to(dev), bet_h.to(dev))
    zz = x_h.double() @ w_h.double().t() + b_h.double() + res_h.double()
    want = torch.nn.functional.layer_norm(zz, (N,), gam_h.double(), bet_h.double(), 1e-5)
    for aligned in (True, False):
        checks = []

        def put(t):
            v, check = _pool(t, aligned, dev)
            checks.append(check)
            return v
        x, w, b, res, gam, bet = (put(t) for t in (x_h, w_h.reshape(-1), b_h, res_h, gam_h, bet_h))      # the weight is dense: ld = K
        z, y, mean, rstd = put((M, N)), put((M, N)), put((M,)), put((M,))
        _lib.check(_lib.lib().bbbp_linear_layernorm_fwd(_stream(), x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), res.data_ptr(), res.stride(0),
                                                        z.data_ptr(), z.stride(0), y.data_ptr(), y.stride(0), gam.data_ptr(), bet.data_ptr(),
                                                        mean.data_ptr(), rstd.data_ptr(), M, N, K, 1e-5, 0.0, 0), "bbbp_linear_layernorm_fwd")
        for t in (z, y, mean, rstd):
            assert t.isfinite().all()
        assert_close(z.cpu().numpy(), z0.cpu().numpy(), rtol=2e-5, atol_frac=2e-6, what="z")
        assert_close(y.cpu().numpy(), y0.cpu().numpy(), rtol=1e-4, atol_frac=1e-5, what="y")
        assert_close(mean.cpu().numpy(), m0.cpu().numpy(), rtol=1e-4, atol_frac=1e-5, what="mean")
        assert_close(rstd.cpu().numpy(), r0.cpu().numpy(), rtol=1e-4, atol_frac=1e-6, what="rstd")
        assert_close(y.cpu().numpy(), want.numpy(), rtol=1e-4, atol_frac=1e-5, what="y vs float64")
        for check in checks:
            check()


@pytest.mark.parametrize("M,N,K", [(37, 128, 167), (33, 17, 192), (3, 5, 7)])
def test_layernorm_linear_with_padded_leading_dimensions(dev, monkeypatch, M, N, K):
    """bbbp_layernorm_linear_fwd at the C ABI with ld > extent on z, y and out.  Tolerances: those of
    test_layernorm_absorbed_by_the_consuming_linear (y, mean, rstd against the row kernel, out against the float64 composition)."""
    z_h = _rnd(M, K, seed=41)
    z_h[: max(1, M // 3)] += 30.0
    gam_h, bet_h = 1 + 0.2 * _rnd(K, seed=42), 0.3 * _rnd(K, seed=43)
    w_h, b_h = _rnd(N, K, seed=44) * 0.2, _rnd(N, seed=45)
    y0, _, m0, r0 = ops.layernorm_fwd(z_h.to(dev), None, gam_h.to(dev), bet_h.to(dev))
    want_y = torch.nn.functional.layer_norm(z_h.double(), (K,), gam_h.double(), bet_h.double(), 1e-5)
    want = torch.relu(want_y @ w_h.double().t() + b_h.double())
    for aligned in (True, False):
        checks = []

        def put(t):
            v, check = _pool(t, aligned, dev)
            checks.append(check)
            return v
        z, gam, bet, w, b = (put(t) for t in (z_h, gam_h, bet_h, w_h.reshape(-1), b_h))
        out, y, mean, rstd = put((M, N)), put((M, K)), put((M,)), put((M,))
        _lib.check(_lib.lib().bbbp_layernorm_linear_fwd(_stream(), z.data_ptr(), z.stride(0), gam.data_ptr(), bet.data_ptr(), 1e-5, w.data_ptr(),
                                                        b.data_ptr(), out.data_ptr(), out.stride(0), 1, 0.0, 0, y.data_ptr(), y.stride(0),
                                                        mean.data_ptr(), rstd.data_ptr(), M, N, K), "bbbp_layernorm_linear_fwd")
        for t in (out, y, mean, rstd):
            assert t.isfinite().all()
        assert_close(mean.cpu().numpy(), m0.cpu().numpy(), rtol=1e-6, atol_frac=1e-7, what="mean")
        assert_close(rstd.cpu().numpy(), r0.cpu().numpy(), rtol=2e-6, atol_frac=1e-7, what="rstd")
        assert_close(y.cpu().numpy(), y0.cpu().numpy(), rtol=1e-5, atol_frac=2e-6, what="y")
        assert_close(out.cpu().numpy(), want.numpy(), rtol=2e-4, atol_frac=2e-5, what="out vs float64")
        for check in checks:
            check()


def test_the_detectors_see_a_wider_product_on_the_device(dev, monkeypatch):
    """The same checks must fail when the kernel really touches what it does not own -- here because the caller describes a product one
    column wider (the store lands in C's moat) or one k deeper (the loads reach the operands' moats) than the buffers hold.  The inputs'
    moats are 0x7B: see test_gemm_family_under_poison for what a NaN moat on both sides cannot show."""
    M, N, K = 40, 24, 33
    a, b = _rnd(M, K, seed=1), _rnd(K, N, seed=2)
    A, _ = moated(a, 0x7B, ld=K + 3, offset=1, device=dev)
    B, _ = moated(b, 0x7B, ld=N + 3, offset=1, device=dev)
    C, check_c = moated((M, N), NAN, ld=N + 3, offset=1, device=dev)
    wide = B.as_strided((K, N + 1), (N + 3, 1), B.storage_offset())
    ops.gemm(A, wide, out=C.as_strided((M, N + 1), (N + 3, 1), C.storage_offset()))
    assert C.isfinite().all()
    with pytest.raises(AssertionError, match=f"row 0 \\+ {N}"):
        check_c()
    deep = A.as_strided((M, K + 1), (K + 3, 1), A.storage_offset())
    Bt, _ = moated(b.t().contiguous(), 0x7B, ld=K + 3, offset=1, device=dev)
    got = ops.gemm(deep, Bt.as_strided((N, K + 1), (K + 3, 1), Bt.storage_offset()), trans_b=True)
    assert not got.isfinite().any()                                          # 1.3e36 squared
    with poisoned_allocations(monkeypatch, NAN) as pa:
        out = ops.gemm(A, B)
    out.as_strided((1,), (1,), out.storage_offset() + M * N)[0] = 0.0        # what a store one element past the last row leaves behind
    with pytest.raises(AssertionError, match="behind"):
        pa.check()
