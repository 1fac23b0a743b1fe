"""The detectors of tests/poison.py detect: "kernels" written in torch on CPU tensors, each in a correct form and with one planted fault
of the kind a ragged-tile clamp, a K-tail path or a vector epilogue gets wrong.  (The device condition of ``poisoned_allocations`` is lifted
by its ``cuda_only`` parameter; everything else is the code the GPU tests run.)"""
import pytest
import torch

from poison import FILLS, GUARD, fill_value, moated, poisoned_allocations

M, N, K = 40, 37, 21


def _operands():
    g = torch.Generator().manual_seed(5)
    return torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)


def _raw(view, rows, cols):
    """What a kernel holds: a base pointer and a leading dimension -- nothing stops it at the extent."""
    return view.as_strided((rows, cols), (view.stride(0), 1), view.storage_offset())


STRAY = 1.2345      # 0x3F9E0419: no byte of it equals a fill byte, so a stray store of it is visible under every fill


def fake_gemm(a, b, out=None, *, fault=None):
    """out = a @ b computed tile by tile (16 x 16) into a ``torch.empty`` output, the way the library's wrappers allocate."""
    m, k = a.shape
    n = b.shape[1]
    if out is None:
        out = torch.empty(m, n, dtype=a.dtype, device=a.device)
    a_used = _raw(a, m, k + 1) if fault == "reads K" else a          # one element past the K tail of every row of A ...
    b_used = torch.cat([b, torch.ones(1, n, dtype=b.dtype)]) if fault == "reads K" else b      # ... meets a nonzero partner
    for i in range(0, m, 16):
        for j in range(0, n, 16):
            if fault == "skips a tile" and (i, j) == (16, 32):
                continue
            out[i:i + 16, j:j + 16] = a_used[i:i + 16] @ b_used[:, j:j + 16]
    if fault == "past the last row":
        out.as_strided((1,), (1,), out.storage_offset() + (m - 1) * out.stride(0) + n)[0] = STRAY
    if fault == "past N":
        _raw(out, m, n + 1)[3, n] = STRAY
    return out


def test_passes_through_on_the_cpu_and_restores(monkeypatch):
    real_empty, real_like = torch.empty, torch.empty_like
    with poisoned_allocations(monkeypatch, 0xFF) as pa:
        assert torch.empty is not real_empty
        t = torch.empty(3, 4)
        u = torch.empty_like(t)
    assert torch.empty is real_empty and torch.empty_like is real_like
    assert pa.pools == [] and t.shape == (3, 4) and u.shape == (3, 4)
    assert pa.check() == 0


@pytest.mark.parametrize("fill", FILLS)
def test_allocations_are_poisoned_aligned_and_behave_like_tensors(monkeypatch, fill):
    with poisoned_allocations(monkeypatch, fill, cuda_only=False) as pa:
        x = torch.empty(5, 7)
        y = torch.empty((2, 3, 4), dtype=torch.float64)
        u = torch.empty(torch.Size([9]), dtype=torch.uint8)
        z = torch.empty(0, 6)
        c = torch.empty(3, dtype=torch.int32)
        like = torch.empty_like(x[:, :3])                      # a strided input: the real function returns a contiguous tensor
        as64 = torch.empty_like(x, dtype=torch.float64)
        perm = torch.empty_like(y.permute(2, 0, 1))            # dense and permuted: strides preserved, served by the real function
        kept = torch.empty(4, 4, pin_memory=False)             # an argument the pools do not model: the real function
        flat = torch.empty(1003)
    assert len(pa.pools) == 8
    assert perm.stride() == y.permute(2, 0, 1).stride() and kept.shape == (4, 4)
    for t in (x, y, u, z, c, like, as64, flat):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        assert t.numel() == 0 or torch.equal(t.view(-1).view(torch.uint8), torch.full((t.numel() * t.dtype.itemsize,), fill, dtype=torch.uint8))
    assert like.shape == (5, 3) and as64.dtype == torch.float64 and z.shape == (0, 6)
    if fill == 0xFF:
        assert x.isnan().all() and y.isnan().all() and int(u[0]) == 255 and int(c[0]) == -1
    if fill == 0x7B:
        assert float(x[0, 0]) > 1e36 and int(u[0]) == 123
    # split, view, slices and in-place arithmetic are those of any tensor
    parts = flat.split([5, 1, 167, 830])
    assert [p.numel() for p in parts] == [5, 1, 167, 830] and parts[2].data_ptr() == flat.data_ptr() + 24
    x.zero_(); x.view(35)[34] = 2.0
    assert float(x.sum()) == 2.0 and float(x[4, 6]) == 2.0
    y.copy_(torch.ones(2, 3, 4, dtype=torch.float64)); u.fill_(7); c.fill_(1); like.zero_(); as64.zero_(); flat.zero_()
    assert pa.check() == 8                                      # every element written, no guard touched
    pa.release()
    assert pa.check() == 0


def test_requires_grad_allocations_are_leaves(monkeypatch):
    with poisoned_allocations(monkeypatch, 0x00, cuda_only=False) as pa:
        w = torch.empty(3, 3, requires_grad=True)
    assert w.is_leaf and w.requires_grad
    (w * 2).sum().backward()
    assert torch.equal(w.grad, torch.full((3, 3), 2.0))
    pa.check()


@pytest.mark.parametrize("where", ["behind", "before"])
def test_guard_check_names_the_allocation(monkeypatch, where):
    with poisoned_allocations(monkeypatch, 0xFF, cuda_only=False) as pa:
        torch.empty(8)
        t = torch.empty(6, 5, dtype=torch.float64)
    off = t.storage_offset() + (30 if where == "behind" else -1)
    t.as_strided((1,), (1,), off)[0] = 0.0
    with pytest.raises(AssertionError, match=r"shape \(6, 5\) dtype torch.float64"):
        pa.check()


def test_a_guard_byte_equal_to_all_but_one_bit_is_seen(monkeypatch):
    with poisoned_allocations(monkeypatch, 0x7B, cuda_only=False) as pa:
        t = torch.empty(4, dtype=torch.uint8)
    pool = pa.pools[0][0]
    pool[GUARD + 4 + GUARD - 1] = 0x7A                          # the very last guard byte, one bit off
    with pytest.raises(AssertionError, match="behind"):
        pa.check()
    assert t.numel() == 4


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("ld,offset", [(None, 0), (N + 7, 0), (N + 3, 1)])
def test_moated_views_hold_the_operand_and_nothing_else(fill, ld, offset):
    src = torch.arange(M * N, dtype=torch.float32).view(M, N)
    v, check = moated(src, fill, ld=ld, offset=offset)
    assert torch.equal(v, src) and v.stride() == (ld or N, 1)
    assert v.storage_offset() * 4 % 256 == 4 * offset
    check()
    v.mul_(2.0)                                                 # the operand itself may change
    check()
    out, check_out = moated((M, N), fill, ld=ld, offset=offset)
    assert torch.equal(out.contiguous().view(-1).view(torch.uint8), torch.full((M * N * 4,), fill, dtype=torch.uint8))
    check_out()


def test_moated_n_d_u8_and_empty():
    src = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).view(2, 3, 4, 5)
    v, check = moated(src, 0xFF, offset=4)
    assert torch.equal(v, src) and v.is_contiguous()
    check()
    m, check_m = moated(torch.arange(24, dtype=torch.uint8).view(2, 12), 0x7B, ld=16)
    assert int(m[1, 11]) == 23
    check_m()
    _raw(m, 2, 13)[0, 12] = 0
    with pytest.raises(AssertionError, match="row 0 \\+ 12"):
        check_m()
    e, check_e = moated(torch.zeros(0, 6), 0xFF)
    assert e.shape == (0, 6)
    check_e()
    one, check_one = moated(torch.ones(7), 0xFF, offset=1)
    one.as_strided((1,), (1,), one.storage_offset() - 1)[0] = 1.0
    with pytest.raises(AssertionError, match="before"):
        check_one()


def _run(monkeypatch, fill, fault, ld_pad=3, offset=1):
    """One call of the fake kernel the way the GPU tests call a real one: operands and output moated, allocations poisoned."""
    a, b = _operands()
    av, check_a = moated(a, fill, ld=K + ld_pad, offset=offset)
    bv, check_b = moated(b, fill, ld=N + ld_pad, offset=offset)
    cv, check_c = moated((M, N), fill, ld=N + ld_pad, offset=offset)
    with poisoned_allocations(monkeypatch, fill, cuda_only=False) as pa:
        fresh = fake_gemm(av, bv, fault=fault)                  # output from torch.empty
        into = fake_gemm(av, bv, out=cv, fault=fault)           # output in the caller's padded buffer
    return fresh, into, pa, (check_a, check_b, check_c)


@pytest.mark.parametrize("fill", FILLS)
def test_correct_kernel_passes_every_check(monkeypatch, fill):
    a, b = _operands()
    fresh, into, pa, moats = _run(monkeypatch, fill, None)
    want = a.double() @ b.double()
    for got in (fresh, into):
        assert got.isfinite().all()
        assert ((got.double() - want).abs() <= 2e-6 * (a.abs().double() @ b.abs().double())).all()
    pa.check()
    for check in moats:
        check()
    zero = _run(monkeypatch, 0x00, None)
    assert torch.equal(fresh, zero[0]) and torch.equal(into, zero[1])      # bit-identical across fills


@pytest.mark.parametrize("fill", FILLS)
def test_write_past_the_last_row_is_caught_by_the_guard_check(monkeypatch, fill):
    fresh, into, pa, moats = _run(monkeypatch, fill, "past the last row")
    with pytest.raises(AssertionError, match=rf"shape \({M}, {N}\) dtype torch.float32.*\+0 \(behind\)"):
        pa.check()
    with pytest.raises(AssertionError, match=f"row {M - 1} \\+ {N}"):       # ... and by the moat of the caller's buffer
        moats[2]()
    moats[0](); moats[1]()


@pytest.mark.parametrize("fill", FILLS)
def test_write_past_n_inside_a_padded_row_is_caught_by_the_moat_check(monkeypatch, fill):
    fresh, into, pa, moats = _run(monkeypatch, fill, "past N")
    with pytest.raises(AssertionError, match=f"row 3 \\+ {N}"):
        moats[2]()
    moats[0](); moats[1]()


def test_unwritten_tile_is_nan_under_ff_and_differs_across_fills(monkeypatch):
    runs = {fill: _run(monkeypatch, fill, "skips a tile") for fill in FILLS}
    for got in runs[0xFF][:2]:
        assert not got.isfinite().all()
        assert got[16:32, 32:].isnan().all() and got[:16].isfinite().all()
    for k in (0, 1):
        assert not torch.equal(runs[0x00][k], runs[0x7B][k])
        assert not torch.equal(runs[0x00][k], runs[0xFF][k])
    for fill in FILLS:                                          # nothing outside the output was touched: only the value checks see it
        runs[fill][2].check()
        for check in runs[fill][3]:
            check()


def test_read_of_the_element_at_k_is_nan_under_ff_and_differs_across_fills(monkeypatch):
    a, b = _operands()
    runs = {fill: _run(monkeypatch, fill, "reads K") for fill in FILLS}
    for got in runs[0xFF][:2]:
        assert got.isnan().all()
    # under 0x00 the fault is invisible to a reference comparison -- which is why the suite could not see it so far
    want = a.double() @ b.double()
    assert ((runs[0x00][0].double() - want).abs() <= 2e-6 * (a.abs().double() @ b.abs().double())).all()
    for k in (0, 1):
        assert not torch.equal(runs[0x00][k], runs[0x7B][k])
        assert not torch.equal(runs[0x00][k], runs[0xFF][k])
    # with ld == K and no offset the element at K is the next row's first: only the last row reads the moat
    dense = _run(monkeypatch, 0xFF, "reads K", ld_pad=0, offset=0)[0]
    assert dense[M - 1].isnan().all() and dense[:M - 1].isfinite().all()


def test_fill_value_bytes():
    assert fill_value(0xFF, torch.float32).isnan().all() and fill_value(0xFF, torch.float64).isnan().all()
    assert int(fill_value(0xFF, torch.int32)) == -1 and int(fill_value(0x7B, torch.uint8)) == 123
    assert 1.3e36 < float(fill_value(0x7B, torch.float32)) < 1.31e36
