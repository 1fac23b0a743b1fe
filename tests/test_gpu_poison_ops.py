"""GPU: the op-level checkers of test_gpu_ops.py again, with every output and workspace allocated from poisoned, guarded pools.

Each case runs under the three fills of tests/poison.py (0x00 twice): the checker's own reference comparison holds under each, the returned
tensors are finite, no guard band is touched, and the results are bit-identical -- first between the two 0x00 runs (the kernels use no float
atomics, so a difference there would be a race, not a fill), then across the fills (a difference there is a read of uninitialised memory)."""
import pytest
import torch

from bbbp_amd import _lib, ops
from oracle import reference_cpu as oracle
from helpers import assert_close
from poison import moated, poisoned_allocations
from test_gpu_ops import (_batchnorm_case, _bias_act_bwd_and_mse_case, _conv_case, _conv_inputs, _conv_run, _dropout_case, _layernorm_case,
                          _layernorm_dropout_case, _softmax_case, rnd)

pytestmark = pytest.mark.gpu

RUNS = (("0x00", 0x00), ("0x00 again", 0x00), ("0xFF", 0xFF), ("0x7B", 0x7B))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def assert_fill_independent(results, what):
    """``results``: {run name: sequence of tensors (None allowed)} for RUNS."""
    first = results["0x00"]
    for name in ("0x00 again", "0xFF", "0x7B"):         # same fill first
        other = results[name]
        assert len(other) == len(first)
        for i, (a, b) in enumerate(zip(first, other)):
            assert (a is None) == (b is None)
            if a is not None:
                assert same_bits(a, b), f"{what}: returned tensor {i} differs between the runs under 0x00 and under {name}"
    for name, outs in results.items():
        for i, t in enumerate(outs):
            if t is not None:
                assert bool(t.isfinite().all()), f"{what}: returned tensor {i} is not finite under {name}"      # every reference here is finite


def under_every_fill(monkeypatch, run, what):
    results = {}
    for name, fill in RUNS:
        with poisoned_allocations(monkeypatch, fill) as pa:
            results[name] = tuple(run())
        assert pa.check() > 0, f"{what}: no allocation went through the pools"
        pa.release()
    assert_fill_independent(results, what)


@pytest.fixture
def conv_form():
    L = _lib.lib()
    old = L.bbbp_get_conv_winograd()

    def set_(form):
        _lib.check(L.bbbp_set_conv_winograd(form), "bbbp_set_conv_winograd")
    yield set_
    L.bbbp_set_conv_winograd(old)


def _conv_under_every_fill(dev, monkeypatch, B, cin, cout, hw, seed):
    """The full checker (float64 oracle) once, under 0xFF; the device calls alone under the other fills, compared bit for bit."""
    results = {}
    with poisoned_allocations(monkeypatch, 0xFF) as pa:
        results["0xFF"] = _conv_case(dev, B, cin, cout, hw, seed)
    assert pa.check() > 0
    inputs = _conv_inputs(B, cin, cout, hw, seed)
    for name, fill in RUNS:
        if name != "0xFF":
            with poisoned_allocations(monkeypatch, fill) as pa:
                results[name] = _conv_run(dev, *inputs)
            assert pa.check() > 0
            assert int(results[name][1].max()) <= 4, f"pooling decisions out of range under {name}"
    assert_fill_independent(results, f"conv {cin}->{cout} B={B}")


# seeds as in test_conv1_3to32 / test_conv2_32to64 / test_conv_wide_deep_shapes / test_conv_many_strips_persistent_loop
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", [0, 32, 96], ids=["f32", "split-bf16-wgrad", "split-bf16-fwd+wgrad"])
def test_conv1_under_poison(dev, monkeypatch, conv_form, form, B):
    conv_form(form)
    _conv_under_every_fill(dev, monkeypatch, B, 3, 32, 128, seed=10 + B)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("form", [0, 3, 28, 28 | 128, 28 | 128 | 256],
                         ids=["direct", "winograd", "split-bf16", "split-bf16-sparse-wgrad-8w", "split-bf16-sparse-wgrad-4w"])
def test_conv2_under_poison(dev, monkeypatch, conv_form, form, B):
    conv_form(form)
    _conv_under_every_fill(dev, monkeypatch, B, 32, 64, 64, seed=20 + B)


@pytest.mark.parametrize("cin,cout,hw", [(3, 64, 128), (64, 128, 64), (128, 256, 32)])
def test_conv_wide_deep_under_poison(dev, monkeypatch, cin, cout, hw):
    _conv_under_every_fill(dev, monkeypatch, 2, cin, cout, hw, seed=100 + cin + 2)


@pytest.mark.parametrize("B,cin,cout,hw,seed", [(24, 3, 32, 128, 42), (40, 32, 64, 64, 41)], ids=["conv1-B24", "conv2-B40"])
def test_conv_many_strips_under_poison(dev, monkeypatch, B, cin, cout, hw, seed):
    _conv_under_every_fill(dev, monkeypatch, B, cin, cout, hw, seed)


@pytest.mark.parametrize("rows,cols", [(5, 7), (3, 1024), (5, 1022), (2, 4096), (3, 4100)])
def test_layernorm_under_poison(dev, monkeypatch, rows, cols):
    under_every_fill(monkeypatch, lambda: _layernorm_case(dev, rows, cols), f"layernorm {rows}x{cols}")


def test_layernorm_dropout_under_poison(dev, monkeypatch):
    under_every_fill(monkeypatch, lambda: _layernorm_dropout_case(dev, 3, 1500), "layernorm + dropout 3x1500")


@pytest.mark.parametrize("rows,cols", [(9, 9), (70, 33), (3, 4096)])
def test_softmax_under_poison(dev, monkeypatch, rows, cols):
    """The checker's two calls work in place on clones; the dropped probabilities of a call with dropout are the kernel's one allocated
    output: each is 0 or its probability scaled up."""
    def run():
        p, ds = _softmax_case(dev, rows, cols)
        p2, pd = ops.softmax_fwd(rnd(rows, cols, seed=1, scale=3.0).to(dev), dropout_p=0.3, seed=5)
        assert torch.equal(p2, p) and bool(((pd == 0) | (pd >= p)).all())
        return p, ds, pd
    under_every_fill(monkeypatch, run, f"softmax {rows}x{cols}")


def test_batchnorm_under_poison(dev, monkeypatch):
    under_every_fill(monkeypatch, lambda: _batchnorm_case(dev), "batchnorm")


def test_mse_and_dense_bias_act_bwd_under_poison(dev, monkeypatch):
    under_every_fill(monkeypatch, lambda: _bias_act_bwd_and_mse_case(dev), "bias_act_bwd + mse")


def test_dropout_under_poison(dev, monkeypatch):
    under_every_fill(monkeypatch, lambda: _dropout_case(dev), "dropout")


@pytest.mark.parametrize("rows,cols", [(50, 70), (37, 5), (3, 1022)])
def test_bias_act_bwd_on_a_strided_slice_under_poison(dev, monkeypatch, rows, cols):
    """dy and y as column slices of wider buffers (how the head's gradient sits inside ``combined``): the rest of either row is poison, dy is
    updated in place inside its extent only, db comes from a guarded allocation.  Tolerances of test_bias_act_bwd_and_mse."""
    y_h, dy_h = torch.relu(rnd(rows, cols, seed=1)), rnd(rows, cols, seed=2)
    want = dy_h * (y_h > 0)
    results = {}
    for name, fill in RUNS:
        d, check_d = moated(dy_h, fill, ld=cols + 3, offset=1, device=dev)
        y, check_y = moated(y_h, fill, ld=cols + 5, offset=3, device=dev)
        with poisoned_allocations(monkeypatch, fill) as pa:
            db = ops.bias_act_bwd(d, y, act="relu")
        assert_close(d.cpu().numpy(), want.numpy(), rtol=1e-6, what="relu bwd")
        assert_close(db.cpu().numpy(), want.double().sum(0).numpy(), rtol=1e-5, what="db")
        assert pa.check() == 1
        check_d(); check_y()
        results[name] = (d.contiguous(), db)
    assert_fill_independent(results, "bias_act_bwd on a slice")


def _adamw_buffers(fill, dev, tensors):
    return [moated(t, fill, device=dev) for t in tensors]      # contiguous, 256-byte aligned, the guard right behind the last element


def test_adamw_step_under_poison(dev):
    """1003 elements: the last float4 of the vector body would cover one element of the guard behind each of the four buffers."""
    n = 1003
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for step in range(1, 4):
        oracle.adamw_step(p, g0 * step, m, v, step)
    results = {}
    for name, fill in RUNS:
        (pd, cp), (md, cm), (vd, cv) = _adamw_buffers(fill, dev, [p0, torch.zeros(n), torch.zeros(n)])
        for step in range(1, 4):
            gd, cg = moated(g0 * step, fill, device=dev)
            ops.adamw_step_(pd, gd, md, vd, step)
            cg()
        assert pd.data_ptr() % 16 == 0
        assert_close(pd.cpu().numpy(), p.numpy(), rtol=1e-5, what="adamw p")
        assert_close(vd.cpu().numpy(), v.numpy(), rtol=1e-5, what="adamw v")
        cp(); cm(); cv()
        results[name] = (pd, md, vd)
    assert_fill_independent(results, "adamw_step_")


@pytest.mark.parametrize("with_hyper", [False, True], ids=["scalars", "device-hyper"])
def test_adamw_step_multi_under_poison(dev, with_hyper):
    """One flat parameter / moment buffer, four gradient tensors of 5, 1, 167 and 1022 elements (no boundary a multiple of 4)."""
    sizes = [5, 1, 167, 1022]
    n = sum(sizes)
    p0 = rnd(n, seed=1)
    grads = [rnd(s, seed=10 + i) for i, s in enumerate(sizes)]
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for step in range(1, 3):
        oracle.adamw_step(p, torch.cat(grads) * step, m, v, step)
    results = {}
    for name, fill in RUNS:
        (pd, cp), (md, cm), (vd, cv) = _adamw_buffers(fill, dev, [p0, torch.zeros(n), torch.zeros(n)])
        for step in range(1, 3):
            gds = [moated(g * step, fill, device=dev) for g in grads]
            offs = [0]
            for s in sizes:
                offs.append(offs[-1] + s)
            table, ct = moated(torch.tensor(offs + [g.data_ptr() for g, _ in gds], dtype=torch.int64), fill, device=dev)
            hyper = None
            if with_hyper:
                hyper, ch = moated(torch.zeros(8), fill, device=dev)
                ops.adamw_hyper_store_(hyper, step)
            ops.adamw_step_multi_(pd, md, vd, table, len(sizes), step, hyper=hyper)
            torch.cuda.synchronize()
            for _, cg in gds:
                cg()
            ct()
            if with_hyper:
                ch()
        assert_close(pd.cpu().numpy(), p.numpy(), rtol=1e-5, what="adamw multi p")
        assert_close(vd.cpu().numpy(), v.numpy(), rtol=1e-5, what="adamw multi v")
        cp(); cm(); cv()
        results[name] = (pd, md, vd)
    assert_fill_independent(results, "adamw_step_multi_")
