"""GPU: the weight-resident short-K NN form of the split-bf16 GEMM (csrc/gemm.hip: gemm_b3r_kernel, the image FC's input gradient)
against the 128 x 128 tile form it replaces (gemm_b3_kernel<1>) -- equal bits -- and against float64.

The GEMM knobs are read once per process, so each form runs in a child process (tests/gemm_resident_cases.py): BBBP_GEMM_B_RESIDENT=2
puts every product of the form's description on gemm_b3_kernel<1> whatever its size, =3 on gemm_b3r_kernel.  Both children run at the
same time, once per test session."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_resident_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def forms(tmp_path_factory, dev):
    tmp = tmp_path_factory.mktemp("gemm_resident")
    procs = {}
    for knob in (2, 3):
        env = dict(os.environ, BBBP_GEMM_B_RESIDENT=str(knob))
        procs[knob] = subprocess.Popen([sys.executable, os.path.join(cases.ROOT, "tests", "gemm_resident_cases.py"), str(tmp / f"form{knob}.npz")],
                                       cwd=cases.ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for knob, pr in procs.items():
        log, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, f"BBBP_GEMM_B_RESIDENT={knob} child failed ({pr.returncode}):\n{log[-4000:]}"
        res[knob] = dict(np.load(tmp / f"form{knob}.npz"))
    return res[2], res[3]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def close_to_float64(got, want, scale):
    """The bound of tests/test_gpu_ops.py::test_gemm_layouts for the split-bf16 GEMMs."""
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 2e-6 * scale + 1e-30).all(), f"max err ratio {(err / (scale + 1e-30)).max():.3e}"


@pytest.mark.parametrize("M,N,K", cases.MAIN)
def test_resident_form_has_the_bits_of_the_tile_form_and_meets_float64(forms, M, N, K):
    old, new = forms
    key = f"{M}x{N}x{K}"
    assert int(old["form/" + key]) == cases.FORM_B3 and int(new["form/" + key]) == cases.FORM_RESIDENT
    assert same_bits(old["main/" + key], new["main/" + key])
    a, b = (t.double() for t in cases.operands(M, N, K))
    close_to_float64(new["main/" + key], (a @ b).numpy(), (a.abs() @ b.abs()).numpy())


@pytest.mark.parametrize("name,M,N,K,batch", cases.FALLBACK)
def test_products_outside_the_forms_description_keep_their_plan(forms, name, M, N, K, batch):
    old, new = forms
    assert int(new["form/" + name]) != cases.FORM_RESIDENT
    assert int(new["form/" + name]) == int(old["form/" + name])
    assert same_bits(old["fallback/" + name], new["fallback/" + name])
    a, b = (t.double() for t in cases.operands(M, N, K, batch))
    close_to_float64(new["fallback/" + name], (a @ b).numpy(), (a.abs() @ b.abs()).numpy())


def test_resident_form_epilogues(forms):
    """alpha + residual, gate, gate after the residual, bias + ReLU: the bits of the tile form, and the float64 result."""
    old, new = forms
    M, N, K = 300, 384, 128
    a, b = (t.double() for t in cases.operands(M, N, K))
    res, gate, bias = (t.double() for t in cases.epilogue_operands(M, N))
    prod, scale = a @ b, (a.abs() @ b.abs()).numpy()
    want = {"residual": 0.5 * prod + res, "gate": prod * (gate > 0) * 1.25, "gate_after_residual": (prod + res) * (gate > 0) * 1.25,
            "bias_relu": torch.relu(0.5 * prod + bias)}
    for name, w in want.items():
        assert same_bits(old["epilogue/" + name], new["epilogue/" + name]), name
        close_to_float64(new["epilogue/" + name], w.numpy(), scale + 1.0)


def test_training_step_is_bit_identical_with_the_resident_form(forms):
    """One training step of MixedInputModel (F = 64, B = 256: the image FC's input gradient is 256 x 65536 x 128, two row tiles): the
    output and every gradient."""
    old, new = forms
    assert int(old["form/engine"]) == cases.FORM_B3 and int(new["form/engine"]) == cases.FORM_RESIDENT
    assert list(old["engine/names"]) == list(new["engine/names"]) and len(old["engine/names"]) > 100
    assert all(np.isfinite(new["engine/sums"])) and float(new["engine/sums"][1:].sum()) > 0.0
    differ = [str(n) for n, x, y in zip(old["engine/names"], old["engine/digests"], new["engine/digests"]) if x != y]
    assert not differ, f"tensors that differ between the two forms: {differ[:8]}"
