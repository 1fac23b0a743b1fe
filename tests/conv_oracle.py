"""Float64 oracle of Conv2d(k3, s1, p1) -> ReLU -> MaxPool2d(2, 2) and its gradients with a PER-ELEMENT error scale, for the conv kernels of
csrc/conv.hip, conv_b3.hip, conv_b3c1.hip and conv_wino.hip.  Built on oracle/reference_cpu.py (conv3x3_relu_pool, pool_decisions,
pool_windows).

Once the pooling decisions (a u8 mask: 0..3 = position in the 2x2 window, 4 = ReLU inactive) are fixed, every result is linear in each
operand, so the same computation on |x|, |w|, |b|, |gy| bounds the magnitude of the terms each element sums:

    y   sum |x||w| + |b| at the picked window position (0 where the mask says 4: the value must then be exactly 0)
    dw  sum |x||gy|        db  sum |gy|        dx  sum |gy||w|

An element passes when |got - want| <= C * scale + 1e-30, C = 2e-6: the constant tests/test_gpu_ops.py::test_gemm_layouts and
tests/test_gpu_poison_gemm.py hold the GEMM kernels to.  torch's own float32 CPU conv and autograd sit 5-25 x inside it on these inputs
(tests/test_conv_oracle_cpu.py recomputes that for every problem the GPU tests use and asserts a factor of 4; the forward of ``wide`` on
the stages of 32 and more input channels has a factor of 2, see there and C_MOVED below)."""
import functools

import torch

from oracle import reference_cpu as oracle

C = 2e-6
FLOOR = 1e-30
TIE_GAP = 1e-5         # a differing decision's picked pre-activation: within TIE_GAP x the output channel's mean |pre-activation| of the maximum
TIE_SHARE = 1e-4       # ... at fewer than this share of the windows

# The one place the constant was moved, (form, op, stage, input kind) -> c = 8 x the float32 CPU ratio of the same case
# (tests/test_conv_oracle_cpu.py holds each entry to that product): the f32 direct FORWARD (csrc/conv.hip: conv3x3_kernel) on ``wide`` at
# the two deep stages.  Measured on the MI355X: 2.81e-6 (W2) and 3.58e-6 (W3) of the scale; every other form and case is below 2e-6 (S2, same
# kernel, same inputs: 1.76e-6; the split-bf16 forms of W2 / W3: 1.55e-6 / 1.83e-6).  The cause is rounding, read off the kernel: its
# accumulator starts from the bias and runs over K = (4-channel chunk, tap, channel pair) with one v_mfma_f32_32x32x2 per pair, so the nine
# terms of the 1e3-scaled channel 0 arrive in the first chunk and each of the 9 cin / 2 - 18 accumulations that follow (270 at W2, 558 at
# W3, two products each) rounds at their magnitude -- about the whole scale -- where ``plain`` rounds at partial sums sqrt(n) times below it.
# A rounding error of standard deviation 2^-24 / sqrt(3) per addition over the 1116 products gives sqrt(1116) * 3.4e-8 = 1.1e-6 at W3; the
# worst of 5e5 elements sits 3 of those out.  torch's CPU conv sums the same terms in vector lanes and blocks (fewer roundings at full magnitude) and stays at
# 9.3e-7; the split-bf16 kernels accumulate 16 channels per MFMA.  The worst case of any float32 sum over n terms is n * 2^-24 of the scale.
C_MOVED = {("F32Direct", "fwd", "W2", "wide"): 8 * 9.40e-7, ("F32Direct", "fwd", "W3", "wide"): 8 * 9.30e-7}

STAGES = {"S1": (3, 32, 128), "S2": (32, 64, 64), "W1": (3, 64, 128), "W2": (64, 128, 64), "W3": (128, 256, 32)}      # cin, cout, map side
_SEED = {"S1": 1100, "S2": 1200, "W1": 1300, "W2": 1400, "W3": 1500}


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def flat_rows(hw):
    """Full-resolution rows [r0, r1) of the ``flat`` kind's band, and the pooled rows whose 3x3 neighbourhoods lie inside it."""
    r0, r1 = hw // 8 + hw // 32, hw // 2 + hw // 8 + hw // 16
    return (r0, r1), slice((r0 + 2) // 2, (r1 - 3) // 2 + 1)


def make_inputs(stage, B, kind):
    """float32 (x, w, b, gy).  ``plain``: what tests/test_gpu_ops.py::_conv_inputs makes.  ``wide``: input channel 0 times 1e3, the first
    quarter of the output channels' filters and biases times 1e-3 -- every bf16 piece of a split operand then carries weight somewhere,
    and small outputs sit beside large ones in one tensor.  ``flat``: image 0 with a band of ones across the left and right borders,
    every further image all ones (exact ties inside the pooling windows)."""
    cin, cout, hw = STAGES[stage]
    seed = _SEED[stage] + 10 * B + {"plain": 0, "wide": 1, "flat": 2}[kind]
    x = _rnd(B, cin, hw, hw, seed=seed)
    w = _rnd(cout, cin, 3, 3, seed=seed + 1, scale=0.2)
    b = _rnd(cout, seed=seed + 2, scale=0.1)
    gy = _rnd(B, cout, hw // 2, hw // 2, seed=seed + 3)
    if kind == "wide":
        x[:, 0] *= 1e3
        w[: cout // 4] *= 1e-3
        b[: cout // 4] *= 1e-3
    elif kind == "flat":
        (r0, r1), _ = flat_rows(hw)
        x[0, :, r0:r1, :] = 1.0
        x[1:] = 1.0
    return x, w, b, gy


def picked(pre, mask):
    """The pre-activation each pooled element takes under ``mask`` (0 where the mask says 4)."""
    m = mask.to(torch.int64)
    return oracle.pool_windows(pre).gather(-1, m.clamp(max=3).unsqueeze(-1)).squeeze(-1) * (m < 4).to(pre.dtype)


def gradients(x, w, b, gy, mask):
    """(y, dw, db, dx) of the stage under the decisions ``mask``, in the dtype of the operands (autograd through the oracle's stage)."""
    xr, wr, br = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    y = oracle.conv3x3_relu_pool(xr, wr, br, pool_mask=mask)
    y.backward(gy)
    return y.detach(), wr.grad, br.grad, xr.grad


class Problem:
    """One seeded input set, its float64 pre-activations and decisions; results under a mask are computed on request."""

    def __init__(self, stage, B, kind):
        self.stage, self.B, self.kind = stage, B, kind
        self.cin, self.cout, self.hw = STAGES[stage]
        self.x, self.w, self.b, self.gy = make_inputs(stage, B, kind)
        self._d = tuple(t.double() for t in (self.x, self.w, self.b, self.gy))
        self._pre = self._pre_abs = self._dec = self._own = None

    @property
    def pre(self):
        if self._pre is None:
            with torch.no_grad():
                self._pre = torch.nn.functional.conv2d(self._d[0], self._d[1], self._d[2], padding=1)
        return self._pre

    @property
    def pre_abs(self):
        if self._pre_abs is None:
            with torch.no_grad():
                self._pre_abs = torch.nn.functional.conv2d(self._d[0].abs(), self._d[1].abs(), self._d[2].abs(), padding=1)
        return self._pre_abs

    @property
    def decisions(self):
        """float64's own decisions (oracle.pool_decisions)."""
        if self._dec is None:
            self._dec = oracle.pool_decisions(self.pre)
        return self._dec

    def forward(self, mask):
        """(y, scale) under ``mask`` -- a form's own decisions, once check_decisions has passed them."""
        return picked(self.pre, mask), picked(self.pre_abs, mask)

    def backward(self, mask=None):
        """{"dw" | "db" | "dx": (want, scale)} under ``mask`` (default: float64's own decisions)."""
        if mask is None:
            if self._own is None:
                self._own = self.backward(self.decisions)
            return self._own
        _, dw, db, dx = gradients(*self._d, mask)
        _, sw, sb, sx = gradients(*(t.abs() for t in self._d), mask)
        return {"dw": (dw, sw), "db": (db, sb), "dx": (dx, sx)}

    def check_decisions(self, mask, what=""):
        """A form's forward mask may differ from float64's only at near-ties (TIE_GAP, per output channel) and at < TIE_SHARE of the
        windows.  Returns the share that differs."""
        mask = mask.cpu()
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(self.decisions.shape) and int(mask.max()) <= 4, what
        differ = mask != self.decisions
        share = float(differ.double().mean())
        if share:
            own = picked(self.pre, self.decisions)
            gap = (own - picked(self.pre, mask)).abs()
            tol = TIE_GAP * self.pre.abs().mean(dim=(0, 2, 3)).view(1, -1, 1, 1) + FLOOR
            bad = differ & (gap > tol)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} decisions differ from float64's beyond a near-tie, worst gap / tolerance {float((gap / tol)[differ].max()):.3e}"
            assert share < TIE_SHARE, f"{what}: decisions differ at a share of {share:.3e} of the windows"
        return share


@functools.lru_cache(maxsize=3)
def problem(stage, B, kind="plain"):
    return Problem(stage, B, kind)


def ratio(got, want, scale):
    """Worst |got - want| / scale over the elements with a nonzero scale (the rest must match to FLOOR: see within)."""
    err = (got.detach().cpu().double() - want).abs()
    nz = scale > 0
    return float((err[nz] / scale[nz]).max()) if bool(nz.any()) else 0.0


def within(got, want, scale, c=C):
    """(every element within c * scale + FLOOR, the worst ratio) -- an element of scale 0 must be exact."""
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    ok = bool(((got - want).abs() <= c * scale + FLOOR).all()) and bool(got.isfinite().all())
    return ok, ratio(got, want, scale)


def synthetic_mask(name, shape, seed=77):
    """Masks no forward produces: constants 0..4, i.i.d. uniform over 0..4, a checkerboard of 0 and 3."""
    if name.startswith("const"):
        return torch.full(shape, int(name[5:]), dtype=torch.uint8)
    if name == "uniform":
        return torch.randint(0, 5, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    assert name == "checker", name
    i = torch.arange(shape[-2]).view(-1, 1) + torch.arange(shape[-1]).view(1, -1)
    return ((i % 2) * 3).to(torch.uint8).expand(shape).contiguous()


SYNTHETIC = ["const0", "const1", "const2", "const3", "const4", "uniform", "checker"]
