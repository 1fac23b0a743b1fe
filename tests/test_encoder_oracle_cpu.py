"""CPU: tests/encoder_oracle.py against float64 torch autograd -- the yardstick of tests/test_gpu_encoder_rows.py and
tests/test_gpu_fold_ops.py must itself be the function nn.TransformerEncoderLayer computes outside attention.  Both sides are float64:
agreement to 1e-12 of each tensor's largest element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import encoder_oracle as E

REL = 1e-12


def close(got, want, what, scale=None):
    """``scale``: the size of the terms of a sum that may cancel (default: the largest element of ``want``)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max()) if scale is None else float(scale)
    assert err <= REL * scale + 1e-300, f"{what}: max err {err:.3e} at scale {scale:.3e}"


def T(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def torch_rows(ctx, xin, w, masks, nxt):
    """The stretch built from torch.nn.functional, float64, with explicit keep-scales; returns the intermediates by the oracle's names."""
    k1, k2, k3 = (T(m) for m in masks)
    F = ctx.shape[1]
    o = {}
    o["sa"] = TF.linear(ctx, w["wo"], w["bo"])
    o["z1"] = o["sa"] * k1 + xin
    o["y1"] = TF.layer_norm(o["z1"], (F,), w["g1"], w["be1"], E.EPS)
    o["pre"] = TF.linear(o["y1"], w["w1"], w["b1"])
    o["hff"] = torch.relu(o["pre"]) * k2
    o["ff"] = TF.linear(o["hff"], w["w2"], w["b2"])
    o["z2"] = o["ff"] * k3 + o["y1"]
    o["y2"] = TF.layer_norm(o["z2"], (F,), w["g2"], w["be2"], E.EPS)
    o["outn"] = None
    if nxt is not None:
        v = TF.linear(o["y2"], T(nxt["wn"]), T(nxt["bn"]))
        o["outn"] = torch.relu(v) if nxt["act"] else v
    return o


@pytest.mark.parametrize("kind", E.NEXT_KINDS)
@pytest.mark.parametrize("p,seeds,base", [(0.0, E.ROW_SEEDS, None), (0.1, E.ROW_SEEDS, None), (0.3, E.HIGH_SEEDS, E.SEED_BASE)])
@pytest.mark.parametrize("B,F,DFF", [(1, 4, 16), (5, 17, 70), (17, 167, 272)])
def test_rows_forward_and_backward_equal_float64_autograd(B, F, DFF, p, seeds, base, kind):
    """p = 0: the plain stretch.  p > 0: the same with the oracle's own masks (rowops_oracle's Philox stream) applied explicitly on the
    torch side.  The backward is evaluated from the forward's own float64 intermediates, with dyout and through stage 0."""
    ctx, xin, w, dyout, up = E.row_inputs(B, F, DFF)
    nxt = E.next_projection(kind, F)
    o = E.rows_fwd(ctx, xin, w, p=p, seeds=seeds, base=base, next=nxt)
    masks = o["masks"]
    if p > 0:
        inv_keep = np.float32(1) / (np.float32(1) - np.float32(p))
        for m, n in zip(masks, (B * F, B * DFF, B * F)):
            assert m.dtype == np.float32 and set(np.unique(m)) <= {np.float32(0), inv_keep}
            assert abs((m == 0).mean() - p) < 0.5 * p + 4 / np.sqrt(n)
        assert B * F < 64 or not np.array_equal(masks[0], masks[2])          # three streams
    tw = {k: T(v, grad=True) for k, v in w.items()}
    tctx, txin = T(ctx, grad=True), T(xin, grad=True)
    t = torch_rows(tctx, txin, tw, masks, nxt)
    for name in ("z1", "y1", "pre", "hff", "z2", "y2") + (("outn",) if nxt else ()):
        close(o[name], t[name].detach().numpy(), f"forward {name}")
    assert (o["outn"] is None) == (nxt is None)
    for i, z in ((1, t["z1"]), (2, t["z2"])):
        zz = z.detach()
        close(o[f"mean{i}"], zz.mean(dim=1).numpy(), f"mean{i}")
        close(o[f"rstd{i}"], (1 / torch.sqrt(zz.var(dim=1, unbiased=False) + E.EPS)).numpy(), f"rstd{i}")
    # ---- backward from dyout ----
    names = ("z2", "ff", "y1", "z1", "sa")
    grads = dict(zip(names + ("ctx",), torch.autograd.grad(t["y2"], [t[n] for n in names] + [tctx], T(dyout), retain_graph=True)))
    b = E.rows_bwd(o, w, dyout=dyout, p=p, seeds=(seeds[0], seeds[2]), base=base)
    # hff feeds linear2 only: its gradient is dff W2; the kernel's dhff is the gradient of linear1's OUTPUT (through the ReLU / dropout gate)
    dpre, = torch.autograd.grad(t["y2"], [t["pre"]], T(dyout), retain_graph=True)
    for name, want in (("dyout", T(dyout)), ("dz2", grads["z2"]), ("dff", grads["ff"]), ("dhff", dpre), ("dz1", grads["z1"]), ("dsa", grads["sa"]),
                       ("dctx", grads["ctx"])):
        close(b[name], want.numpy(), f"backward {name}")
    # dy1: y1 feeds linear1 and the residual of z2
    close(b["dy1"], grads["y1"].numpy(), "backward dy1")
    # ---- stage 0: dyout = dqkv_up Win_up + dz1_up is the input gradient of the layer above (in_proj of y2, plus its residual path) ----
    b0 = E.rows_bwd(o, w, up=up, p=p, seeds=(seeds[0], seeds[2]), base=base)
    y2 = t["y2"].detach().clone().requires_grad_(True)
    above = (TF.linear(y2, T(up["win_up"])) * T(up["dqkv_up"])).sum() + (y2 * T(up["dz1_up"])).sum()
    want_dyout, = torch.autograd.grad(above, [y2])
    close(b0["dyout"], want_dyout.numpy(), "stage 0 dyout")
    ref = E.rows_bwd(o, w, dyout=b0["dyout"], p=p, seeds=(seeds[0], seeds[2]), base=base)
    for name in E.BWD_NAMES:
        assert np.array_equal(b0[name], ref[name]), name


def test_rows_oracle_in_float32_stays_float32_and_near_float64():
    ctx, xin, w, dyout, up = E.row_inputs(17, 167, 272)
    nxt = E.next_projection("fc", 167)
    o64 = E.rows_fwd(ctx, xin, w, p=0.1, seeds=E.ROW_SEEDS, next=nxt)
    o32 = E.rows_fwd(ctx, xin, w, p=0.1, seeds=E.ROW_SEEDS, next=nxt, dtype=np.float32)
    for name in E.FWD_NAMES + ("outn",):
        assert o32[name].dtype == np.float32 and o64[name].dtype == np.float64
        assert np.abs(o32[name] - o64[name]).max() <= 1e-4 * np.abs(o64[name]).max(), name
    b32 = E.rows_bwd(o32, w, up=up, p=0.1, seeds=(11, 13), dtype=np.float32)
    assert all(b32[n].dtype == np.float32 for n in E.BWD_NAMES)


@pytest.mark.parametrize("with_bo", [True, False])
@pytest.mark.parametrize("F,B", [(1, 1), (5, 3), (64, 17), (167, 37)])
def test_fold_and_unfold_equal_autograd_of_the_unfolded_out_proj(F, B, with_bo):
    """z = out_proj(Pd (x Wv^T + bv)) unfolded against z = Pd (x W'^T + 1 b'^T) + bo folded: same z, and the gradients of Wo, bo, Wv, bv
    unfolded from dW', db' (the V block of the folded in_proj's weight gradient) equal autograd's."""
    (win,), (bin_,), (wo,), (bo,) = E.fold_inputs(F, 1)
    x, pd, dz = E.rnd(B, F, seed=1), np.abs(E.rnd(B, B, seed=2)), E.rnd(B, F, seed=3)
    wf, bf, wvt = E.fold(win, bin_, wo, bo if with_bo else None)
    assert np.array_equal(wf[:2 * F], win[:2 * F].astype(np.float64)) and np.array_equal(bf[:2 * F], bin_[:2 * F].astype(np.float64))
    assert np.array_equal(wvt[:F], win[2 * F:].T.astype(np.float64)) and np.array_equal(wvt[F], bin_[2 * F:].astype(np.float64))
    two, tbo = T(wo, grad=True), T(bo, grad=True)
    twv, tbv = T(win[2 * F:], grad=True), T(bin_[2 * F:], grad=True)
    z = TF.linear(T(pd) @ TF.linear(T(x), twv, tbv), two, tbo)
    # bo rides in b' only where the caller asks for it (no dropout between attention and the bias): then z = Pd (x W'^T + 1 b'^T) needs rows
    # of Pd that sum to 1 -- checked on the products themselves instead
    close(wf[2 * F:], (two @ twv).detach().numpy(), "W' = Wo Wv")
    close(bf[2 * F:], (two @ tbv + (tbo if with_bo else 0)).detach().numpy(), "b' = Wo bv (+ bo)")
    tw, tb = T(wf[2 * F:], grad=True), T(bf[2 * F:] - (bo.astype(np.float64) if with_bo else 0), grad=True)
    zf = T(pd) @ TF.linear(T(x), tw, tb) + tbo.detach()
    close(zf.detach().numpy(), z.detach().numpy(), "folded z")
    tdw, tdb = torch.autograd.grad(zf, [tw, tb], T(dz))
    want = torch.autograd.grad(z, [two, tbo, twv, tbv], T(dz))
    got = E.unfold(tdw.numpy(), tdb.numpy(), wo, wvt, dz)
    for g, w_, name in zip(got, want, ("dWo", "dbo", "dWv", "dbv")):
        close(g, w_.numpy(), name)


@pytest.mark.parametrize("n,rows,cols", [(1, 1, 1), (2, 33, 17), (3, 100, 167)])
def test_ln_param_grad_equals_autograd_of_layer_norm(n, rows, cols):
    for dy, z, mean, rstd in E.ln_grad_inputs(n, rows, cols):
        g, b = T(np.ones(cols), grad=True), T(np.zeros(cols), grad=True)
        y = TF.layer_norm(T(z), (cols,), g, b, E.EPS)
        want_g, want_b = torch.autograd.grad(y, [g, b], T(dy))
        z64 = z.astype(np.float64)
        mean64 = z64.mean(axis=1)
        rstd64 = 1 / np.sqrt(z64.var(axis=1) + E.EPS)
        assert np.abs(mean - mean64).max() <= 1e-6 * max(1.0, np.abs(mean64).max()) and np.abs(rstd / rstd64 - 1).max() <= 1e-6
        got_g, got_b = E.ln_param_grad(dy, z, mean64, rstd64)
        # one column: xhat is 0 up to rounding on either side, so the sum is held to the size of dy, not to its own
        close(got_g, want_g.numpy(), "dgamma", scale=np.abs(dy).sum(axis=0).max())
        close(got_b, want_b.numpy(), "dbeta")
