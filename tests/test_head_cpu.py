"""CPU: tests/head_oracle.py itself, and the argument checks of bbbp_head_fwd / bbbp_head_bwd.

On the forward pass's manifold the oracle is compared with torch float64 autograd of the same composition.  Off it -- saved tensors no
forward pass produces, the inputs that make the fusion block's backward visible -- autograd has nothing to say, so every stage's VJP is
compared with torch's own backward op for that stage, which takes the saved output as an argument: _softmax_backward_data, tanh_backward,
threshold_backward, native_batch_norm_backward with given save_mean / save_invstd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_oracle as H
from bbbp_amd import _lib
from helpers import assert_close

aten = torch.ops.aten
T64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
TIGHT = dict(rtol=1e-10, atol_frac=1e-12)
BATCHES = (2, 15, 16, 17, 33, 100, 530)


def torch_forward(comb, p, running, training):
    """The composition in torch float64; returns (tensors by the oracle's names, running statistics after the call)."""
    P = {k: ([T64(a) for a in v] if k in H.PER_HEAD else T64(v)) for k, v in p.items()}
    for k in ("gamma", "beta"):
        P[k].requires_grad_(True)
    o = {"comb": T64(comb).requires_grad_(True)}
    o["pre"] = torch.stack([F.linear(o["comb"], P["fw1"][h], P["fb1"][h]) for h in range(4)])
    o["hid"] = torch.tanh(o["pre"])
    o["logit"] = torch.stack([F.linear(o["hid"][h], P["fw2"][h][None, :], P["fb2"][h])[:, 0] for h in range(4)], dim=1)
    o["attn"] = torch.softmax(o["logit"], dim=1)
    o["fused"] = (o["attn"][:, :, None] * o["comb"][:, None, :]).sum(dim=1)
    o["h"] = torch.relu(F.linear(o["fused"], P["w0"], P["b0"]))
    rm, rv = T64(running[0]).clone(), T64(running[1]).clone()
    o["hb"] = F.batch_norm(o["h"], rm, rv, P["gamma"], P["beta"], training=training, momentum=H.MOMENTUM, eps=H.EPS)
    o["h2"] = torch.relu(F.linear(o["hb"], P["w3"], P["b3"]))
    o["h3"] = torch.relu(F.linear(o["h2"], P["w5"], P["b5"]))
    o["out"] = F.linear(o["h3"], P["w7"][None, :], P["b7"])[:, 0]
    for k in ("pre", "logit", "h", "hb", "h2", "h3"):
        o[k].retain_grad()
    return o, P, (rm, rv)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", [2, 17, 100])
def test_oracle_matches_torch_autograd_on_the_manifold(B, training):
    p, running = H.make_params()
    comb, dout = H.make_comb(B), H.make_dout(B)
    want, P, (rm, rv) = torch_forward(comb, p, running, training)
    got = H.forward(comb, p, running, training)
    for k in H.FORWARD_OUT:
        if k not in ("bn_mean", "bn_rstd"):
            assert_close(got[k], want[k].detach().numpy(), what=f"B={B} {k}", **TIGHT)
    assert_close(got["running_mean"], rm.numpy(), what="running_mean", **TIGHT)
    assert_close(got["running_var"], rv.numpy(), what="running_var", **TIGHT)
    if training:
        h = want["h"].detach()
        assert_close(got["bn_mean"], h.mean(0).numpy(), what="bn_mean", **TIGHT)
        assert_close(got["bn_rstd"], (h.var(0, unbiased=False) + H.EPS).rsqrt().numpy(), what="bn_rstd", **TIGHT)
    else:
        assert np.array_equal(got["running_mean"], running[0].astype(np.float64)) and np.array_equal(got["running_var"], running[1].astype(np.float64))
    want["out"].backward(T64(dout))
    back = H.backward(dout, dict(got, comb=comb), p, training)
    # hb is the BatchNorm's OUTPUT, the oracle's dhb the gradient there; dh the gradient at the ReLU's input (autograd's at the output h
    # is the unmasked one: mask it)
    for k, w in (("dh3", want["h3"].grad * (want["h3"] > 0)), ("dh2", want["h2"].grad * (want["h2"] > 0)), ("dhb", want["hb"].grad),
                 ("dh", want["h"].grad * (want["h"] > 0)), ("dcomb", want["comb"].grad * (want["comb"] > 0)),
                 ("dgamma", P["gamma"].grad), ("dbeta", P["beta"].grad)):
        assert_close(back[k], w.detach().numpy(), what=f"B={B} training={training} {k}", **TIGHT)
    # the analytic zero: sum_h a_h = 1, so dlogit_h = a_h (t - t sum a) is what float64 rounding leaves of t, and autograd's is no more
    t = np.abs(back["t"])
    assert t.min() > 0 and (np.abs(back["dlogit"]) <= 1e-15 * t[None, :]).all()
    assert (np.abs(want["logit"].grad.numpy().T) <= 1e-15 * t[None, :]).all()
    w2 = np.abs(np.stack(p["fw2"]).astype(np.float64))
    assert (np.abs(back["dpre"]) <= 1e-15 * t[None, :, None] * w2[:, None, :]).all()
    # ... which the float32 floor of the GPU test covers with room, and is itself noise against the terms it is made of
    dl_floor, dpre_floor = H.fusion_noise_floor(dout, dict(got, comb=comb), p, training)
    assert (np.abs(back["dlogit"]) <= dl_floor).all() and (np.abs(back["dpre"]) <= dpre_floor).all()
    assert (dl_floor <= 1e-5 * t[None, :] + 1e-9 * np.abs(back["dfused"]).max() * np.abs(comb).max() * 256).all()


# ---- off the manifold ---------------------------------------------------------------------------------------------------------------------
def test_stage_vjps_match_torchs_backward_ops_on_arbitrary_saved_outputs():
    rng = np.random.default_rng(5)
    B = 37
    dy, y = rng.standard_normal((B, 256)), rng.uniform(-1, 1, (B, 256))
    assert_close(H.tanh_vjp(dy, y), aten.tanh_backward(T64(dy), T64(y)).numpy(), what="tanh", **TIGHT)
    y0 = np.where(rng.random((B, 256)) < 0.5, 0, np.abs(y))
    assert_close(H.relu_vjp(dy, y0), aten.threshold_backward(T64(dy), T64(y0), 0).numpy(), what="relu", **TIGHT)
    a = rng.uniform(0.05, 0.4, (B, 4))                       # rows do not sum to 1
    da = rng.standard_normal((B, 4))
    assert_close(H.softmax_vjp(da, a), torch._softmax_backward_data(T64(da), T64(a), 1, torch.float64).numpy(), what="softmax", **TIGHT)
    gamma, mean, rstd = 1 + 0.3 * rng.standard_normal(256), 0.3 * rng.standard_normal(256), rng.uniform(0.5, 3.0, 256)
    for training in (True, False):
        # eval: torch derives invstd from running_var, so hand it the variance that gives this rstd
        rv = T64(1 / rstd ** 2 - H.EPS)
        want = aten.native_batch_norm_backward(T64(dy), T64(y0), T64(gamma), T64(mean), rv, T64(mean), T64(rstd), training, H.EPS, [True, True, True])
        for name, g, w in zip(("dx", "dgamma", "dbeta"), H.batchnorm_vjp(dy, y0, gamma, mean, rstd, training), want):
            assert_close(g, w.numpy(), what=f"batchnorm training={training} {name}", rtol=1e-9, atol_frac=1e-11)


def torch_backward(dout, s, p, training):
    """The chain over saved tensors, every nonlinearity's backward by torch's own op."""
    P = {k: ([T64(a) for a in v] if k in H.PER_HEAD else T64(v)) for k, v in p.items()}
    s = {k: T64(v) for k, v in s.items()}
    o = {}
    o["dh3"] = aten.threshold_backward(T64(dout)[:, None] * P["w7"][None, :], s["h3"], 0)
    o["dh2"] = aten.threshold_backward(o["dh3"] @ P["w5"], s["h2"], 0)
    o["dhb"] = o["dh2"] @ P["w3"]
    rv = 1 / s["bn_rstd"] ** 2 - H.EPS
    dx, o["dgamma"], o["dbeta"] = aten.native_batch_norm_backward(o["dhb"], s["h"], P["gamma"], s["bn_mean"], rv, s["bn_mean"], s["bn_rstd"],
                                                                    training, H.EPS, [True, True, True])
    o["dh"] = aten.threshold_backward(dx, s["h"], 0)
    dfused = o["dh"] @ P["w0"]
    # fused = sum_h attn_h * comb, by autograd with attn and comb as leaves (a bilinear form: no saved output involved)
    attn, comb = s["attn"].clone().requires_grad_(True), s["comb"].clone().requires_grad_(True)
    (attn[:, :, None] * comb[:, None, :]).sum(dim=1).backward(dfused)
    dlogit = torch._softmax_backward_data(attn.grad, s["attn"], 1, torch.float64)
    o["dlogit"] = dlogit.T.contiguous()
    o["dpre"] = torch.stack([aten.tanh_backward(dlogit[:, h, None] * P["fw2"][h][None, :], s["hid"][h]) for h in range(4)])
    dcomb = comb.grad + sum(o["dpre"][h] @ P["fw1"][h] for h in range(4))
    o["dcomb"] = aten.threshold_backward(dcomb, s["comb"], 0)
    return {k: v.detach().numpy() for k, v in o.items()}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B", [17, 100])
def test_oracle_backward_off_the_manifold_matches_the_chain_of_torchs_backward_ops(B, training):
    p, _ = H.make_params()
    s, dout = H.off_manifold(B), H.make_dout(B)
    sums = s["attn"].sum(axis=1)
    assert 0.49 < sums.min() and sums.max() < 0.91 and (s["attn"] > 0).all() and np.abs(s["hid"]).max() < 1
    for k in ("comb", "h", "h2", "h3"):
        assert 0.4 < (s[k] == 0).mean() < 0.6
    got, want = H.backward(dout, s, p, training), torch_backward(dout, s, p, training)
    for k in H.BACKWARD_OUT:
        assert_close(got[k], want[k], what=f"B={B} training={training} {k}", rtol=1e-9, atol_frac=1e-11)
    # here the fusion block's gradient has full magnitude: dlogit ~ a_h t (1 - sum a), and the W1 product carries weight in dcomb
    assert np.abs(got["dlogit"]).max() > 0.05 * np.abs(got["t"]).max() * s["attn"].max() * 0.1
    through_w1 = sum(got["dpre"][h] @ p["fw1"][h].astype(np.float64) for h in range(4)) * (s["comb"] > 0)
    assert np.abs(through_w1).max() > 0.05 * np.abs(got["dcomb"]).max()


# ---- what the GPU cases claim about their inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_dead_columns_are_dead_and_offset_columns_sit_far_from_zero(B):
    p, running = H.make_params(case="dead_offset")
    o = H.forward(H.make_comb(B), p, running, True)
    dead, off = list(H.DEAD_COLUMNS), list(H.OFFSET_COLUMNS)
    assert (o["h"][:, dead] == 0).all() and (o["bn_mean"][dead] == 0).all()
    assert np.allclose(o["bn_rstd"][dead], H.EPS ** -0.5) and np.array_equal(o["hb"][:, dead], np.broadcast_to(p["beta"][dead].astype(np.float64), (B, 3)))
    spread = o["h"][:, off].std(axis=0)
    assert (o["h"][:, off].min(axis=0) > 40).all() and (o["bn_mean"][off] > 15 * spread).all() and (spread > 0).all()
    o32 = H.forward(H.make_comb(B), p, running, True, dtype=np.float32)
    assert all(v is None or v.dtype == np.float32 for v in o32.values())
    assert (o32["h"][:, dead] == 0).all()


def test_saturated_case_has_underflowed_heads_and_tied_rows_in_float32():
    p, running = H.make_params(case="saturated")
    for B in (17, 100):
        o = H.forward(H.make_comb(B), p, running, True, dtype=np.float32)
        a = o["attn"]
        assert np.isfinite(a).all() and np.abs(a.sum(axis=1) - 1).max() < 1e-6
        assert ((a == 0).sum(axis=1) == 3).any(), "no row that one head takes alone, the others underflowing to 0"
        assert np.array_equal(a[:, 0], a[:, 1]) and (a[:, 0] == 0.5).any(), "heads 0 and 1 tie; in some rows they share everything"
        assert 0 < (a == 0).mean() < 0.9


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def _fwd_args(B=4, training=1, concat=0, world=1, rank=0, null=None):
    fake = ctypes.c_void_p(4096)                         # never dereferenced: validation comes first
    four = lambda: _lib.ptr_array([4096] * 4)
    a = [None, fake, four(), four(), four(), four()] + [fake] * 23 + [B, training, concat, world, rank]
    if null is not None:
        a[null] = None
    return a


def _bwd_args(B=4, training=1, world=1, rank=0, null=None):
    fake = ctypes.c_void_p(4096)
    four = lambda: _lib.ptr_array([4096] * 4)
    a = [None] + [fake] * 10 + [four(), four()] + [fake] * 14 + [B, training, world, rank]
    if null is not None:
        a[null] = None
    return a


def test_head_entry_points_validate_their_arguments_before_touching_the_gpu():
    L = _lib.lib()
    ERR_ARG = 1
    for null in range(1, 29):
        assert L.bbbp_head_fwd(*_fwd_args(null=null)) == ERR_ARG, null
        assert b"null pointer" in L.bbbp_last_error()
    for null in range(1, 27):
        assert L.bbbp_head_bwd(*_bwd_args(null=null)) == ERR_ARG, null
        assert b"null pointer" in L.bbbp_last_error()
    a = _fwd_args()
    a[2] = _lib.ptr_array([4096, 4096, None, 4096])      # one head's weight missing
    assert L.bbbp_head_fwd(*a) == ERR_ARG and b"null pointer" in L.bbbp_last_error()
    a = _fwd_args(concat=1)
    for i in (2, 3, 4, 5, 18, 19, 20):                   # concat: the fusion block's parameters and outputs are not needed ...
        a[i] = None
    a[28] = None                                          # ... partial still is
    assert L.bbbp_head_fwd(*a) == ERR_ARG and b"null pointer" in L.bbbp_last_error()
    for fn, args in ((L.bbbp_head_fwd, _fwd_args), (L.bbbp_head_bwd, _bwd_args)):
        assert fn(*args(B=0)) == ERR_ARG and b"empty batch" in L.bbbp_last_error()
        assert fn(*args(B=-3)) == ERR_ARG
        for world, rank in ((1, 1), (2, 2), (2, -1), (0, 0)):
            assert fn(*args(world=world, rank=rank)) == ERR_ARG and b"rank" in L.bbbp_last_error(), (world, rank)
        assert fn(*args(B=1, training=1)) == ERR_ARG
        assert b"Expected more than 1 value per channel when training, got input size [1, 256]" in L.bbbp_last_error()
