"""GPU: parity at the sizes that are BENCHMARKED (BASELINE configs 3 and 5) and of the optimizer against the reference's own
AdamW trajectory -- the small-batch goldens and oracle checks in test_gpu_model.py cover every code path, these cover the
grids, partitions and slab counts that only exist at full size."""
import numpy as np
import pytest
import torch

import bbbp_amd
from bbbp_amd import _lib
from oracle import reference_cpu as oracle
from helpers import assert_close, assert_close_or_as_accurate_as_fp32, check_summary_adam, golden, synth_inputs
from test_gpu_model import FUSION, build, zero_dropout

pytestmark = pytest.mark.gpu


def oracle_params(m, double=True):
    return {k: ((v.detach().cpu().double() if double else v.detach().cpu()) if v.dtype.is_floating_point else v.detach().cpu()).clone()
            .requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in m.state_dict().items()}


def check_b512_step_against_float64(dev, F, seed, conv_mask, max_flips=8):
    """One B = 512 training step (train mode, branch overlap ON, dropout 0) of MixedInputModel(F): output, loss, BatchNorm running
    statistics and EVERY element of every non-degenerate gradient against the float64 oracle.

    ReLU kinks: a step has 6.3 M hidden FFN activations, and a float32 pre-activation carries ~1e-7 of rounding, so in about
    every second step ONE of them lands on the other side of zero than in float64 (measured: tools/exp_b512_accuracy.py).  That
    single decision moves its unit's linear1 weight-gradient row by percents (the batch has only 512 rows) and everything
    upstream by 2-5e-4 -- in ANY float32 implementation, torch's CPU path included.  So the oracle is evaluated with the
    GPU's own FFN ReLU decisions (bbbp_mixed_debug_ffn_gate), after checking that they differ from float64's only where the
    float64 pre-activation is within 2e-6 of zero, and at no more than a handful of elements.

    Pooling ties: the same effect in the conv stages, 10^8 windows per step.  A 2x2 window whose two largest pre-activations agree
    to float32 rounding routes its gradient to either element (and a maximum within rounding of zero passes or blocks it), and the
    conv weight / bias gradients are 10^7-term cancelling sums over those decisions -- round 2 could hold them only to "as accurate
    as torch-CPU float32".  Now the oracle is evaluated with the GPU's own saved decisions (bbbp_mixed_debug_pool_mask) after
    checking that they differ from float64's only at such near-ties (value picked vs float64's maximum within 1e-5 of the mean
    |pre-activation|) and at <= 1e-4 of the windows; with that the conv tensors meet float64 ELEMENT-WISE at the tolerance of
    every other tensor."""
    L = _lib.lib()
    B = 512
    m = build(F, seed, dev)
    zero_dropout(m)
    m.train()
    m.keep_workspace = True
    fp, img, y = synth_inputs(512512, B, F, 49152)
    p = oracle_params(m)                                 # before the forward call updates the BatchNorm running statistics
    old_w, old_o = L.bbbp_get_conv_winograd(), L.bbbp_set_overlap(1)
    _lib.check(L.bbbp_set_conv_winograd(conv_mask), "bbbp_set_conv_winograd")
    try:
        out = m(fp.to(dev), img.to(dev))
        gates = [g.cpu() for g in m.debug_ffn_gates()]
        masks = tuple(t.cpu() for t in m.debug_pool_masks())
        loss = bbbp_amd.MSELoss()(out.squeeze(), y.to(dev))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        L.bbbp_set_conv_winograd(old_w)
        L.bbbp_set_overlap(old_o)
    # the oracle's own decisions first: where do the GPU's differ?
    parts = {}
    with torch.no_grad():
        free_out = oracle.mixed_input_forward(p, fp.double(), img.double(), training=True, bn_state={}, parts=parts)
    flips = 0
    for l, (g, pre) in enumerate(zip(gates, parts["ffn_pre"])):
        diff = g.bool() != (pre > 0)
        flips += int(diff.sum())
        if diff.any():
            assert float(pre[diff].abs().max()) <= 2e-6 * float(pre.abs().mean()), f"layer {l}: ReLU decision differs away from zero"
    assert flips <= max_flips, f"{flips} ReLU decisions differ from float64"
    for stage, (mask, pre) in enumerate(zip(masks, parts["conv_pre"]), 1):
        own = oracle.pool_decisions(pre)
        diff = own != mask
        n_diff = int(diff.sum())
        assert n_diff <= 1e-4 * mask.numel(), f"conv stage {stage}: {n_diff} of {mask.numel()} pooling decisions differ from float64"
        if n_diff:
            win = oracle.pool_windows(pre)[diff]                                  # [n_diff, 4]
            want = win.max(dim=-1).values.clamp_min(0.0)                          # what ReLU + max-pool passes in float64
            gm = mask[diff].to(torch.int64)
            got = win.gather(-1, gm.clamp(max=3).unsqueeze(-1)).squeeze(-1).clamp_min(0.0) * (gm < 4)
            gap = float((want - got).abs().max())
            assert gap <= 1e-5 * float(pre.abs().mean()), f"conv stage {stage}: a pooling decision differs away from a tie (gap {gap:.3e})"
        del own, diff
    parts.clear()
    assert_close(out.detach().cpu().numpy(), free_out.numpy(), rtol=1e-4, atol_frac=2e-5, what=f"F={F} B=512 train output")
    # gradients of the function with those decisions
    st = {}
    ref_out = oracle.mixed_input_forward(p, fp.double(), img.double(), training=True, bn_state=st, ffn_gates=gates, pool_masks=masks)
    ref_loss = oracle.mse_loss(ref_out, y.double())
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-4 * abs(float(ref_loss.detach()))
    sd = m.state_dict()
    for k in ("fc.2.running_mean", "fc.2.running_var"):
        assert_close(sd[k].cpu().numpy(), st[k].numpy(), rtol=1e-4, what=k)
    checked = 0
    for k, q in m.named_parameters():
        if k.startswith(FUSION):
            continue
        assert_close(q.grad.cpu().numpy(), p[k].grad.numpy(), rtol=1e-4, atol_frac=5e-5, what=k)
        checked += 1
    return checked


@pytest.mark.parametrize("conv_mask", [252, 124, 3, 0], ids=["split-bf16-sparse-default", "split-bf16-dense-wgrad", "winograd", "direct"])
def test_headline_batch_fwd_bwd_against_oracle(dev, conv_mask):
    """BASELINE config 3 exactly as bench.py runs it: B = 512, F = 167, the library's DEFAULT conv mask 252 (conv2 forward / data
    gradient / weight gradient AND conv1's weight gradient in the split-bf16 form -- conv_b3_wgrad3_kernel at its B = 512 slab
    count; bit 6, conv1's split-bf16 forward, runs here too: beside a training step's encoder chain the engine takes its
    software-pipelined one-work-group-per-CU form, BBBP_C1_TRAIN's default), and the two all-float32 alternatives (Winograd on the
    192-CU partition, direct)."""
    assert _lib.lib().bbbp_get_conv_winograd() == 252, "the library default changed: run the B = 512 step under the new default too"
    assert check_b512_step_against_float64(dev, 167, 20250113, conv_mask) == 90


def test_morgan_2048_batch_512_every_gradient_against_oracle(dev):
    """BASELINE config 4 at its benchmarked shape: F = 2048 (nhead 256, head_dim 8: fused small-head attention; 160 M parameters;
    every encoder GEMM on the 128 x 128 split-bf16 plan, wide-row LayerNorm), B = 512, default conv forms -- every non-degenerate
    gradient tensor, element for element, at the tolerances of the F = 167 step."""
    assert check_b512_step_against_float64(dev, 2048, 7, 252) == 90


def test_screening_batch_4096_eval_and_screen(dev):
    """BASELINE config 5 at its stated size: eval-mode forward at B = 4096 (attention rows of 4096, the inference workspace)
    against the oracle, and ensemble.screen with batch_size = 4096 over 4096 + 40 molecules (network + random forest +
    precomputed column through the shipped linear meta-learner) against the column-wise reference."""
    ens = pytest.importorskip("sklearn.ensemble")
    from bbbp_amd.ensemble import StackedEnsemble, screen
    from bbbp_amd.trees import ForestGPU
    B, tail, F = 4096, 40, 167
    n = B + tail
    m = build(F, 20250113, dev).eval()
    fp, img, _ = synth_inputs(4096, n, F, 49152)
    p = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        got = m(fp[:B].to(dev), img[:B].to(dev)).cpu().numpy()
        want = np.concatenate([oracle.mixed_input_forward(p, fp[:B], img[:B], training=False).numpy(),
                               oracle.mixed_input_forward(p, fp[B:], img[B:], training=False).numpy()])
    assert_close(got, want[:B], rtol=1e-4, atol_frac=2e-5, what="B=4096 eval")
    rs = np.random.RandomState(5)
    feats = np.hstack([fp.numpy(), img.numpy()])
    rf = ens.RandomForestRegressor(n_estimators=6, max_depth=5, max_features=64, random_state=42).fit(feats[:96], rs.randn(96))
    xgb_col = rs.randn(n)
    stack = StackedEnsemble.from_coefficients([0.19813994153864287, 0.8730076113813537, 0.16470120078934247], 0.019492486407121146)
    out = screen(m, ForestGPU.from_sklearn(rf, device=dev), stack, fp.to(dev), img.to(dev), extra_columns=(xgb_col,), batch_size=B)
    ref = stack.predict(np.stack([want.reshape(-1).astype(np.float64), rf.predict(feats), xgb_col], axis=1))
    # the network column carries the 1e-4 tolerance; the forest and the stack arithmetic are exact to float64 rounding
    scale = float(np.abs(ref).max())
    assert np.abs(out.cpu().numpy() - ref).max() <= 0.2 * (1e-4 * scale + 2e-5 * float(np.abs(want).max())) + 1e-9


def test_hip_adamw_follows_the_reference_trajectory(dev):
    """The reference's own three AdamW steps (torch.optim.AdamW(lr 1e-4, wd 1e-5) on the reference class, B = 7, goldens
    adamw/B7/step{1,3} of tests/golden/flagship_f167.npz) with the HIP forward/backward and the fused bbbp_adamw_step:
    losses, parameters after steps 1 and 3, BatchNorm running statistics -- same bands as the CPU oracle is held to."""
    from bbbp_amd.optim import AdamW
    from test_oracle_golden import adam_noise_amplified
    g = golden("flagship_f167")
    B, F = 7, 167
    m = build(F, 20250113, dev)
    zero_dropout(m)
    m.train()
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=1e-5)
    fp, img, y = (t.to(dev) for t in synth_inputs(1000 + B, B, F, 49152))
    for step in range(1, 4):
        opt.zero_grad(set_to_none=True)
        loss = bbbp_amd.MSELoss()(m(fp, img).squeeze(), y)
        loss.backward()
        opt.step()
        want = float(g[f"adamw/B{B}/step{step}/loss"])
        assert abs(float(loss.detach()) - want) <= (1e-4 if step == 1 else 3e-3) * abs(want), (step, float(loss.detach()), want)
        if step in (1, 3):
            for k, q in m.named_parameters():
                if not adam_noise_amplified(k):
                    check_summary_adam(g, f"adamw/B{B}/step{step}/{k}", q, lr=1e-4, steps=step,
                                       tight_lr_frac=0.02 if step == 1 else 0.6, min_frac=0.9 if step == 1 else 0.75)
            sd = m.state_dict()
            # step 3: measured yardstick (round 4, CPU): the float32 ORACLE itself sits 2.4e-3 (absolute, at a scale of 0.49) from the reference's
            # float32 golden on running_mean after three AdamW steps, its half-ulp-perturbed variants 2.4 .. 3.1e-3 (the float64 oracle 6e-5:
            # three steps of sign-normalised updates amplify float32 rounding) -- the band is twice the worst of those
            for k in ("fc.2.running_mean", "fc.2.running_var"):
                assert_close(sd[k].cpu().numpy(), g[f"adamw/B{B}/step{step}/bn/{k}"], rtol=2e-4 if step == 1 else 5e-3,
                             atol_frac=2e-4 if step == 1 else 1.3e-2, what=k)
    assert opt.state[next(iter(m.parameters()))]["step"] == 3
