"""GPU: PSNR / loss-curve parity over a short training run (SURVEY 8d "PSNR parity").

Both paths start from identical weights and consume identical batches and identical random draws each step:
  * oracle : fp32 CPU restatement, torch.autograd backward, torch.optim.Adam(eps=1e-15) (model/trainer/recon.py:203)
  * HIP    : I2SDFNetwork + I2SDFLoss + the same optimizer class on the drop-in module's parameters
The sampler runs inside the loop on both sides (each with its own convergence decisions).  Bars: PSNR of the rendered
batch against its target within 0.1 dB at every step (the bar SURVEY 8d names) and the total loss within 1e-2 relative.
The trajectories are not expected to agree to 1e-4: Adam with eps=1e-15 turns fp32 rounding noise in near-zero gradient
entries into +-lr steps, and the eikonal / smooth terms are evaluated at sampler-chosen depths (ill-conditioned in the
reference itself, see test_gpu_sampler.py); the per-step 1e-4 checks with identical state are in test_gpu_network.py.
The trained weights are compared entry-wise in units of the learning rate.
"""
import pytest
import torch

from oracle import i2sdf_oracle as orc
from helpers import camera_inputs, make_draws, make_gt, rel_max
from test_gpu_network import build, cuda

pytestmark = pytest.mark.gpu

STEPS, B, LR = 24, 48, 2e-3


def _draws_dict(dr):
    return {k: getattr(dr, k).cuda() for k in ("strat_u", "cdf_u", "extra_idx", "eik_idx", "eik_pts", "nbr_off")}


@pytest.mark.parametrize("light", [False, True])
def test_training_curves_match_oracle(light):
    from i2sdf_amd import plumbing_conf, I2SDFLoss
    ocfg = orc.plumbing_cfg(skip=True, light=light)
    ocfg.use_normal = True
    sd = orc.init_params(ocfg, seed=3)
    sd["density.beta"] = torch.tensor(0.05)
    lkw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=8, depth_weight=0.1, normal_weight=0.05,
               light_mask_weight=0.5 if light else 0.0)                       # smooth term switches on at step 8
    lc = orc.LossCfg(**lkw)
    n_row = ocfg.sampler.N_samples_eval + ocfg.sampler.N_samples

    # --- oracle run (does not depend on the weight-gradient mode of the library: computed once, tests/helpers.py: memo) -----------
    def oracle_run():
        leaves = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
        opt_o = torch.optim.Adam(list(leaves.values()), lr=LR, eps=1e-15)
        psnr_o, loss_o = [], []
        for step in range(STEPS):
            inp = camera_inputs(B, (0.0, 0.0, -2.0), W=32, H=32, f=30.0, seed=100 + step)
            gt = make_gt(B, seed=step, light=light)
            dr = make_draws(ocfg, B, n_row=n_row, seed=1000 + step)
            cur = {k: p.detach() for k, p in leaves.items()}
            out, losses, grads = orc.training_step_grads(cur, ocfg, inp, gt, lc, dr, step=step)
            psnr_o.append(float(orc.get_psnr(out["rgb_values"].detach(), gt["rgb"])))
            loss_o.append(float(losses["loss"].detach()))
            opt_o.zero_grad()
            for k, p in leaves.items():
                p.grad = grads[k].reshape(p.shape).clone()
            opt_o.step()
        return psnr_o, loss_o, {k: p.detach().clone() for k, p in leaves.items()}

    from helpers import memo
    psnr_o, loss_o, leaves = memo(("24-step oracle run", light), oracle_run)

    # --- HIP run ------------------------------------------------------------------------------
    net = build(plumbing_conf(skip=True, light=light), sd, train=True)
    loss_fn = I2SDFLoss(**lkw)
    opt_h = torch.optim.Adam(net.get_param_groups(LR), eps=1e-15)
    psnr_h, loss_h = [], []
    for step in range(STEPS):
        inp = camera_inputs(B, (0.0, 0.0, -2.0), W=32, H=32, f=30.0, seed=100 + step)
        gt = make_gt(B, seed=step, light=light)
        dr = make_draws(ocfg, B, n_row=n_row, seed=1000 + step)
        out = net(cuda(inp), draws=_draws_dict(dr))
        losses = loss_fn(out, cuda(gt), step)
        opt_h.zero_grad()
        losses["loss"].backward()
        opt_h.step()
        psnr_h.append(float(orc.get_psnr(out["rgb_values"].detach().cpu(), gt["rgb"])))
        loss_h.append(float(losses["loss"].detach()))

    dps = max(abs(a - b) for a, b in zip(psnr_o, psnr_h))
    dl = max(abs(a - b) / abs(a) for a, b in zip(loss_o, loss_h))
    print(f"PSNR oracle {psnr_o[0]:.3f} -> {psnr_o[-1]:.3f} dB, HIP {psnr_h[0]:.3f} -> {psnr_h[-1]:.3f} dB, max |dPSNR| {dps:.2e} dB, "
          f"max rel loss diff {dl:.2e}")
    assert abs(psnr_o[-1] - psnr_o[0]) > 0.05 or abs(loss_o[-1] - loss_o[0]) / loss_o[0] > 0.05, "the run must actually train"
    assert dps < 0.1, (psnr_o, psnr_h)
    assert dl < 1e-2, (loss_o, loss_h)
    got = net.state_dict()
    # weights: every entry moves by at most STEPS*LR.  Entries whose gradient is noise (ReLU units that fire for a handful of
    # samples, v-components along v) take +-LR Adam steps that differ between the runs -- measured: mean 0.2-0.3 LR per
    # tensor, max 7.5 LR on one such unit; well-conditioned tensors (e.g. rendering lin2.bias) agree to 1e-7.  Stale packed
    # weights or a wrong gradient give mean differences of several LR.
    # The mean is taken over tensors with at least 16 entries: the "mean" of a one-element tensor (light_network.lin1.weight_g) is that entry's
    # own difference, i.e. a max criterion in disguise -- it moved 0.21 -> 0.53 LR when round 6 changed the association of a wave-wide sum
    # (scripts/ab/parity_diag.py: every tensor with more than one entry stayed at 0.18-0.28 LR in all four builds / paths compared).
    worst_abs, worst_mean, small = 0.0, 0.0, []
    for k in leaves:
        d = (got[k].cpu().reshape(-1).double() - leaves[k].detach().reshape(-1).double()).abs()
        worst_abs = max(worst_abs, float(d.max()))
        if d.numel() >= 16:
            worst_mean = max(worst_mean, float(d.mean()))
        else:
            small.append(d)
    # the tensors with fewer than 16 entries (density.beta, the last radiance layer's bias / weight_g, the light head's last layer) pooled
    # into ONE mean, and beta -- whose gradient the fused path reduces in render_loss_finish_kernel -- bounded on its own against the oracle
    pooled_mean = float(torch.cat(small).mean())
    d_beta = float((got["density.beta"].cpu().double() - leaves["density.beta"].detach().double()).abs())
    print(f"trained weights: max |diff| {worst_abs:.2e}, worst per-tensor mean |diff| {worst_mean:.2e}, pooled mean |diff| of the "
          f"{sum(x.numel() for x in small)} entries of tensors < 16 entries {pooled_mean:.2e}, |d beta| {d_beta:.2e} (LR {LR}, {STEPS} steps)")
    # a single noise-dominated entry can differ by up to 2*STEPS*LR (opposite +-LR steps every step): only the mean is a criterion
    assert worst_abs <= 2 * STEPS * LR * 1.01 and worst_mean < 0.5 * LR
    # measured: pooled mean 0.006 LR (0.083 LR with the light head), |d beta| 0.0015 LR, in both weight-gradient modes; with beta's gradient
    # sign-flipped (monkeypatched) 2.1 LR and 13.7 LR
    assert pooled_mean < 0.5 * LR, pooled_mean
    assert d_beta < 0.05 * LR, d_beta
