#!/usr/bin/env python3
"""Generate tests/golden/g17_idr_*.npz by RUNNING THE REFERENCE with `rendering_network.mode: idr`, `d_in: 9` (the two-line switch
config/synthetic.yml documents).  Needs the reference next to this checkout (tests/golden/ref_import.py); only data is written.

    python tests/golden/gen_golden_idr.py

  g17_idr_rgb         plumbing-size radiance net alone: forward and every parameter gradient, d/d feature, d/d normals on 256 points
  g17_idr_eval        plumbing-size net, eval forward of a 32 x 32 view (the reference's own depths recorded).  The camera stands inside
                      the scene, as the data set's do; on this view the reference's own arithmetic is well conditioned WITH the sampler in the
                      loop: tests/idr_ref.py in fp64 and in fp32 with weight noise of 1e-6, each with its own sampler, stay within 4e-5 of
                      the recorded render (stored as ref_spread.*, asserted < 5e-5 here), so a 1e-4 check of a render that samples its own
                      depths asks for arithmetic, not for the luck of a depth pick.  (From (0, 0.2, -1.8) at beta 0.05 the same runs are 4e-4
                      to 2e-3 apart.)
  g17_idr_train       plumbing-size net, one training step with captured draws: outputs, loss, every parameter gradient
  g17_idr_train_full  the synthetic.yml net (256 wide), one training step; weights rebuilt by tests/idr_ref.init_params (checksummed),
                      gradients as the strided digest of gen_golden.grad_digest
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import gen_golden as G  # noqa: E402

torch.set_num_threads(4)


def idr_(cfg):
    cfg.rendering_network.mode = "idr"
    cfg.rendering_network.d_in = 9
    return cfg


def train_case(full, B, cam_t, W, H, f, seed, g):
    inp = G.camera_batch(B, cam_t, W=W, H=H, f=f, seed=seed)
    gt = {"rgb": torch.rand(B, 3, generator=g), "depth": torch.rand(B, generator=g) * 3, "depth_mask": torch.rand(B, generator=g) > 0.2,
          "normal": torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1), "normal_mask": torch.rand(B, generator=g) > 0.1}
    lkw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05)
    from model.network import I2SDFLoss
    np.random.seed(0)
    zrec = G.record_z(full)
    with G.DrawRecorder() as rec:
        out = full(inp)
    losses = I2SDFLoss(**lkw)(out, gt, 10)
    full.zero_grad()
    losses["loss"].backward()
    kinds = [k for k, _ in rec.log]
    assert kinds == ["rand", "rand", "randperm", "randint", "uniform", "uniform"], kinds
    arrs = {"in." + k: v for k, v in inp.items()}
    arrs.update({"gt." + k: v for k, v in gt.items()})
    arrs.update({"out." + k: v for k, v in out.items()})
    arrs.update({"loss." + k: v for k, v in losses.items()})
    n_extra = full.ray_sampler.N_samples_extra
    arrs.update({"draw.strat_u": rec.log[0][1], "draw.cdf_u": rec.log[1][1], "draw.extra_idx": rec.log[2][1][:n_extra],
                 "draw.eik_idx": rec.log[3][1], "draw.eik_pts": rec.log[4][1], "draw.nbr_off": rec.log[5][1]})
    arrs["loss_kwargs"] = np.array(sorted(lkw.items(), key=lambda kv: kv[0]), dtype=object).astype(str)
    arrs["ref.z_vals"], arrs["ref.z_eik"] = zrec[0]
    grads = [(n, p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in full.named_parameters()]
    return arrs, grads


def main():
    ref_model, _ = ref_import.import_reference()
    from model.network.mlp import RenderingNetwork
    import idr_ref
    from oracle import i2sdf_oracle as orc
    g = torch.Generator().manual_seed(1717)

    # ---- the radiance net alone, plumbing size
    torch.manual_seed(0)
    cfg = idr_(G.small_conf())
    rnet = RenderingNetwork(64, **cfg.rendering_network)
    G.perturb_(rnet)
    M = 256
    pts = (torch.rand(M, 3, generator=g) * 2 - 1) * 1.5
    nrm = torch.randn(M, 3, generator=g) * 0.8
    view = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    feat = torch.randn(M, 64, generator=g) * 0.5
    w = torch.randn(M, 3, generator=g)
    f_, n_ = feat.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
    rgb = rnet(pts, n_, view, f_)
    rnet.zero_grad()
    (rgb * w).sum().backward()
    arrs = dict(points=pts, normals=nrm, view_dirs=view, feat=feat, rgb_bar=w, rgb=rgb, fbar=f_.grad, nbar=n_.grad)
    arrs.update(G.sd_arrays(rnet, "sd.rendering_network."))
    arrs.update({"grad.rendering_network." + n: p.grad for n, p in rnet.named_parameters()})
    G.save("g17_idr_rgb", **arrs)

    # ---- eval forward, 32 x 32 view
    torch.manual_seed(0)
    full = ref_model.I2SDFNetwork(idr_(G.small_conf(skip=True)))
    G.perturb_(full)
    full.eval()
    with torch.no_grad():
        full.density.beta.fill_(0.1)
    inp = G.camera_batch(1024, (0.1, -0.2, 0.3), train_layout=False)
    zrec = G.record_z(full)
    out = full(inp)
    arrs = {"in." + k: v for k, v in inp.items()}
    arrs.update({"out." + k: v for k, v in out.items()})
    arrs.update(G.sd_arrays(full))
    arrs["ref.z_vals"], arrs["ref.z_eik"] = zrec[0]
    # the conditioning of this view with the sampler in the loop, measured with the restatement only
    from helpers import perturbed_weights, rel_max
    ocfg = orc.plumbing_cfg(skip=True)
    sd = {k: v.detach().clone() for k, v in full.state_dict().items()}
    runs = [idr_ref.network_forward({k: v.double() for k, v in sd.items()}, ocfg, {k: v.double() for k, v in inp.items()}, False)]
    runs += [idr_ref.network_forward(perturbed_weights(sd, rel=1e-6, seed=100 + i), ocfg, inp, False) for i in range(3)]
    for k in ("rgb_values", "depth_values", "weight_sum"):
        arrs["ref_spread." + k] = np.float64(max(rel_max(r[k].detach().float(), out[k].detach()) for r in runs))
        assert arrs["ref_spread." + k] < 5e-5, (k, arrs["ref_spread." + k])
    G.save("g17_idr_eval", **arrs)

    # ---- one training step, plumbing size, captured draws (use_normal on: both sources of d loss / d normal add)
    torch.manual_seed(0)
    full = ref_model.I2SDFNetwork(idr_(G.small_conf(skip=True)))
    G.perturb_(full)
    full.train()
    with torch.no_grad():
        full.density.beta.fill_(0.05)
    sd = {k: v.detach().clone() for k, v in full.state_dict().items()}
    arrs, grads = train_case(full, 64, (0.0, 0.2, -1.8), 32, 32, 30.0, 3, g)
    arrs.update({"sd." + k: v for k, v in sd.items()})
    arrs.update({"grad." + n: v for n, v in grads})
    G.save("g17_idr_train", **arrs)

    # ---- one training step, synthetic.yml size: weights rebuilt on both sides, gradient digest
    ocfg = orc.synthetic_cfg(False)
    sd = orc.perturb_params(idr_ref.init_params(ocfg, seed=171), 0.03, seed=172)
    sd["density.beta"] = torch.tensor(0.05)
    cfg = idr_(ref_import.load_cfg("synthetic.yml").model)
    cfg.use_normal = True
    full = ref_model.I2SDFNetwork(cfg)
    full.load_state_dict(sd)
    full.train()
    torch.manual_seed(1)
    arrs, grads = train_case(full, 16, (0.0, 0.0, -2.0), 640, 480, 600.0, 14, g)
    arrs.update(G.grad_digest(grads))
    arrs["init_seed"], arrs["perturb_seed"], arrs["perturb_scale"], arrs["grad_stride"] = np.int64(171), np.int64(172), np.float32(0.03), np.int64(61)
    arrs["sd_checksum"] = torch.stack([v.double().sum() for v in sd.values()])
    G.save("g17_idr_train_full", **arrs)


if __name__ == "__main__":
    main()
