#!/usr/bin/env python3
"""Generate tests/golden/g21_hdr_*.npz by RUNNING THE REFERENCE: `RenderingNetwork(..., output_activation=...)` for 'relu' and 'softplus'
in 'nerf' and 'idr' mode, and `utils.rend_util.linear_to_srgb`.  Needs the reference next to this checkout (tests/golden/ref_import.py);
only data is written.

    python tests/golden/gen_golden_hdr.py

  g21_hdr_<mode>_<act>  plumbing-size radiance net alone on 64 points: weights, inputs, output, and the autograd gradients of
                        sum(rgb * rgb_bar) with respect to every parameter, the features and (idr) the normals.  The last layer's
                        weight_g is scaled up (x 500) so that the outputs leave [0, 1]: some exceed 1, some pre-activations exceed 20 (softplus's
                        linear branch), some are negative (relu's zero branch).
  g21_hdr_tonemap       linear_to_srgb on a grid that holds 0, 0.0031308, its two fp32 neighbours, 1 and values outside [0, 1]: the fp32
                        grid, the reference's fp32 results without and behind clamp(0, 1), and the same from the fp64 grid
"""
import importlib
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


def main():
    ref_import.import_reference()
    from model.network.mlp import RenderingNetwork
    rend_util = importlib.import_module("utils.rend_util")
    g = torch.Generator().manual_seed(2121)
    M = 64
    pts = (torch.rand(M, 3, generator=g) * 2 - 1) * 1.5
    nrm = torch.randn(M, 3, generator=g) * 0.8
    view = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    feat = torch.randn(M, 64, generator=g) * 0.5
    w = torch.randn(M, 3, generator=g)
    for mode in ("nerf", "idr"):
        for act in ("relu", "softplus"):
            torch.manual_seed(0)
            cfg = G.small_conf()
            cfg.rendering_network.mode = mode
            cfg.rendering_network.d_in = 9 if mode == "idr" else 3
            rnet = RenderingNetwork(64, output_activation=act, **cfg.rendering_network)
            G.perturb_(rnet)
            with torch.no_grad():
                rnet.lin2.weight_g.mul_(500.0)
            f_, n_ = feat.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
            rgb = rnet(pts, n_, view, f_)
            rnet.zero_grad()
            (rgb * w).sum().backward()
            assert float(rgb.detach().max()) > 20.0 and float(rgb.detach().min()) < 0.5, (mode, act, float(rgb.detach().min()), float(rgb.detach().max()))
            arrs = dict(view_dirs=view, feat=feat, rgb_bar=w, rgb=rgb, fbar=f_.grad)
            if mode == "idr":
                arrs.update(points=pts, normals=nrm, nbar=n_.grad)
            arrs.update(G.sd_arrays(rnet, "sd.rendering_network."))
            arrs.update({"grad.rendering_network." + n: p.grad for n, p in rnet.named_parameters()})
            G.save(f"g21_hdr_{mode}_{act}", **arrs)

    thr = np.float32(0.0031308)
    special = [0.0, float(thr), float(np.nextafter(thr, np.float32(0))), float(np.nextafter(thr, np.float32(1))), 1.0,
               float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 1e-30, 1e-6, 0.5]
    outside = [-1e-3, -0.25, -3.0, 1.5, 8.0, 65504.0]
    grid = torch.tensor(special + outside + list(np.linspace(0.0, 1.0, 101)[1:-1]) + list(np.geomspace(1e-5, 0.9, 48)), dtype=torch.float32)
    g64 = grid.double()
    G.save("g21_hdr_tonemap", x=grid, srgb=rend_util.linear_to_srgb(grid), srgb_clamped=rend_util.linear_to_srgb(grid.clamp(0, 1)),
           srgb64=rend_util.linear_to_srgb(g64), srgb64_clamped=rend_util.linear_to_srgb(g64.clamp(0, 1)), n_special=np.int64(len(special)),
           n_outside=np.int64(len(outside)))


if __name__ == "__main__":
    main()
