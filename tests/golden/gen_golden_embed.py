#!/usr/bin/env python3
"""Generate tests/golden/g22_embed_*.npz by RUNNING THE REFERENCE: its `SHEncoder` and `FourierFeature` view embedders
(model/network/embedder.py) alone, and `RenderingNetwork(..., embed_type=...)` with them in 'nerf' and 'idr' mode.  Needs the reference next
to this checkout (tests/golden/ref_import.py); only data is written.

    python tests/golden/gen_golden_embed.py

  g22_embed_rows           E(v) on 256 unit directions (the six axis directions first): spherical harmonics of degree 1..5 (`sh<d>`) and
                           Fourier features with 1, 5 and 12 channels, sigma 1 (`ff<c>`, their matrices as `B.ff<c>`) -- the reference's
                           fp32 results and, as `<tag>.f64`, the same modules on the fp64 directions (B as it is, widened)
  g22_embed_<mode>_<kind>  plumbing-size radiance net alone on 64 points (nerf: sh4, sh5, ff12; idr: sh4, ff5): state_dict (with the buffer
                           B), inputs, output, and the autograd gradients of sum(rgb * rgb_bar) with respect to every parameter, the
                           features and (idr) the normals -- the layout of g21_hdr_<mode>_<act>
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import gen_golden as G  # noqa: E402

torch.set_num_threads(4)
NETS = [("nerf", "sh4"), ("nerf", "sh5"), ("nerf", "ff12"), ("idr", "sh4"), ("idr", "ff5")]


def embed_kwargs(tag):
    return dict(embed_type="spherical_harmonics", degree=int(tag[2:])) if tag.startswith("sh") else \
        dict(embed_type="fourier", channels=int(tag[2:]), sigma=1.0)


def main():
    ref_import.import_reference()
    from model.network.embedder import get_embedder
    from model.network.mlp import RenderingNetwork

    g = torch.Generator().manual_seed(2222)
    axes = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    dirs64 = torch.cat([axes.double(), torch.nn.functional.normalize(torch.randn(250, 3, generator=g, dtype=torch.float64), dim=1)])
    dirs = dirs64.float()
    rows = dict(dirs=dirs)
    for tag in ["sh1", "sh2", "sh3", "sh4", "sh5", "ff1", "ff5", "ff12"]:
        torch.manual_seed(100 + int(tag[2:]))
        kw = embed_kwargs(tag)
        fn, width = get_embedder(kw.pop("embed_type"), input_dims=3, **kw)
        with torch.no_grad():
            rows[tag] = fn(dirs)
            assert rows[tag].shape == (256, width)
            if tag.startswith("ff"):
                rows["B." + tag] = fn.B.clone()
                fn = fn.double()
            rows[tag + ".f64"] = fn(dirs.double())
    G.save("g22_embed_rows", **rows)

    M = 64
    pts = (torch.rand(M, 3, generator=g) * 2 - 1) * 1.5
    nrm = torch.randn(M, 3, generator=g) * 0.8
    view = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    feat = torch.randn(M, 64, generator=g) * 0.5
    w = torch.randn(M, 3, generator=g)
    for mode, tag in NETS:
        torch.manual_seed(0)
        cfg = dict(G.small_conf().rendering_network)
        cfg.pop("multires")                      # (beside these embedders the reference raises a TypeError on it)
        cfg.update(embed_kwargs(tag))
        cfg.update(mode=mode, d_in=9 if mode == "idr" else 3)
        rnet = RenderingNetwork(64, **cfg)
        G.perturb_(rnet)
        f_, n_ = feat.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
        rgb = rnet(pts, n_, view, f_)
        rnet.zero_grad()
        (rgb * w).sum().backward()
        arrs = dict(view_dirs=view, feat=feat, rgb_bar=w, rgb=rgb, fbar=f_.grad)
        if mode == "idr":
            arrs.update(points=pts, normals=nrm, nbar=n_.grad)
        arrs.update(G.sd_arrays(rnet, "sd.rendering_network."))
        arrs.update({"grad.rendering_network." + n: p.grad for n, p in rnet.named_parameters()})
        G.save(f"g22_embed_{mode}_{tag}", **arrs)


if __name__ == "__main__":
    main()
