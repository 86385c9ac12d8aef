#!/usr/bin/env python3
"""Digests of what the MLP entry points compute on paths the headline benchmark does not run: one forward and backward through
`RenderEngine` per configuration, fixed parameters and inputs, `name sha256` per output and for the flat gradient.

    I2SDF_LIB_PATH=/path/to/libi2sdf_hip.so python scripts/entry_digests.py > digests.txt

Meant for comparing two builds of the library whose kernels should be the same (a host-side refactor): run it once per library, each run
in a fresh process, and diff the outputs.  Reads nothing outside the repository; a few seconds on one GPU.  Workspaces are zero-filled, so
the padding rows the kernels may leave alone are the same in every run; the entry points run outside a chain (the headline benchmark
covers the chained step).

Configurations: the 64-wide nets ('nerf', 'idr') at 200 points; the 256-wide net in split arithmetic with point ranges off / 2 at
2 * 2048 + 200 points and with ranges off at n_cu * 128 + 3 * 128 - 5 points (a split-K tail), each with two- and three-plane weight
gradients; the 256-wide net without split arithmetic; the radiance modes ('idr' with PE4 and without encoding, spherical harmonics of
degree 4 and Fourier features with 12 channels in both modes); the light head; sphere tracing, stepwise and fused, 256 rays and 8 steps on
both widths; one eval sampler pass of 128 rays with force_iters = 1."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

EMBEDS = {"pe4": {"embed_type": "positional", "multires": 4}, "none": {}, "sh4": {"embed_type": "spherical_harmonics", "degree": 4},
          "ff12": {"embed_type": "fourier", "channels": 12, "sigma": 1.0}}


def conf_of(wide=True, mode="nerf", embed="pe4", light=False, bf16x3=True):
    from i2sdf_amd import synthetic_conf, plumbing_conf
    conf = synthetic_conf(light) if wide else plumbing_conf(True, light)
    r = {k: v for k, v in conf["rendering_network"].items() if k not in ("embed_type", "multires")}
    r.update(EMBEDS[embed])
    if mode == "idr":
        r.update(mode="idr", d_in=9)
    conf["rendering_network"] = r
    conf["bf16x3"] = bf16x3
    return conf


def show(name, t):
    print(name, hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest(), flush=True)


def engine(conf, dev, parts=None, x2=None):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.engine import RenderEngine
    eng = RenderEngine(NetConfig.from_conf(conf), dev)
    eng._ws = lambda *shape, device=None: torch.zeros(*shape, dtype=torch.float32, device=device)
    if parts is not None:
        eng.set_parts(parts)
    if x2 is not None:
        eng.set_wgrad_bf16x2(x2)
    buffers = {}
    flat = eng.layout.init_flat(torch.Generator().manual_seed(3), buffers).to(dev)
    flat += 0.01 * torch.randn(flat.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    eng.pack(flat)
    for B in buffers.values():
        eng.set_view_embed(B)
    return eng, flat


def step(name, conf, M, dev, parts=None, x2=None):
    """sdf forward + d sdf/dx, radiance (and light) forward on the leading ray samples, fixed upstream gradients, every backward, weight grads"""
    eng, flat = engine(conf, dev, parts, x2)
    n = 8
    B = (3 * M // 4) // n
    Mm = B * n
    g = torch.Generator().manual_seed(1)
    cam = (torch.randn(B, 3, generator=g) * 0.2).to(dev)
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(dev)
    z = torch.sort(torch.rand(B, n + 1, generator=g) * 3.0, -1)[0].to(dev)
    pts = (torch.rand(M - Mm, 3, generator=g) * 2 - 1).to(dev)
    rgb_bar = torch.randn(Mm, 3, generator=g).to(dev)
    sbar, nbar_in, lm_bar = torch.randn(M, generator=g).to(dev), torch.randn(M, 3, generator=g).to(dev), torch.randn(Mm, generator=g).to(dev)
    grad_flat = torch.zeros_like(flat)
    # every entry point on its own (no chain: each forks and joins its point ranges, so the zero-filled workspaces are ordered before it)
    fw = eng.sdf_forward_grad(points=pts, rays=(cam, dirs, z, n), want_grad=True, save=True)
    rgb, rs, pev = eng.rgb_forward(dirs, n, fw["feat"], Mm, save=True, fw=fw)
    nbar = nbar_in.clone()
    gar, ga_last, fbar = eng.rgb_backward(rgb, rgb_bar, rs, Mm, nbar=nbar)
    light = None
    if eng.cfg.light is not None:
        lm, hl = eng.light_forward(fw["feat"], Mm)
        gal0, gal_last = eng.light_backward(lm, lm_bar, hl, Mm)
        light = {"hl": hl, "gal0": gal0, "gal_last": gal_last}
        show(name + ".lm", lm)
    bw = eng.sdf_backward(fw, sbar=sbar, fbar=fbar, m_fbar=Mm, nbar=nbar)
    eng.weight_grads(flat, grad_flat, fw, bw, M_main=Mm, fbar=fbar, rgb_fw={"pev": pev, "rs": rs}, rgb_bw={"gar": gar, "ga_last": ga_last},
                     light=light)
    torch.cuda.synchronize()
    for k, t in (("sdf", fw["sdf"]), ("grad", fw["grad"]), ("feat", fw["feat"][:M]), ("rgb", rgb), ("fbar", fbar[:Mm]), ("nbar", nbar),
                 ("grad_flat", grad_flat)):
        show(f"{name}.{k}", t)


def main():
    if not torch.cuda.is_available():
        sys.exit("entry_digests.py needs a GPU")
    dev = torch.device("cuda")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    M1, M_tail = 2 * 2048 + 200, n_cu * 128 + 3 * 128 - 5
    for mode in ("nerf", "idr"):
        step(f"w64.{mode}", conf_of(False, mode), 200, dev)
    for x2 in (False, True):
        for parts, M in ((0, M1), (2, M1), (0, M_tail)):
            step(f"w256.x3.parts{parts}.M{'tail' if M == M_tail else '1'}.wgrad{'x2' if x2 else 'x3'}", conf_of(), M, dev, parts, x2)
    step("w256.fp32", conf_of(bf16x3=False), M1, dev)
    for mode, embed in (("idr", "pe4"), ("idr", "none"), ("nerf", "sh4"), ("idr", "sh4"), ("nerf", "ff12"), ("idr", "ff12")):
        step(f"w256.{mode}.{embed}", conf_of(True, mode, embed), M1, dev)
    step("w256.light", conf_of(light=True), M1, dev)
    step("w64.light", conf_of(False, light=True), 200, dev)

    g = torch.Generator().manual_seed(7)
    cam = (torch.randn(256, 3, generator=g) * 0.2).to(dev)
    dirs = torch.nn.functional.normalize(torch.randn(256, 3, generator=g), dim=1).to(dev)
    for wide in (True, False):
        eng, flat = engine(conf_of(wide), dev)
        for route in ("stepwise", "fused"):
            r = eng.trace_rays(cam, dirs, eps=1e-4, max_steps=8, route=route, return_f=True)
            torch.cuda.synchronize()
            for k, t in (("t", r.t), ("status", r.status), ("steps", r.steps), ("f_trace", torch.nan_to_num(r.f_trace, nan=-7.0))):
                show(f"trace.w{256 if wide else 64}.{route}.{k}", t)
        z_all, z_eik, iters = eng.sample_rays(flat, cam[:128], dirs[:128], training=False, force_iters=1)
        torch.cuda.synchronize()
        show(f"sampler.w{256 if wide else 64}.z", z_all)
        show(f"sampler.w{256 if wide else 64}.iters", iters)


if __name__ == "__main__":
    main()
