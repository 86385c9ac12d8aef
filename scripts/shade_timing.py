#!/usr/bin/env python3
"""Time the shading layer (i2sdf_amd.RenderingLayer: csrc/shade.hip) forward + backward on one GPU against the eager torch restatement of the
same arithmetic (tests/shade_ref.py, fp32, on the same GPU), same process.  Prints one JSON line and writes it to `--out`.

    python scripts/shade_timing.py [--windows 7] [--out profiles/shade_timing.json]

The model is the closed-form stand-in (tests/shade_ref.py: standin_radiance), evaluated under no_grad in both routes, so only the layer's own
arithmetic is timed.  Sizes (points x spp) 4096 x 64 and 1024 x 256: arbitrary, the reference ships no material configuration to take them
from.  A window is `calls` forward + backward passes between two HIP events after a warm-up; the two routes alternate; median / min / max and
every window are recorded, and torch.cuda.max_memory_allocated above the inputs for one pass of each route.  One further figure, not a
comparison: the layer at 64 x 8 with the real I2SDFNetwork.get_incident_radiance of the synthetic.yml net as the model, next to the same
layer call with the stand-in -- the secondary-ray render is bn spp rays through the whole volume renderer and is where the stage's time goes.
No ratio is promised and there is no threshold: the figures are a record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from view_embed_timing import alternate  # noqa: E402  (scripts/ is sys.path[0])


def inputs(bn, spp, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.rand(*s, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(bn, 3, generator=g), dim=1)
    view = torch.nn.functional.normalize(nrm + 0.7 * torch.randn(bn, 3, generator=g), dim=1)
    d = dict(surface_points=R(bn, 3) * 2 - 1, view_direction=view, normal=nrm, Kd=R(bn, 3), Ks=(R(bn, 3) * 0.6).clamp_min(0.04),
             rough=R(bn, 1).clamp_min(0.05), radiance_scale=torch.tensor([1.5, 0.7, 1.1]), samples=R(bn, spp, 3),
             w_diffuse=torch.randn(bn, 3, generator=g), w_spec=torch.randn(bn, 3, generator=g))
    return {k: v.to(dev) for k, v in d.items()}


def routes_for(bn, spp, dev, calls):
    import shade_ref as SR
    from i2sdf_amd import RenderingLayer
    d = inputs(bn, spp, dev)
    layer = RenderingLayer(spp, 1 << 30)
    model = SR.StandinModel(graph=False)
    leaves = [d[k].requires_grad_(True) for k in ("Kd", "Ks", "rough", "radiance_scale")]

    def clear():
        for t in leaves:
            t.grad = None

    def hip():
        clear()
        cd, cs, _ = layer(model, d["surface_points"], d["view_direction"], d["Kd"], d["Ks"], d["normal"], d["rough"], d["radiance_scale"],
                          samples=d["samples"])
        ((cd * d["w_diffuse"]).sum() + (cs * d["w_spec"]).sum()).backward()

    def eager():
        clear()
        o = SR.shade(model, d["surface_points"], d["view_direction"], d["Kd"], d["Ks"], d["normal"], d["rough"], d["radiance_scale"], d["samples"])
        ((o["colorDiffuse"] * d["w_diffuse"]).sum() + (o["colorSpec"] * d["w_spec"]).sum()).backward()

    peak = {}
    for name, fn in (("hip", hip), ("eager_torch", eager)):
        fn()
        clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
    res = alternate([("hip", hip, calls), ("eager_torch", eager, calls)], ARGS.windows)
    res["eager_over_hip_median"] = round(res["eager_torch"]["median_ms"] / res["hip"]["median_ms"], 2)
    res["peak_bytes_above_inputs"] = peak
    return res


def end_to_end(dev):
    import shade_ref as SR
    from i2sdf_amd import RenderingLayer, I2SDFNetwork, synthetic_conf
    torch.manual_seed(0)
    net = I2SDFNetwork(synthetic_conf()).to(dev).eval()
    bn, spp = 64, 8
    d = inputs(bn, spp, dev, seed=2)
    d["surface_points"] = d["surface_points"] * 0.5
    layer = RenderingLayer(spp, 1 << 30)
    leaves = [d[k].requires_grad_(True) for k in ("Kd", "Ks", "rough")]

    def run(model):
        def fn():
            for t in leaves:
                t.grad = None
            cd, cs, _ = layer(model, d["surface_points"], d["view_direction"], d["Kd"], d["Ks"], d["normal"], d["rough"], samples=d["samples"])
            (cd.sum() + cs.sum()).backward()
        return fn

    res = alternate([("real_get_incident_radiance", run(net), 3), ("standin_model", run(SR.StandinModel(graph=False)), 3)], ARGS.windows)
    res["rays"] = bn * spp
    return res


def main():
    global ARGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls", type=int, default=10, help="forward + backward passes per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_timing.json"), help="also write the JSON line here ('' to skip)")
    ARGS = ap.parse_args()
    if ARGS.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("shade_timing.py needs a GPU: nothing is timed on the host")
    dev = torch.device("cuda")
    res = {"device_name": torch.cuda.get_device_name(), "windows": ARGS.windows,
           "clock": "HIP events around a window of forward + backward passes, ms per pass; median / min / max and every window; the routes alternate",
           "sizes_are_arbitrary": "the reference ships no material configuration", "model": "closed-form stand-in under no_grad in both routes"}
    for bn, spp in ((4096, 64), (1024, 256)):
        res[f"{bn}x{spp}"] = routes_for(bn, spp, dev, ARGS.calls)
    res["end_to_end_64x8_synthetic_net"] = end_to_end(dev)
    line = json.dumps(res)
    print(line)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
