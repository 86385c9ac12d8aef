#!/usr/bin/env python3
"""Time the sphere tracer (include/i2sdf.h: i2sdf_trace_rays; csrc/mlp_trace.hip) on one GPU, on the synthetic.yml net (geometric init).
Prints one JSON line and writes it to `--out`.

    python scripts/trace_timing.py [--windows 7] [--out profiles/trace_timing.json]

  routes           RenderEngine.trace_rays, route "fused" against route "stepwise", at 1024, 16 384 and 307 200 rays of one 640 x 480 view
                   (every k-th pixel for the smaller sizes), defaults otherwise (eps 1e-4, max_steps 64).  The route that is faster at
                   307 200 rays is what route "auto" should take (csrc/mlp_trace.hip: i2sdf_trace_rays).
  view             I2SDFNetwork.render_surface against I2SDFNetwork.render_image for that view.
  shading_64x8     i2sdf_amd.RenderingLayer at 64 points x 8 samples (512 secondary rays), forward + backward, with the module's volume-rendered
                   get_incident_radiance against the same call with intersect_func = net.sphere_tracer() (scripts/shade_timing.py measured the
                   former at 1.55 ms).
A window is `calls` calls between two HIP events after a warm-up; the routes of a comparison alternate; median / min / max and every window
are recorded.  No figure is promised and there is no threshold: the numbers are a record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from view_embed_timing import alternate  # noqa: E402  (scripts/ is sys.path[0])
from shade_timing import inputs as shade_inputs  # noqa: E402

H, W = 480, 640


def view_input(dev):
    from i2sdf_amd import views as V
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 600.0
    K[0, 2], K[1, 2] = W / 2, H / 2
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.2, -2.2])
    return {"uv": V.pixel_grid(H, W, dev), "pose": pose.unsqueeze(0).to(dev), "intrinsics": K.unsqueeze(0).to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("trace_timing.py needs a GPU: nothing is timed on the host")
    from i2sdf_amd import I2SDFNetwork, RenderingLayer, synthetic_conf
    from i2sdf_amd import trace as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = I2SDFNetwork(synthetic_conf()).to(dev).eval()
    eng = net._engine_for(dev)
    inp = view_input(dev)
    cam, dirs, _ = eng.ray_setup(inp["uv"], inp["pose"], inp["intrinsics"])
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows, "net": "synthetic.yml shapes, geometric init, seed 0",
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; the routes of a comparison alternate",
           "trace": "eps 1e-4, max_steps 64, step_scale 1, interval [near, 2 scene_bounding_sphere]"}
    routes = {}
    for n in (1024, 16384, H * W):
        k = (H * W) // n
        c, d = cam[::k][:n].contiguous(), dirs[::k][:n].contiguous()
        r = eng.trace_rays(c, d, route="stepwise")
        r2 = eng.trace_rays(c, d, route="fused")
        assert torch.equal(r.status, r2.status) and torch.equal(r.steps, r2.steps) and torch.equal(r.t, r2.t)
        calls = 20 if n <= 16384 else 3
        t = alternate([("fused", lambda: eng.trace_rays(c, d, route="fused"), calls), ("stepwise", lambda: eng.trace_rays(c, d, route="stepwise"), calls)],
                      args.windows)
        t["stepwise_over_fused_median"] = round(t["stepwise"]["median_ms"] / t["fused"]["median_ms"], 3)
        t["status_counts"] = {name: int((r.status == v).sum()) for name, v in (("hit", T.HIT), ("miss", T.MISS), ("unresolved", T.UNRESOLVED),
                                                                               ("inside", T.INSIDE))}
        t["mean_steps"] = round(float(r.steps.float().mean()), 2)
        t["max_steps_of_a_hit"] = int(r.steps[r.status == T.HIT].max()) if bool((r.status == T.HIT).any()) else 0
        routes[str(n)] = t
    res["routes"] = routes
    res["auto_should_be"] = "fused" if routes[str(H * W)]["fused"]["median_ms"] < routes[str(H * W)]["stepwise"]["median_ms"] else "stepwise"
    res["view_640x480"] = alternate([("render_surface", lambda: net.render_surface(inp), 1), ("render_image", lambda: net.render_image(inp), 1)],
                                    args.windows)
    res["view_640x480"]["render_image_over_render_surface_median"] = round(
        res["view_640x480"]["render_image"]["median_ms"] / res["view_640x480"]["render_surface"]["median_ms"], 2)
    # the 64 x 8 shading pass of scripts/shade_timing.py (end_to_end), with and without the tracer
    bn, spp = 64, 8
    sd = shade_inputs(bn, spp, dev, seed=2)
    sd["surface_points"] = sd["surface_points"] * 0.5
    layer = RenderingLayer(spp, 1 << 30)
    leaves = [sd[k].requires_grad_(True) for k in ("Kd", "Ks", "rough")]
    tracer = net.sphere_tracer()

    def shade(hook):
        def fn():
            for t_ in leaves:
                t_.grad = None
            cd, cs, _ = layer(net, sd["surface_points"], sd["view_direction"], sd["Kd"], sd["Ks"], sd["normal"], sd["rough"], intersect_func=hook,
                              samples=sd["samples"])
            (cd.sum() + cs.sum()).backward()
        return fn

    res["shading_64x8"] = alternate([("traced_incident_radiance", shade(tracer), 3), ("volume_rendered_incident_radiance", shade(None), 3)], args.windows)
    res["shading_64x8"]["rays"] = bn * spp
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
