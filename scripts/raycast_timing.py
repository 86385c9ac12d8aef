#!/usr/bin/env python3
"""Time the mesh ray caster (include/i2sdf.h: "Ray casting"; csrc/bvh.hip) on one GPU, on the synthetic.yml net (geometric init).
Prints one JSON line and writes it to `--out`.

    python scripts/raycast_timing.py [--windows 7] [--out profiles/raycast_timing.json]

  mesh             the zero level on a 640^3 grid over [-0.7, 0.7]^3 (about 2 M faces), extracted on the device.
  build            i2sdf_amd.build_bvh of that mesh: keys, torch.sort, topology, boxes.
  trace_640x480    i2sdf_amd.ray_mesh_intersect and i2sdf_amd.occluded of the 307 200 primary rays of one view against the tree.
  view_640x480     I2SDFNetwork.render_surface with intersect_func = net.mesh_tracer(bvh) against render_surface by sphere tracing.
  shading_64x8     i2sdf_amd.RenderingLayer at 64 points x 8 samples (512 secondary rays), forward + backward, three ways: incident radiance
                   through the mesh tracer, through the sphere tracer, and volume-rendered (scripts/trace_timing.py timed the latter two).
  small_mesh       512 rays against 256 faces, route "brute" against route "bvh": what route "auto" decides on a bare mesh.
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
from trace_timing import view_input  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--resolution", type=int, default=640, help="grid points per axis of the extracted mesh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("raycast_timing.py needs a GPU: nothing is timed on the host")
    import i2sdf_amd as A
    from i2sdf_amd import trace as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = A.I2SDFNetwork(A.synthetic_conf()).to(dev).eval()
    eng = net._engine_for(dev)
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows, "net": "synthetic.yml shapes, geometric init, seed 0",
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; the routes of a comparison alternate"}
    mesh = net.extract_mesh(A.uniform_axes(args.resolution, (-0.7, 0.7)))
    F = int(mesh.faces.shape[0])
    res["mesh"] = {"grid": f"{args.resolution}^3 over [-0.7, 0.7]^3", "faces": F, "verts": int(mesh.verts.shape[0]),
                   "bvh_bytes": int(A.build_bvh(mesh).buffer.numel())}
    res["build"] = alternate([("build_bvh", lambda: A.build_bvh(mesh), 3)], args.windows)
    bvh = A.build_bvh(mesh)
    inp = view_input(dev)
    cam, dirs, _ = eng.ray_setup(inp["uv"], inp["pose"], inp["intrinsics"])
    hits = A.ray_mesh_intersect(bvh, cam, dirs)
    res["trace_640x480"] = alternate([("closest_hit", lambda: A.ray_mesh_intersect(bvh, cam, dirs), 5),
                                      ("occluded", lambda: A.occluded(bvh, cam, dirs), 5)], args.windows)
    res["trace_640x480"].update(rays=int(cam.shape[0]), hits=int(hits.hit.sum()), status=int(hits.status.item()))
    tracer = net.mesh_tracer(bvh)
    sphere = net.render_surface(inp)
    on_mesh = net.render_surface(inp, intersect_func=tracer)
    both = sphere["hit"] & on_mesh["hit"]
    res["view_640x480"] = alternate([("render_surface_mesh_tracer", lambda: net.render_surface(inp, intersect_func=tracer), 1),
                                     ("render_surface_sphere_tracing", lambda: net.render_surface(inp), 1)], args.windows)
    res["view_640x480"].update(
        sphere_over_mesh_median=round(res["view_640x480"]["render_surface_sphere_tracing"]["median_ms"] /
                                      res["view_640x480"]["render_surface_mesh_tracer"]["median_ms"], 2),
        hits_sphere=int(sphere["hit"].sum()), hits_mesh=int(on_mesh["hit"].sum()), hits_both=int(both.sum()),
        max_abs_t_difference_on_both=float((sphere["t"][both] - on_mesh["t"][both]).abs().max()) if bool(both.any()) else None,
        max_abs_rgb_difference_on_both=float((sphere["rgb_values"][both] - on_mesh["rgb_values"][both]).abs().max()) if bool(both.any()) else None)
    # the 64 x 8 shading pass of scripts/shade_timing.py (end_to_end), as scripts/trace_timing.py runs it
    bn, spp = 64, 8
    sd = shade_inputs(bn, spp, dev, seed=2)
    sd["surface_points"] = sd["surface_points"] * 0.5
    layer = A.RenderingLayer(spp, 1 << 30)
    leaves = [sd[k].requires_grad_(True) for k in ("Kd", "Ks", "rough")]

    def shade(hook):
        def fn():
            for t_ in leaves:
                t_.grad = None
            cd, cs, _ = layer(net, sd["surface_points"], sd["view_direction"], sd["Kd"], sd["Ks"], sd["normal"], sd["rough"], intersect_func=hook,
                              samples=sd["samples"])
            (cd.sum() + cs.sum()).backward()
        return fn

    res["shading_64x8"] = alternate([("mesh_traced_incident_radiance", shade(tracer), 3),
                                     ("sphere_traced_incident_radiance", shade(net.sphere_tracer()), 3),
                                     ("volume_rendered_incident_radiance", shade(None), 3)], args.windows)
    res["shading_64x8"]["rays"] = bn * spp
    # a small mesh: one staged tile of faces per ray against a tree over them
    g = torch.Generator().manual_seed(4)
    centre = torch.rand(256, 1, 3, generator=g) * 2 - 1
    sv = (centre + 0.08 * torch.randn(256, 3, 3, generator=g)).reshape(-1, 3).to(dev)
    sf = torch.arange(768, dtype=torch.int32).reshape(256, 3).to(dev)
    so = (torch.rand(512, 3, generator=g) * 2 - 1).to(dev)
    sdir = torch.nn.functional.normalize(torch.randn(512, 3, generator=g), dim=1).to(dev)
    small = A.build_bvh((sv, sf))
    a, b = A.ray_mesh_intersect((sv, sf), so, sdir, route="brute"), A.ray_mesh_intersect(small, so, sdir)
    assert torch.equal(a.t, b.t) and torch.equal(a.face, b.face)
    res["small_mesh"] = alternate([("brute", lambda: A.ray_mesh_intersect((sv, sf), so, sdir, route="brute"), 20),
                                   ("bvh", lambda: A.ray_mesh_intersect(small, so, sdir), 20)], args.windows)
    res["small_mesh"].update(faces=256, rays=512, hits=int(a.hit.sum()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
