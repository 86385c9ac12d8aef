#!/usr/bin/env python3
"""Time mesh simplification by vertex clustering (include/i2sdf.h: "Mesh simplification"; csrc/simplify.hip) on one GPU, on the
synthetic.yml net (geometric init).  Prints one JSON line and writes it to `--out`.

    python scripts/simplify_timing.py [--windows 7] [--out profiles/simplify_timing.json]

  mesh             the zero level on a 384^3 grid over [-0.7, 0.7]^3, extracted on the device; `clean` of it; `topology` of both.
  h_2 / h_4 / h_8  simplify_vertex_clustering of the cleaned mesh at a cell of 2, 4 and 8 grid spacings:
    stages         per stage (keys + sorts, quadric reduce + solve, faces, compaction) the time between the front end's own HIP events and
                   the achieved bytes / s against the bytes the stage must move (every array it reads or writes counted once: `bytes`
                   below says which).  The front end reads two counts back on the way (the cells; the kept faces and vertices): the
                   stage that holds such a read includes the wait for it, and the script says which stages do.
    whole          the whole call, `quadric` against `average`, alternating.
    result         faces in and out, the fallback share, `topology` after.
    distance       the two-sided mean surface distance to the original (surface_scores: Acc pred -> original, Comp original -> pred,
                   2^18 samples each way) for `average` and for `quadric`.
    bvh_and_rays   build_bvh plus the 307 200 primary rays of one 640 x 480 view on the simplified mesh against the original.
  clean            the whole `clean` call and `topology` (enqueue + its one read) on the original.
A window is `calls` calls between two HIP events after a warm-up; the routes of a comparison alternate; median / min / max and every window
are recorded.  No figure is promised and there is no threshold: the numbers are a record.  Not timed: other meshes, `reg`, the C calls
one by one without the front end's reads."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from view_embed_timing import alternate, summary  # noqa: E402  (scripts/ is sys.path[0])
from trace_timing import view_input  # noqa: E402

STAGES = ("keys_sort", "reduce_solve", "faces", "compaction")


def stage_bytes(V, F, M, F_out, V_out, normals, quadric):
    """bytes every stage must move, each array it reads or writes counted once"""
    n = 12 if normals else 0
    keys = 2 * 12 * V + 8 * V + 24 * V + 12 * V + 8 * V + 24 * V + 4 * (M + 1)      # bounds, keys, sort, heads, scan, vertex cells
    reduce_ = V * (8 + 12 + n) + M * (8 + 12 + n + 1)                                # vertex runs in, the cell table out
    if quadric:
        keys += 12 * F + 12 * F + 12 * F + 12 * F + 36 * F + 12 * F + 8 * M           # corner keys (faces, cells, keys), sort, runs
        reduce_ += 3 * F * (8 + 12 + 36) + 8 * M                                      # per corner: its index, its face, three vertices
    faces = 12 * F + 12 * F + 12 * F + 16 * F + 2 * (8 * F + 16 * F) + 3 * 16 * F + 24 * F + F      # face keys, two sorts, gathers, heads
    compaction = 12 * F + F + 4 * F + 4 * M + 8 * F + 8 * M + 12 * F + 12 * F_out + 8 * M + V_out * (12 + n) * 2 + 4 * V + 4 * F_out
    return dict(keys_sort=keys, reduce_solve=reduce_, faces=faces, compaction=compaction)


def staged(A, mesh, h, contraction, windows):
    """per-stage times of `windows` calls from the front end's own events"""
    per = {s: [] for s in STAGES}
    for w in range(windows + 2):
        stats = []
        A.simplify_vertex_clustering(mesh, h, contraction, _stats=stats)
        torch.cuda.synchronize()
        ev = dict(stats)
        if w < 2:
            continue                                            # warm-up
        prev = ev["start"]
        for s in STAGES:
            per[s].append(prev.elapsed_time(ev[s]))
            prev = ev[s]
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--resolution", type=int, default=384, help="grid points per axis of the extracted mesh")
    ap.add_argument("--samples", type=int, default=1 << 18, help="surface samples each way for the distance")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("simplify_timing.py needs a GPU: nothing is timed on the host")
    import i2sdf_amd as A
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = A.I2SDFNetwork(A.synthetic_conf()).to(dev).eval()
    eng = net._engine_for(dev)
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows, "net": "synthetic.yml shapes, geometric init, seed 0",
           "clock": "HIP events around a window of calls (stages: the front end's own events, one call a window), ms per call; median / min / "
                    "max and every window; the routes of a comparison alternate",
           "host_reads": "keys_sort ends with the read of the cell count, compaction holds the read of the kept counts and the two "
                         "boolean gathers (face_map, fallback): their times include those waits"}
    ax = A.uniform_axes(args.resolution, (-0.7, 0.7))
    spacing = float(ax.spacing[0])
    raw = net.extract_mesh(ax)
    cleaned = A.clean(raw)
    mesh = cleaned.mesh
    V, F = int(mesh.verts.shape[0]), int(mesh.faces.shape[0])
    res["mesh"] = {"grid": f"{args.resolution}^3 over [-0.7, 0.7]^3", "spacing": spacing, "faces": int(raw.faces.shape[0]),
                   "verts": int(raw.verts.shape[0]), "topology": A.topology(raw).as_dict(), "faces_after_clean": F, "verts_after_clean": V,
                   "topology_after_clean": A.topology(mesh).as_dict()}
    res["clean"] = alternate([("clean", lambda: A.clean(raw), 2), ("topology", lambda: A.topology(raw).as_dict(), 2)], args.windows)
    inp = view_input(dev)
    cam, dirs, _ = eng.ray_setup(inp["uv"], inp["pose"], inp["intrinsics"])
    base_tree = A.build_bvh(mesh)
    base_rays = alternate([("build_bvh", lambda: A.build_bvh(mesh), 3), ("closest_hit", lambda: A.ray_mesh_intersect(base_tree, cam, dirs), 5)],
                          args.windows)
    base_rays.update(rays=int(cam.shape[0]), hits=int(A.ray_mesh_intersect(base_tree, cam, dirs).hit.sum()), faces=F)
    res["original_bvh_and_rays"] = base_rays
    for k in (2, 4, 8):
        h = k * spacing
        out = {"h": h}
        both = {c: A.simplify_vertex_clustering(mesh, h, c) for c in ("quadric", "average")}
        q = both["quadric"]
        M = int(A.voxel_down_sample(mesh.verts, h)[0].shape[0])
        F_out, V_out = int(q.mesh.faces.shape[0]), int(q.mesh.verts.shape[0])
        out["result"] = {"faces_in": F, "faces_out": F_out, "verts_in": V, "verts_out": V_out, "cells": M,
                         "fallback_share": float(q.fallback.double().mean()) if V_out else None, "topology": A.topology(q.mesh).as_dict(),
                         "watertight": A.topology(q.mesh).watertight, "oriented": A.topology(q.mesh).oriented}
        out["stages"] = {}
        for c in ("quadric", "average"):
            per = staged(A, mesh, h, c, args.windows)
            nbytes = stage_bytes(V, F, M, F_out, V_out, True, c == "quadric")
            out["stages"][c] = {}
            for s in STAGES:
                r = summary(per[s], 1)
                r.update(bytes=nbytes[s], gbytes_per_s=round(nbytes[s] / (float(np.median(per[s])) * 1e-3) / 1e9, 2))
                out["stages"][c][s] = r
        out["whole"] = alternate([("quadric", lambda: A.simplify_vertex_clustering(mesh, h, "quadric"), 2),
                                  ("average", lambda: A.simplify_vertex_clustering(mesh, h, "average"), 2)], args.windows)
        out["distance"] = {}
        for c in ("average", "quadric"):
            g = torch.Generator(device=dev).manual_seed(11)
            s = A.surface_scores(both[c].mesh, mesh, args.samples, threshold=spacing, generator=g)
            acc, comp = float(s["Acc"]), float(s["Comp"])
            out["distance"][c] = {"pred_to_original": acc, "original_to_pred": comp, "two_sided_mean": 0.5 * (acc + comp),
                                  "in_spacings": 0.5 * (acc + comp) / spacing}
        sm = q.mesh
        tree = A.build_bvh(sm)
        rays = alternate([("build_bvh", lambda: A.build_bvh(sm), 3), ("closest_hit", lambda: A.ray_mesh_intersect(tree, cam, dirs), 5)], args.windows)
        rays.update(rays=int(cam.shape[0]), hits=int(A.ray_mesh_intersect(tree, cam, dirs).hit.sum()), faces=F_out, bvh_bytes=int(tree.buffer.numel()))
        out["bvh_and_rays"] = rays
        res[f"h_{k}"] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
