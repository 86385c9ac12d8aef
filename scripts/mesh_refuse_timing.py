#!/usr/bin/env python3
"""Time i2sdf_amd.mesh.refuse on one GPU at the reference's size (utils/mesh_util.py:refuse as model/eval/recon.py calls it): a
synthetic 5 x 4 x 3 m room with a box of furniture, as the marching-cubes mesh of its signed distance volume (`--grid` points per
axis; 448 gives about 2 M faces, the size of extract_mesh_high_res's export), `--cameras` cameras at 640 x 480 on a loop inside
it, voxel 0.01, truncation 0.03, stride 4.  Prints one JSON line.

    python scripts/mesh_refuse_timing.py [--grid 448] [--cameras 150] [--reps 3] [--out profiles/mesh_refuse_timing.json]

Device: medians of `reps` runs after one warm-up, by events on the current stream, host synchronisations included; the per-stage
times (depth, mark + integrate, extract) come from events the library records between its stages on a further run.  Also recorded:
touched units, mesh sizes and the peak of torch's allocator over one run.  The reference's own pipeline (pyrender on EGL, open3d)
is not required and not run, so no ratio against it is given.  `--host-size` (> 0) also runs the numpy restatement of the tests
(tests/refuse_ref.py) on a small version of the scene, labelled as such: it is a check that the two agree, not a competitor."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from i2sdf_amd.mesh import marching_cubes, refuse, camera_matrices

SIZE = np.array([5.0, 4.0, 3.0])
BOX_LO, BOX_HI = np.array([1.5, 1.2, 0.0]), np.array([2.6, 2.1, 0.9])


def room_mesh(n, dev):
    """Marching-cubes mesh of the room's free space (positive inside the room and outside the furniture box), made on the device."""
    pad = 0.2
    ax = [torch.linspace(-pad, float(SIZE[k]) + pad, n, device=dev, dtype=torch.float32) for k in range(3)]

    def box_sdf(lo, hi):
        q = [torch.abs(ax[k] - 0.5 * (lo[k] + hi[k])) - 0.5 * (hi[k] - lo[k]) for k in range(3)]
        qx, qy, qz = q[0][:, None, None], q[1][None, :, None], q[2][None, None, :]
        out = torch.sqrt(qx.clamp_min(0) ** 2 + qy.clamp_min(0) ** 2 + qz.clamp_min(0) ** 2)
        return out + torch.maximum(torch.maximum(qx, qy), qz).clamp_max(0)
    vol = torch.minimum(-box_sdf(np.zeros(3), SIZE), box_sdf(BOX_LO, BOX_HI))
    sp = (SIZE + 2 * pad) / (n - 1)
    m = marching_cubes(vol, 0.0, spacing=tuple(sp), origin=(-pad,) * 3)
    del vol
    return m


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
    return P


def cameras(n):
    """n poses on a loop at eye height, each looking at a point further along the loop on the other side of the room."""
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    c = SIZE / 2
    eye = np.stack([c[0] + 1.6 * np.cos(t), c[1] + 1.2 * np.sin(t), 1.4 + 0.3 * np.sin(3 * t)], 1)
    tgt = np.stack([c[0] - 2.0 * np.cos(t + 0.7), c[1] - 1.6 * np.sin(t + 0.7), 1.0 + 0.8 * np.cos(2 * t)], 1)
    return torch.from_numpy(np.stack([look_at(e, g) for e, g in zip(eye, tgt)]))


def stages(stats):
    out, prev, extra = {}, None, {}
    for label, what in stats:
        if not isinstance(what, torch.cuda.Event):
            extra[label] = what
            continue
        if label != "start" and prev is not None:
            out[label] = out.get(label, 0.0) + prev.elapsed_time(what)
        prev = what
    rec = {k + "_ms": round(v, 3) for k, v in out.items()}
    rec["touched_units"] = int(extra.get("touched_units", 0))
    if "raster_counters" in extra:
        c = extra["raster_counters"].sum(0).tolist()
        rec["triangles_by_workgroup"], rec["triangles_by_lane"] = int(c[0]), int(c[1])
    return rec


def host_check(args, dev):
    """The numpy restatement on a small version of the scene (not the reference's pipeline): times and agreement."""
    import refuse_ref as R
    H, W = args.host_size * 3 // 4, args.host_size
    K = np.array([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1]])
    poses = cameras(4)
    mesh = room_mesh(64, dev)
    vl = 0.05
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = refuse(mesh, poses, K, H, W, voxel_length=vl)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    c2w, w2c = (a.numpy() for a in camera_matrices(poses))
    d = R.mesh_depth(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), w2c, K, H, W)["depth"]
    fz = R.tsdf_integrate(d, c2w, w2c, K, voxel_length=vl)
    rv, rf = R.tsdf_extract(fz["units"], fz["tsdf32"], fz["weight"], vl)
    t2 = time.perf_counter()
    return {"what": "numpy restatement of the tests (tests/refuse_ref.py), not the reference's pyrender + open3d pipeline",
            "faces_in": int(mesh.faces.shape[0]), "cameras": 4, "image": [W, H], "voxel_length": vl,
            "device_ms_first_call": round(1e3 * (t1 - t0), 1), "numpy_ms": round(1e3 * (t2 - t1), 1),
            "vertices": [int(got.verts.shape[0]), int(rv.shape[0])], "faces": [int(got.faces.shape[0]), int(rf.shape[0])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=448)
    ap.add_argument("--cameras", type=int, default=150)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-size", type=int, default=64, help="image width of the small scene the numpy restatement also runs (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_refuse_timing.json"), help="also write the JSON line to this file ('' to skip)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    mesh = room_mesh(args.grid, dev)
    poses = cameras(args.cameras)
    H, W = args.height, args.width
    K = np.array([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1]])
    run = lambda stats=None: refuse(mesh, poses, K, H, W, voxel_length=args.voxel, _stats=stats)
    out = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stats = []
    run(stats)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    res = {"faces_in": int(mesh.faces.shape[0]), "verts_in": int(mesh.verts.shape[0]), "cameras": args.cameras, "image": [W, H],
           "voxel_length": args.voxel, "sdf_trunc": 3 * args.voxel, "depth_sampling_stride": 4, "reps": args.reps,
           "device_name": torch.cuda.get_device_name(),
           "device": {"total_ms": round(float(np.median(ms)), 3), "stages": stages(stats), "verts_out": int(out.verts.shape[0]),
                      "faces_out": int(out.faces.shape[0]), "peak_bytes": int(peak), "peak_bytes_above_inputs": int(peak - base),
                      "depth_maps_bytes": 4 * args.cameras * H * W},
           "reference_pipeline": "not run (pyrender and open3d are not required by this repository): no ratio is claimed"}
    if args.host_size > 0:
        res["restatement_check"] = host_check(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
