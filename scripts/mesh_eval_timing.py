#!/usr/bin/env python3
"""Time i2sdf_amd.mesh.evaluate on one GPU beside the host route the reference takes (utils/mesh_util.py:evaluate): two seeded
clouds of `--points` points each on the walls of a 5 x 4 x 3 room (the second with 1 cm of noise), scored with the reference's
defaults (down_sample 0.02, threshold 0.05).  Prints one JSON line.

    python scripts/mesh_eval_timing.py [--points 2000000] [--reps 5] [--out profiles/mesh_eval_timing.json]

Device: medians of `reps` runs after one warm-up, by events on the current stream, host synchronisations included; the
per-stage times come from events the library records between its stages (keys + sort, mean, grid build, query, fallback) on a
further run, summed over both point sets / both directions.  Host: download of both clouds, the numpy down-sample of
tests/pointops_ref.py (open3d is not required) and scikit-learn's KDTree in both directions (scipy's cKDTree when scikit-learn is
not importable, "absent" when neither is); wall-clock, `--host-reps` runs."""
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

import pointops_ref as P
from i2sdf_amd.mesh import evaluate

KEYS = ("Acc", "Comp", "Prec", "Recal", "F-score")


def room(n, seed, noise, size=(5.0, 4.0, 3.0)):
    rng = np.random.default_rng(seed)
    areas = np.array([size[1] * size[2]] * 2 + [size[0] * size[2]] * 2 + [size[0] * size[1]] * 2)
    wall = rng.choice(6, size=n, p=areas / areas.sum())
    p = rng.random((n, 3)) * np.array(size)
    axis = wall // 2
    p[np.arange(n), axis] = (wall % 2) * np.array(size)[axis]
    return (p + rng.normal(0.0, noise, (n, 3))).astype(np.float32)


def host_tree():
    try:
        from sklearn.neighbors import KDTree
        return "sklearn.neighbors.KDTree", lambda q, r: KDTree(r).query(q)[0].reshape(-1)
    except ImportError:
        pass
    try:
        from scipy.spatial import cKDTree
        return "scipy.spatial.cKDTree (scikit-learn not importable)", lambda q, r: cKDTree(r).query(q)[0]
    except ImportError:
        return "absent", None


def host_route(pred, trgt, args):
    how, nn = host_tree()
    rec = {"nearest_neighbour": how, "down_sample": "numpy restatement (tests/pointops_ref.py)"}
    if nn is None:
        return rec, None
    t_down, t_ds, t_nn, m = [], [], [], None
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p, t = pred.cpu().numpy(), trgt.cpu().numpy()
        t1 = time.perf_counter()
        p, _ = P.voxel_down_sample(p, args.down_sample)
        t, _ = P.voxel_down_sample(t, args.down_sample)
        t2 = time.perf_counter()
        p64, t64 = p.astype(np.float64), t.astype(np.float64)
        dist1, dist2 = nn(t64, p64), nn(p64, t64)
        m = P.metrics(dist1, dist2, args.threshold)
        t3 = time.perf_counter()
        t_down.append(1e3 * (t1 - t0)); t_ds.append(1e3 * (t2 - t1)); t_nn.append(1e3 * (t3 - t2))
    med = lambda v: round(float(np.median(v)), 3)
    rec.update({"download_ms": med(t_down), "down_sample_ms": med(t_ds), "build_query_ms": med(t_nn),
                "total_ms": med(np.array(t_down) + np.array(t_ds) + np.array(t_nn)), "points_after_down_sample": [int(p.shape[0]), int(t.shape[0])]})
    return rec, m


def stages(stats):
    """Sum the time between consecutive stage events by the later event's label."""
    out, prev, n_fb = {}, None, 0
    for label, what in stats:
        if label == "fallback_count":
            n_fb += int(what)
            continue
        if label != "start" and prev is not None:
            out[label] = out.get(label, 0.0) + prev.elapsed_time(what)
        prev = what
    rec = {k + "_ms": round(v, 3) for k, v in out.items()}
    rec["fallback_queries"] = n_fb
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--down-sample", type=float, default=0.02)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    pred, trgt = torch.from_numpy(room(args.points, 1, 0.002)).cuda(), torch.from_numpy(room(args.points, 2, 0.01)).cuda()
    run = lambda stats=None: evaluate(pred, trgt, args.threshold, args.down_sample, _stats=stats)
    run()
    torch.cuda.synchronize()
    ms, got = [], None
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    stats = []
    run(stats)
    torch.cuda.synchronize()
    res = {"points": args.points, "threshold": args.threshold, "down_sample": args.down_sample, "reps": args.reps,
           "device_name": torch.cuda.get_device_name(),
           "device": {"total_ms": round(float(np.median(ms)), 3), "stages": stages(stats), "metrics": got}}
    host, m = host_route(pred, trgt, args)
    res["host"] = host
    if m is not None:
        res["host"]["metrics"] = m
        res["host_over_device"] = round(host["total_ms"] / res["device"]["total_ms"], 1)
        res["device_faster_than_host_route"] = bool(res["device"]["total_ms"] < host["total_ms"])
        res["metrics_max_rel_diff"] = max(abs(got[k] - m[k]) / max(abs(m[k]), 1e-300) for k in KEYS)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
