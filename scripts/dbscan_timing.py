#!/usr/bin/env python3
"""Time the density clustering (DBSCAN with the library's defaults, eps 0.5 and min_samples 5) on one GPU: the device route
(i2sdf_amd.DBSCAN, csrc/dbscan.hip) at the reference's sample of 10 000 points and at 2^20 points, and the reference's host route (the
download plus sklearn.cluster.DBSCAN) at 10 000 points.  Prints one JSON line and writes it to `--out`.

    python scripts/dbscan_timing.py [--windows 7] [--out profiles/dbscan_timing.json]

The clouds: 8 lamp-sized Gaussian blobs (sigma 0.15) with centres 3 apart on a 2 x 2 x 2 grid, shuffled.  The reference ships no emitter
configuration; 10 000 is the sample its own DBSCAN route draws, 2^20 the order of a whole emitter cloud.

Route "device": DBSCAN().fit_predict(X, check=False): cell keys, one stable torch.sort, labels -- stream-ordered, no host read.
Route "host":   X.cpu().numpy() and sklearn.cluster.DBSCAN().fit_predict, at 10 000 points only; a recorded skip where scikit-learn
                is not importable.
The routes alternate in one process; a window is `calls` calls between two HIP events after a warm-up and ends in a synchronise, so the
host route's download and host time are inside its numbers.  Every window is recorded.  Peak memory is torch's allocator peak above
what was allocated before the call (the inputs).  Also recorded per size: the occupied cells, the share of points made core by the
dense-cell shortcut (points of cells holding min_samples points or more), clusters, core and noise points.  The cost of each phase
(keys, sort, core flags, unions, labels) is NOT attributed: only whole calls are timed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

SIZES = (10000, 1 << 20)
HOST_SIZE = 10000
EPS, MIN_SAMPLES = 0.5, 5


def cloud(n, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    centres = 3.0 * torch.tensor([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=torch.float32, device=dev)
    X = centres[torch.arange(n, device=dev) % 8] + 0.15 * torch.randn(n, 3, device=dev, generator=g)
    return X[torch.randperm(n, device=dev, generator=g)].contiguous()


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def summary(ws, calls):
    return {"median_ms": round(float(np.median(ws)), 4), "min_ms": round(min(ws), 4), "max_ms": round(max(ws), 4),
            "windows_ms": [round(x, 4) for x in ws], "calls_per_window": calls}


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def cell_census(X):
    """occupied cells and the share of points in cells of min_samples points or more, from the library's own keys"""
    from i2sdf_amd import lib as L
    h = L.load()
    n = X.shape[0]
    ws = torch.empty(int(h.i2sdf_dbscan_workspace_bytes(n)), dtype=torch.uint8, device=X.device)
    keys = torch.empty(n, dtype=torch.int64, device=X.device)
    status = torch.zeros(1, dtype=torch.int32, device=X.device)
    L.check(h.i2sdf_dbscan_cell_keys(L.ptr(X), n, EPS, L.ptr(ws), L.ptr(keys), L.ptr(status), L.stream_ptr()), "i2sdf_dbscan_cell_keys")
    _, counts = torch.unique(keys, return_counts=True)
    return {"occupied_cells": int(counts.numel()), "largest_cell_points": int(counts.max()),
            "share_of_points_core_by_dense_cell": round(float(counts[counts >= MIN_SAMPLES].sum()) / n, 6)}


def one_size(n, args, dev, host_fit):
    from i2sdf_amd import DBSCAN
    X = cloud(n, dev)
    db = DBSCAN(EPS, MIN_SAMPLES)
    device = lambda: db.fit_predict(X, check=False)
    routes = {"device": (device, args.calls_device)}
    out = {"n": n, "eps": EPS, "min_samples": MIN_SAMPLES}
    if n == HOST_SIZE:
        if host_fit is None:
            out["host"] = {"skipped": "scikit-learn is not importable on this machine"}
        else:
            routes["host"] = (lambda: host_fit(X.cpu().numpy()), args.calls_host)
    live = {}
    for name, (fn, calls) in routes.items():
        fn(), fn()                                        # warm-up
        out[name] = {"peak_bytes_above_inputs": peak_above_inputs(fn)}
        live[name] = (fn, calls, [])
    for _ in range(args.windows):
        for name, (fn, calls, ws) in live.items():
            ws.append(window(fn, calls))
    for name, (fn, calls, ws) in live.items():
        out[name].update(summary(ws, calls))
    labels = device()
    out.update(cell_census(X))
    out.update({"clusters": int(db.n_clusters_), "core_points": int(db.core_sample_mask_.sum()), "noise_points": int((labels < 0).sum()),
                "status": int(db.status_)})
    if "host" in live:
        out["labels_differing_from_host"] = int((torch.from_numpy(host_fit(X.cpu().numpy())).to(dev) != labels).sum())
        clear = out["device"]["max_ms"] < out["host"]["min_ms"]
        out["device_slowest_window_below_host_fastest"] = clear
        if clear:
            out["host_over_device_median"] = round(out["host"]["median_ms"] / out["device"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls-device", type=int, default=50)
    ap.add_argument("--calls-host", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("dbscan_timing.py needs a GPU: nothing is timed on the host alone")
    try:
        from sklearn.cluster import DBSCAN as Library
        host_fit = lambda P: Library(eps=EPS, min_samples=MIN_SAMPLES).fit_predict(P)
    except ImportError:
        host_fit = None
    dev = torch.device("cuda")
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows,
           "sizes": "10 000 = the sample the reference's DBSCAN route draws; 2^20 = the order of a whole emitter cloud; no other size timed",
           "cloud": "8 Gaussian blobs, sigma 0.15, centres 3 apart on a 2 x 2 x 2 grid, shuffled",
           "clock": "HIP events around a window of calls ending in a synchronise, ms per call, median / min / max and every window; device "
                    "and host alternate; a ratio only where the device route's slowest window is below the host route's fastest",
           "not_attributed": "the cost of each phase (keys, sort, core flags, unions, labels): only whole calls are timed",
           "runs": [one_size(n, args, dev, host_fit) for n in SIZES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
