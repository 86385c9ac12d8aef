#!/usr/bin/env python3
"""Time the emitter clustering on one GPU: k-means++ seeding and Lloyd's iteration, the device route (csrc/kmeans.hip) against an eager
torch restatement of the reference's two functions on the same GPU.  Prints one JSON line and writes it to `--out`.

    python scripts/emitter_cluster_timing.py [--windows 7] [--out profiles/emitter_cluster_timing.json]

The reference ships no emitter configuration, so the sizes are ARBITRARY: n = 2^16, k = 8 and n = 2^20, k = 16 points of Gaussian blobs.

Route "device": i2sdf_amd.kmeans_pp_centroid and i2sdf_amd.KMeans.fit_predict -- stream-ordered, no host read.
Route "eager":  utils.kmeans_pp_centroid restated (an (n, i, 3) tensor per round, the pick by a running sum, numpy's global stream)
                and fast_pytorch_kmeans.KMeans.fit_predict restated from its source (similarity 2ab - a^2 - b^2, a dense (k, n) float mask
                every iteration, a blocking `error <= tol`); the library itself is not installed here.
"fit" starts both routes from the SAME centroids (a device seeding), so both run the same number of iterations unless a near tie decides
otherwise; the counts are recorded.  "seeding" is each route's own draw.  The routes alternate in one process; a window is `calls` calls
between two HIP events after a warm-up, and ends in a synchronise, so the eager route's blocking reads are inside its numbers.  Every window
is recorded; a ratio is claimed only where the device route's slowest window is below the eager route's fastest.  Peak memory is torch's
allocator peak above what was allocated before the call (the inputs)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

SIZES = ((1 << 16, 8), (1 << 20, 16))


def eager_pp(cloud, k):
    """The reference's seeding route restated in eager torch ops, paying what it pays: per round the (n, round, 3) block of offsets to
    every seed so far, its norms and their minimum over the seeds, an inverse-CDF pick (sum, running sum, threshold from numpy's global
    stream, first index past it) and one row gathered for the next round."""
    n = cloud.shape[0]
    picked = torch.empty(k, dtype=torch.int64, device=cloud.device)
    picked[0] = int(np.random.randint(n))
    for rnd in range(1, k):
        seeds = cloud.index_select(0, picked[:rnd])
        offsets = cloud[:, None, :] - seeds[None, :, :]
        nearest = torch.linalg.vector_norm(offsets, dim=2).amin(dim=1)
        threshold = float(np.random.random()) * nearest.sum()
        past = torch.gt(nearest.cumsum(0) - threshold, 0)
        picked[rnd] = past.to(torch.int32).argmax()
    return cloud.index_select(0, picked)


def eager_fit(X, centroids, max_iter=100, tol=1e-4):
    """fast_pytorch_kmeans.KMeans.fit_predict (euclidean, no minibatch) -> (labels, centroids, iterations)"""
    c = centroids.clone()
    k = c.shape[0]
    arange = torch.arange(k, device=X.device)[:, None]
    for it in range(max_iter):
        sim = 2 * X @ c.T - (X ** 2).sum(1)[:, None] - (c ** 2).sum(1)[None, :]
        closest = sim.argmax(1)
        mask = (closest[None, :].expand(k, -1) == arange).to(X.dtype)
        c_grad = torch.nan_to_num(mask @ X / mask.sum(-1)[:, None])
        error = (c_grad - c).pow(2).sum()
        c = c_grad
        if error <= tol:                                  # (blocks the host)
            break
    return closest, c, it + 1


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


def compare(routes, windows):
    """routes: name -> (fn, calls).  A route that cannot run is recorded with the reason instead of its times."""
    res, live = {}, {}
    for name, (fn, calls) in routes.items():
        try:
            fn(), fn()                                    # warm-up
            res[name] = {"peak_bytes_above_inputs": peak_above_inputs(fn)}
            live[name] = (fn, calls, [])
        except (RuntimeError, MemoryError) as e:
            res[name] = {"cannot_run": str(e).splitlines()[0][:300]}
            torch.cuda.empty_cache()
    for _ in range(windows):
        for name, (fn, calls, ws) in live.items():
            ws.append(window(fn, calls))
    for name, (fn, calls, ws) in live.items():
        res[name].update(summary(ws, calls))
    if "device" in live and "eager" in live:
        clear = res["device"]["max_ms"] < res["eager"]["min_ms"]
        res["device_slowest_window_below_eager_fastest"] = clear
        if clear:
            res["eager_over_device_median"] = round(res["eager"]["median_ms"] / res["device"]["median_ms"], 2)
    return res


def one_size(n, k, args, dev):
    from i2sdf_amd import KMeans, kmeans_pp_centroid
    g = torch.Generator(device=dev).manual_seed(n + k)
    centres = torch.rand(k, 3, device=dev, generator=g) * 4 - 2
    X = (centres[torch.randint(0, k, (n,), device=dev, generator=g)] + 0.15 * torch.randn(n, 3, device=dev, generator=g)).contiguous()
    np.random.seed(0)
    out = {"n": n, "k": k}
    out["seeding"] = compare({"device": (lambda: kmeans_pp_centroid(X, k, seed=1), args.calls_device),
                              "eager": (lambda: eager_pp(X, k), args.calls_eager)}, args.windows)
    init = kmeans_pp_centroid(X, k, seed=1)
    km = KMeans(k)
    out["fit"] = compare({"device": (lambda: km.fit_predict(X, init), args.calls_device),
                          "eager": (lambda: eager_fit(X, init), args.calls_eager)}, args.windows)
    labels = km.fit_predict(X, init)
    out["fit"]["device"]["iterations"] = int(km.n_iter)
    if "cannot_run" not in out["fit"]["eager"]:
        e_labels, _, e_iters = eager_fit(X, init)
        out["fit"]["eager"]["iterations"] = e_iters
        out["fit"]["labels_differing"] = int((e_labels != labels).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls-device", type=int, default=10)
    ap.add_argument("--calls-eager", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emitter_cluster_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("emitter_cluster_timing.py needs a GPU: nothing is timed on the host")
    dev = torch.device("cuda")
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows,
           "sizes": "arbitrary: the reference ships no emitter configuration",
           "clock": "HIP events around a window of calls ending in a synchronise, ms per call, median / min / max and every window; device "
                    "and eager alternate; a ratio only where the device route's slowest window is below the eager route's fastest",
           "runs": [one_size(n, k, args, dev) for n, k in SIZES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
