#!/usr/bin/env python3
"""Time the bubble-point draw on one GPU at the size of the reference's own data set: n = 150 x 640 x 480 = 46 080 000 points, weights
uniform in [0.05, 0.2] on a fraction of them (the rest 0), k = 1600.  Prints one JSON line and writes it to `--out`.

    python scripts/bubble_sample_timing.py [--n 46080000] [--k 1600] [--windows 7] [--out profiles/bubble_sample_timing.json]

Route "device": BubblePDF(sampler="device").sample_bubble -- one i2sdf_bubble_sample call (csrc/bubble.hip), no host read.
Route "eager":  BubblePDF().sample_bubble, the default sampler -- torch.where (a blocking read), two gathers, torch.multinomial; it
                refuses 2^24 or more positive entries, so it is timed at the eligible fractions 0.1 and 0.3 only; 1.0 is device only.
The routes alternate in one process; a window is `calls` calls between two HIP events after a warm-up of every shape, and the host clock
around the same window (ending in a synchronise) is recorded next to it, so the eager route's blocking read is inside both numbers.
Every window is recorded.  The device route reads the PDF `passes` times -- 2 to 4, decided on the device by the keys; the count is read
back from a draw on the timed PDF (BubblePDF.last_passes, outside the windows) -- and its time is also given as a multiple of the
streaming floor, passes x (4 n bytes at the 4.8 TB/s the project has measured for a streaming kernel).

Separately (`--views`, 0 to skip): BubblePDF.from_depth (depth maps uploaded, cloud and links built on the device) against a per-image
torch loop on the host in the style of the reference's data set followed by the upload of what it built, host clock, whole routes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

STREAM_BYTES_PER_S = 4.8e12       # measured for wgrad_all, a streaming kernel of this project


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls, 1e3 * (time.perf_counter() - t0) / calls


def summary(ws, calls):
    ev, host = [w[0] for w in ws], [w[1] for w in ws]
    return {"median_ms": round(float(np.median(ev)), 4), "min_ms": round(min(ev), 4), "max_ms": round(max(ev), 4),
            "host_median_ms": round(float(np.median(host)), 4), "windows_event_ms": [round(x, 4) for x in ev],
            "windows_host_ms": [round(x, 4) for x in host], "calls_per_window": calls}


def sample_routes(args, dev):
    from i2sdf_amd import BubblePDF
    n, k = args.n, args.k
    cloud = torch.rand(n, 3, device=dev)
    links = torch.zeros(1, dtype=torch.int64)
    g = torch.Generator(device=dev).manual_seed(1)
    base = torch.rand(n, device=dev, generator=g) * 0.15 + 0.05
    pick = torch.rand(n, device=dev, generator=g)
    device_bp = BubblePDF(cloud, links, sampler="device", seed=7)
    eager_bp = BubblePDF(cloud, links)
    out = {}
    for frac in args.fractions:
        pdf = torch.where(pick < frac, base, torch.zeros_like(base))
        device_bp.pdf.copy_(pdf)
        eager_bp.pdf.copy_(pdf)
        positive = int((pdf > 0).sum())
        routes = [("device", lambda: device_bp.sample_bubble(k), args.calls_device)]
        if positive < (1 << 24):
            routes.append(("eager", lambda: eager_bp.sample_bubble(k), args.calls_eager))
        for _, fn, _ in routes:                                   # warm-up of every shape
            fn(), fn()
        ws = {name: [] for name, _, _ in routes}
        for _ in range(args.windows):
            for name, fn, calls in routes:
                ws[name].append(window(fn, calls))
        res = {name: summary(ws[name], calls) for name, _, calls in routes}
        res["positive_entries"] = positive
        seen = set()                                              # the count depends on (pdf, draw): look at several draws
        for _ in range(8):
            device_bp.sample_bubble(k)
            seen.add(device_bp.last_passes())
        passes = max(seen)
        floor_ms = 1e3 * passes * 4 * n / STREAM_BYTES_PER_S
        res["device"]["passes"], res["device"]["passes_seen"], res["device"]["bytes_read"] = passes, sorted(seen), passes * 4 * n
        res["device"]["streaming_floor_ms"] = round(floor_ms, 4)
        res["device"]["multiple_of_streaming_floor"] = round(res["device"]["median_ms"] / floor_ms, 2)
        if "eager" in res:
            res["device_slowest_window_faster_than_eager_fastest"] = res["device"]["max_ms"] < res["eager"]["min_ms"]
            res["eager_over_device_median"] = round(res["eager"]["median_ms"] / res["device"]["median_ms"], 2)
        else:
            res["eager"] = "refuses: 2^24 or more positive entries (torch.multinomial's category limit)"
        out[f"eligible_{frac}"] = res
    out["shortfall_rows"] = device_bp.shortfall()
    return out


def host_loop(depth, K, pose, H, W, dev):
    """The data set's way: one image at a time on the host, then everything it built goes to the device."""
    total = H * W
    p = torch.arange(total)
    u, v = (p % W).float(), (p // W).float()
    clouds, links, pixs, masks, n_points = [], [], [], [], 0
    for i in range(depth.shape[0]):
        d = depth[i]
        mask = (d > 1e-3) & (d < 6)
        valid = torch.nonzero(mask)[:, 0]
        link = torch.full((total,), -1, dtype=torch.long)
        link[valid] = torch.arange(valid.numel()) + n_points
        n_points += valid.numel()
        fx, fy, cx, cy, sk = K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2], K[i, 0, 1]
        dv, uu, vv = d[valid], u[valid], v[valid]
        cam = torch.stack([(uu - cx + cy * sk / fy - sk * vv / fy) / fx * dv, (vv - cy) / fy * dv, dv, torch.ones_like(dv)], 0)
        clouds.append((pose[i] @ cam).T)
        links.append(link), pixs.append(valid + i * total), masks.append(mask)
    cloud = torch.cat(clouds)
    cloud = cloud[:, :3] / cloud[:, 3:]
    res = [x.to(dev) for x in (cloud, torch.cat(links), torch.cat(pixs), torch.stack(masks), depth)]
    torch.cuda.synchronize()
    return res


def cloud_routes(args, dev):
    from i2sdf_amd import BubblePDF
    n_img, H, W = args.views, args.height, args.width
    g = torch.Generator().manual_seed(3)
    depth = torch.rand(n_img, H * W, generator=g) * 7.0
    K = torch.eye(4).repeat(n_img, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 0.9 * W
    K[:, 0, 2], K[:, 1, 2], K[:, 0, 1] = W / 2, H / 2, 0.1
    pose = torch.eye(4).repeat(n_img, 1, 1)
    pose[:, :3, 3] = torch.rand(n_img, 3, generator=g)

    def device_route():
        bp = BubblePDF.from_depth(depth, K, pose, (H, W))
        torch.cuda.synchronize()
        return bp

    bp, ref = device_route(), host_loop(depth, K, pose, H, W, dev)          # warm-up, and the agreement
    agree = {"links_equal": bool(torch.equal(bp.pointlinks, ref[1]) and torch.equal(bp.pixlinks, ref[2])),
             "cloud_max_abs": float((bp.pointcloud - ref[0]).abs().max()), "points": int(bp.pointcloud.shape[0])}
    del bp, ref
    ms = {"from_depth": [], "host_loop_and_upload": []}
    for _ in range(args.windows):
        for name, fn in (("from_depth", device_route), ("host_loop_and_upload", lambda: host_loop(depth, K, pose, H, W, dev))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    out = {name: {"median_ms": round(float(np.median(t)), 1), "min_ms": round(min(t), 1), "max_ms": round(max(t), 1),
                  "windows_ms": [round(x, 1) for x in t]} for name, t in ms.items()}
    out.update(agreement=agree, views=n_img, image=[W, H], host_threads=torch.get_num_threads(),
               clock="host clock around the whole route, ending in a device synchronise; the routes alternate; both start from depth maps "
                     "in host memory and end with cloud, links, masks and depth maps on the device")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150 * 640 * 480)
    ap.add_argument("--k", type=int, default=1600)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.3, 1.0])
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls-device", type=int, default=200)
    ap.add_argument("--calls-eager", type=int, default=10)
    ap.add_argument("--views", type=int, default=150, help="views of the from_depth comparison (0: skip)")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bubble_sample_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("bubble_sample_timing.py needs a GPU: nothing is timed on the host")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda")
    res = {"device_name": torch.cuda.get_device_name(), "n": args.n, "k": args.k, "windows": args.windows,
           "clock": "HIP events around a window of calls, ms per call, median / min / max and every window; the host clock around the same "
                    "window next to it; device and eager alternate",
           "one_pass_floor_ms": round(1e3 * 4 * args.n / STREAM_BYTES_PER_S, 4), "sample": sample_routes(args, dev)}
    if args.views > 0:
        res["from_depth"] = cloud_routes(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
