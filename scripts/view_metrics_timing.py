#!/usr/bin/env python3
"""Time the rendered-view metrics of i2sdf_amd.views on one GPU at the reference's test size: `--views` (20) views of 480 x 640,
seeded inputs (tests/views_ref.py:view_pair).  Prints one JSON line and writes it to `--out`.

    python scripts/view_metrics_timing.py [--views 20] [--calls 50] [--calls-fast 1000] [--windows 7] [--out profiles/view_metrics_timing.json]

Route A: views.image_metrics (one stats pass + the SSIM kernel, csrc/imgops.hip), all views in one call.
Route B: the same numbers by eager PyTorch ops on the same GPU -- the fp32 F.conv2d restatement of torchmetrics' SSIM (reflect pad, the
         five moments, crop) plus get_psnr, view by view as the reference calls them (about 25 small ops per view).  It is what a port without the
         kernel would run; it is not torchmetrics itself (not installed here).
Route C: route B batched -- the same eager ops once over all views (one conv2d over the stack): the eager route without the per-view
         launches, so that B - C shows what the launches cost and C what the library's 11 x 11 convolution and its elementwise passes cost.
A, B and C alternate in the same process; each number is the median over `--windows` windows between two events, after a warm-up
of every shape, with the minimum and maximum next to it.  A window holds `--calls` calls of B or C and `--calls-fast` calls of A
(so that A's window is not a few milliseconds).  Separately: views.to_frames on the same stack, and I2SDFNetwork.evaluate_views on the
synthetic configuration for 2 views of `--render-res` against render_image + download + the CPU restatement for the same two views
(whole routes, host work included, by the host clock around a synchronise; `--windows` alternating repeats, median, minimum and
maximum).  Agreement of the values is recorded next to the times.  No ratio is fixed in advance."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

import views_ref as VR
from i2sdf_amd import views as V


def eager_metrics(pred, gt, H, W, kernel):
    """Route B for one view: (psnr, ssim) as 0-d device tensors."""
    mse = torch.mean((pred - gt) ** 2)
    psnr = -10.0 * torch.log(mse) / math.log(10)
    p = pred.T.reshape(3, H, W).unsqueeze(0)
    t = gt.T.reshape(3, H, W).unsqueeze(0)
    R = torch.max(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    m = F.conv2d(torch.cat([p, t, p * p, t * t, p * t]), kernel, groups=3)
    pp, tt, pt = m[0] ** 2, m[1] ** 2, m[0] * m[1]
    sp, st, spt = m[2] - pp, m[3] - tt, m[4] - pt
    full = ((2 * pt + c1) * (2 * spt + c2)) / ((pp + tt + c1) * (sp + st + c2))
    return psnr, full[..., 5:-5, 5:-5].mean()


def eager_metrics_batched(pred, gt, H, W, kernel):
    """Route C: (psnr, ssim) (n,) device tensors for the whole stack, the ops of eager_metrics once."""
    n = pred.shape[0]
    psnr = -10.0 * torch.log(torch.mean((pred - gt) ** 2, dim=(1, 2))) / math.log(10)
    p = pred.reshape(n, H, W, 3).permute(0, 3, 1, 2)
    t = gt.reshape(n, H, W, 3).permute(0, 3, 1, 2)
    R = torch.maximum(p.amax((1, 2, 3)) - p.amin((1, 2, 3)), t.amax((1, 2, 3)) - t.amin((1, 2, 3))).reshape(n, 1, 1, 1)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    m = F.conv2d(torch.cat([p, t, p * p, t * t, p * t]), kernel, groups=3).reshape(5, n, 3, H, W)
    pp, tt, pt = m[0] ** 2, m[1] ** 2, m[0] * m[1]
    sp, st, spt = m[2] - pp, m[3] - tt, m[4] - pt
    full = ((2 * pt + c1) * (2 * spt + c2)) / ((pp + tt + c1) * (sp + st + c2))
    return psnr, full[..., 5:-5, 5:-5].mean((1, 2, 3))


def windows(fns, calls, n_windows):
    """Median, minimum and maximum ms per call of each fn over windows of calls[k] calls, the windows alternating between the fns."""
    ms = [[] for _ in fns]
    for _ in range(n_windows):
        for k, (fn, c) in enumerate(zip(fns, calls)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(c):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / c)
    return [{"median_ms": round(float(np.median(m)), 4), "min_ms": round(min(m), 4), "max_ms": round(max(m), 4), "calls_per_window": c}
            for m, c in zip(ms, calls)]


def render_routes(args, dev):
    from i2sdf_amd import I2SDFNetwork, synthetic_conf
    H, W = args.render_res
    net = I2SDFNetwork(synthetic_conf())
    net._init_parameters(torch.Generator().manual_seed(7))
    net = net.to(dev).eval()
    K = torch.eye(4); K[0, 0] = K[1, 1] = 0.9 * W; K[0, 2], K[1, 2] = W / 2, H / 2
    p0, p1 = VR.pose_pair(3, 20.0, t_scale=0.2)
    for p in (p0, p1):
        p[:3, 3] += -2.0 * p[:3, 2]
    poses = torch.from_numpy(np.stack([p0, p1])).float().to(dev)
    gt_np = np.stack([VR.view_pair(H, W, 90 + v, 0.0)[1] for v in range(2)])
    gt = torch.from_numpy(gt_np).to(dev)
    uv = V.pixel_grid(H, W, dev)

    def route_a():
        r = net.evaluate_views(poses, K, (H, W), gt_rgb=gt, keep_outputs=False)
        return r["psnr"].cpu().numpy(), r["ssim"].cpu().numpy()        # the one synchronisation

    def route_b():
        ps, ss = [], []
        for i in range(2):
            o = net.render_image({"uv": uv, "pose": poses[i:i + 1], "intrinsics": K[None].to(dev)})
            rgb = o["rgb_values"].cpu().numpy()
            o["depth_values"].cpu(), o["normal_map"].cpu()                # the reference downloads what it plots
            ps.append(VR.psnr(rgb, gt_np[i]))
            ss.append(float(VR.ssim_map_f32_conv2d(rgb.reshape(H, W, 3), gt_np[i].reshape(H, W, 3)).mean()))
        return np.array(ps), np.array(ss)

    routes = (("evaluate_views", route_a), ("render_image_download_cpu_restatement", route_b))
    vals = {name: fn() for name, fn in routes}                 # warm-up, and the values
    ms = {name: [] for name, _ in routes}
    for _ in range(args.windows):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    out = {name: {"median_ms": round(float(np.median(t)), 2), "min_ms": round(min(t), 2), "max_ms": round(max(t), 2),
                  "psnr": [float(x) for x in vals[name][0]], "ssim": [float(x) for x in vals[name][1]]} for name, t in ms.items()}
    a, b = out["evaluate_views"], out["render_image_download_cpu_restatement"]
    out["agreement"] = {"psnr_max_abs": float(np.abs(np.array(a["psnr"]) - np.array(b["psnr"])).max()),
                        "ssim_max_abs": float(np.abs(np.array(a["ssim"]) - np.array(b["ssim"])).max())}
    out["views"], out["image"], out["clock"] = 2, [W, H], f"host clock around a device synchronise, {args.windows} alternating repeats after one warm-up"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window (at least 50)")
    ap.add_argument("--calls-fast", type=int, default=1000, help="calls per timed window of image_metrics and to_frames")
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported")
    ap.add_argument("--render-res", type=int, nargs=2, default=[96, 128], metavar=("H", "W"), help="size of the 2 rendered views (0 0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_metrics_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.calls < 50 or args.calls_fast < 50 or args.windows < 7:
        ap.error("at least 50 calls per window and 7 windows")
    if not torch.cuda.is_available():
        sys.exit("view_metrics_timing.py needs a GPU: nothing is timed on the host")
    dev = torch.device("cuda")
    H, W, n = args.height, args.width, args.views
    pairs = [VR.view_pair(H, W, 500 + v, 0.02) for v in range(n)]
    pred = torch.from_numpy(np.stack([p for p, _ in pairs])).to(dev)
    gt = torch.from_numpy(np.stack([g for _, g in pairs])).to(dev)
    g1 = torch.from_numpy(VR.gaussian(np.float32)).reshape(1, 11).to(dev)
    kernel = (g1.t() @ g1).expand(3, 1, 11, 11).contiguous()
    route_a = lambda: V.image_metrics(pred, gt, (H, W))
    route_b = lambda: [eager_metrics(pred[v], gt[v], H, W, kernel) for v in range(n)]
    rng = np.random.default_rng(1)
    nrm = torch.from_numpy(rng.standard_normal((n, H * W, 3)).astype(np.float32)).to(dev)
    depth = torch.from_numpy(rng.uniform(0, 6, (n, H * W, 1)).astype(np.float32)).to(dev)
    poses = torch.eye(4, device=dev).repeat(n, 1, 1)
    frames = lambda: V.to_frames(rgb=pred, normal_map=nrm, depth=depth, pose=poses, img_res=(H, W))
    route_c = lambda: eager_metrics_batched(pred, gt, H, W, kernel)
    a, b, c = route_a(), route_b(), route_c()                # warm-up of every shape, and the values
    frames()
    torch.cuda.synchronize()
    b_psnr = torch.stack([x[0] for x in b]).double().cpu().numpy()
    b_ssim = torch.stack([x[1] for x in b]).double().cpu().numpy()
    diff = lambda x, y: float(np.abs(x.double().cpu().numpy() - y).max())
    t_a, t_b, t_c = windows([route_a, route_b, route_c], [args.calls_fast, args.calls, args.calls], args.windows)
    t_f, = windows([frames], [args.calls_fast], args.windows)
    res = {"device_name": torch.cuda.get_device_name(), "views": n, "image": [W, H], "windows": args.windows,
           "clock": "HIP events around a window of calls, ms per call (all views), median / min / max of the windows; A, B and C alternate",
           "image_metrics": t_a, "eager_conv2d_and_get_psnr": t_b, "eager_batched": t_c,
           "eager_route": "fp32 F.conv2d restatement of torchmetrics 0.11.4 SSIM + get_psnr, view by view, PyTorch-ROCm ops on the same GPU "
                          "(torchmetrics itself is not installed); about 25 small ops per view",
           "eager_batched_route": "the same eager ops once over the whole stack (one conv2d over all views)",
           "compulsory_bytes_per_call": 2 * 2 * 4 * 3 * H * W * n,      # stats and SSIM each read both stacks once
           "agreement": {"psnr_max_abs": diff(a["psnr"], b_psnr), "ssim_max_abs": diff(a["ssim"], b_ssim),
                         "batched_psnr_max_abs": diff(c[0], b_psnr), "batched_ssim_max_abs": diff(c[1], b_ssim)},
           "to_frames": dict(t_f, outputs="rgb8, normal8, depth8")}
    if args.render_res[0] > 0:
        res["evaluate_views_vs_download"] = render_routes(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
