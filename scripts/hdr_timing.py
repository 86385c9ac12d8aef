#!/usr/bin/env python3
"""Time the radiance net's output activations (rendering_network.output_activation: sigmoid / relu / softplus) and the HDR validation
views on one GPU, same build, same process.  Prints one JSON line and writes it to `--out`.

    python scripts/hdr_timing.py [--rays 1024] [--windows 7] [--out profiles/hdr_timing.json] [--bench this=FILE parent=FILE]

  rgb_forward_backward : i2sdf_rgb_forward + i2sdf_rgb_backward on `--rays` x 97 points, the synthetic.yml net (256 wide, bf16x3 kernels, the
                         module's default options), the same features, view directions and upstream gradient for the three activations
  views                : views.linear_to_srgb of a stack of `--views` views of 480 x 640, and views.image_metrics(hdr=True) against
                         image_metrics(hdr=False) on the same stack
The routes alternate; a window is `calls` calls between two HIP events after a warm-up; median / min / max and every window are recorded.
No threshold: the figures are a record.  `--bench`: two files holding the JSON result line of `bench.py --windows 7` of this commit and of
its parent, taken on the same machine in the same session; they are stored under "default_bench" with the check the change set for them (the
two ms_per_step medians differ by no more than the larger of the two runs' own min-to-max window ranges)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from idr_timing import alternate, bench_record      # the same windows and the same bench record as the 'idr' timing

ACTS = ("sigmoid", "relu", "softplus")


def entry_points(args, dev):
    from i2sdf_amd import synthetic_conf
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.engine import RenderEngine
    B, n = args.rays, 97
    M = B * n
    g = torch.Generator().manual_seed(1)
    cam = (torch.randn(B, 3, generator=g) * 0.2).to(dev)
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(dev)
    z = torch.sort(torch.rand(B, n + 1, generator=g) * 3.0, -1)[0].to(dev)
    cw = torch.randn(M, 3, generator=g).to(dev)
    routes, keep = [], []
    for act in ACTS:
        conf = synthetic_conf()
        conf["rendering_network"] = dict(conf["rendering_network"], output_activation=act)
        eng = RenderEngine(NetConfig.from_conf(conf), dev)
        eng.pack(eng.layout.init_flat(torch.Generator().manual_seed(3)).to(dev))
        fw = eng.sdf_forward_grad(rays=(cam, dirs, z, n), want_grad=True, save=True)

        def both(eng=eng, fw=fw):
            with eng.chain(M):
                rgb, rs, pev = eng.rgb_forward(dirs, n, fw["feat"], M, save=True)
                eng.rgb_backward(rgb, cw, rs, M)

        routes.append((act, both, args.calls))
        keep.append((eng, fw))
    res = alternate(routes, args.windows)
    for act in ACTS[1:]:
        res[f"{act}_over_sigmoid_median"] = round(res[act]["median_ms"] / res["sigmoid"]["median_ms"], 4)
    res["points"] = M
    return res


def views(args, dev):
    from i2sdf_amd import views as V
    n, H, W = args.views, 480, 640
    g = torch.Generator().manual_seed(7)
    pred = (torch.rand(n, H * W, 3, generator=g) * 4.0 - 0.2).to(dev)
    gt = (pred + 0.05 * torch.randn(n, H * W, 3, generator=g).to(dev)).contiguous()
    routes = [("linear_to_srgb", lambda: V.linear_to_srgb(pred), args.view_calls),
              ("image_metrics", lambda: V.image_metrics(pred, gt, (H, W)), args.view_calls),
              ("image_metrics_hdr", lambda: V.image_metrics(pred, gt, (H, W), hdr=True), args.view_calls)]
    res = alternate(routes, args.windows)
    res["views"], res["img_res"] = n, [H, W]
    # the tone map reads and writes every value once: what that is of the device's memory rate, from the median
    res["linear_to_srgb_GB_per_s"] = round(2 * 4 * pred.numel() / (res["linear_to_srgb"]["median_ms"] * 1e-3) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls", type=int, default=20, help="entry-point pairs per window")
    ap.add_argument("--view-calls", type=int, default=3, help="calls per window of the view routes")
    ap.add_argument("--bench", nargs="*", default=[], metavar="NAME=FILE", help="this=FILE parent=FILE: bench.py result lines to record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdr_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("hdr_timing.py needs a GPU: nothing is timed on the host")
    dev = torch.device("cuda")
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows,
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; the routes alternate",
           "rgb_forward_backward": entry_points(args, dev), "views": views(args, dev)}
    if args.bench:
        res["default_bench"] = bench_record(args.bench)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
