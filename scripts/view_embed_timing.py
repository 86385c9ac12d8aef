#!/usr/bin/env python3
"""Time the radiance net's view embedders -- positional (multires 4), spherical harmonics of degree 4, Fourier features with 12 channels --
in 'nerf' and 'idr' mode on one GPU, same build, same process.  Prints one JSON line and writes it to `--out`.

    python scripts/view_embed_timing.py [--rays 1024] [--windows 7] [--out profiles/view_embed_timing.json] [--bench this=FILE parent=FILE]

Sizes: `--rays` x 97 points, the synthetic.yml net (256 wide, bf16x3 kernels, the module's default options).  A route is the radiance forward
plus backward entry points (i2sdf_rgb_forward + i2sdf_rgb_backward, or their _idr twins) on the same features, view directions and upstream
gradient.  The six routes alternate; a window is `calls` calls between two HIP events after a warm-up; median / min / max and every window are
recorded.  The GEMM shapes, stage counts and saved-tensor widths of the three embedders are the same (csrc/plan.h: side_chunks), so no ratio
is promised and there is no threshold: the figures are a record.  `--bench`: two files holding the JSON result line of `bench.py --windows 7`
of this commit and of its parent, taken on the same box in the same session; they are stored under "default_path_bench" with both runs'
window ranges."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

EMBEDS = {"positional": {"embed_type": "positional", "multires": 4}, "sh4": {"embed_type": "spherical_harmonics", "degree": 4},
          "ff12": {"embed_type": "fourier", "channels": 12, "sigma": 1.0}}


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


def alternate(routes, windows):
    for _, fn, _ in routes:
        fn(), fn()
    ws = {name: [] for name, _, _ in routes}
    for _ in range(windows):
        for name, fn, calls in routes:
            ws[name].append(window(fn, calls))
    return {name: summary(ws[name], calls) for name, _, calls in routes}


def conf_of(mode, embed):
    from i2sdf_amd import synthetic_conf
    conf = synthetic_conf()
    r = {k: v for k, v in conf["rendering_network"].items() if k not in ("embed_type", "multires")}
    r.update(EMBEDS[embed])
    if mode == "idr":
        r.update(mode="idr", d_in=9)
    conf["rendering_network"] = r
    return conf


def entry_points(args, dev):
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
    for mode in ("nerf", "idr"):
        for embed in EMBEDS:
            cfg = NetConfig.from_conf(conf_of(mode, embed))
            eng = RenderEngine(cfg, dev)
            buffers = {}
            eng.pack(eng.layout.init_flat(torch.Generator().manual_seed(3), buffers).to(dev))
            for Bm in buffers.values():
                eng.set_view_embed(Bm)
            fw = eng.sdf_forward_grad(rays=(cam, dirs, z, n), want_grad=True, save=True)
            nbar = torch.zeros(M, 3, device=dev)

            def both(eng=eng, fw=fw, nbar=nbar):
                with eng.chain(M):
                    rgb, rs, pev = eng.rgb_forward(dirs, n, fw["feat"], M, save=True, fw=fw)
                    eng.rgb_backward(rgb, cw, rs, M, nbar=nbar)

            routes.append((f"{mode}/{embed}", both, args.calls))
            keep.append((eng, fw))
    res = alternate(routes, args.windows)
    for mode in ("nerf", "idr"):
        for embed in ("sh4", "ff12"):
            res[f"{mode}/{embed}_over_positional_median"] = round(res[f"{mode}/{embed}"]["median_ms"] / res[f"{mode}/positional"]["median_ms"], 4)
    res["points"] = M
    return res


def bench_record(pairs):
    rec = {}
    for pair in pairs:
        name, path = pair.split("=", 1)
        line = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
        rec[name] = json.loads(line)
    out = {"lines": rec}
    if "this" in rec and "parent" in rec:
        def ms(r):
            w = r.get("windows_ms_per_step") or r.get("ms_per_step_windows") or [r["ms_per_step"]]
            return float(r["ms_per_step"]), [float(min(w)), float(max(w))]
        (a, ra), (b, rb) = ms(rec["this"]), ms(rec["parent"])
        out.update(ms_per_step_this=a, ms_per_step_parent=b, window_range_this=ra, window_range_parent=rb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls", type=int, default=20, help="entry-point pairs per window")
    ap.add_argument("--bench", nargs="*", default=[], metavar="NAME=FILE", help="this=FILE parent=FILE: bench.py result lines to record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_embed_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("view_embed_timing.py needs a GPU: nothing is timed on the host")
    dev = torch.device("cuda")
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows,
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; the six routes alternate",
           "rgb_forward_backward": entry_points(args, dev),
           "layer0_reduction_columns": {"nerf": 288, "idr": 320}, "view_columns_used": {"positional": 27, "sh4": 16, "ff12": 27}}
    if args.bench:
        res["default_path_bench"] = bench_record(args.bench)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
