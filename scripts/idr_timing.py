#!/usr/bin/env python3
"""Time the radiance net's 'idr' mode (rendering_network.mode: idr, d_in: 9) against 'nerf' mode on one GPU, same build, same process.
Prints one JSON line and writes it to `--out`.

    python scripts/idr_timing.py [--rays 1024] [--windows 7] [--out profiles/idr_timing.json] [--bench this=FILE parent=FILE]

Sizes: `--rays` x 97 points, the synthetic.yml net (256 wide, bf16x3 kernels, the module's default options).
  entry points : i2sdf_rgb_forward + i2sdf_rgb_backward ('nerf') against i2sdf_rgb_forward_idr + i2sdf_rgb_backward_idr ('idr') on the same
                 features, view directions, upstream gradient; 'idr' also reads the points (from the rays) and the normals and adds into nbar
  step         : I2SDFNetwork forward (sampler with a fixed iteration count) + I2SDFLoss + backward, both modes
The routes alternate; a window is `calls` calls between two HIP events after a warm-up; median / min / max and every window are recorded.
No threshold: the figures are a record.  `--bench`: two files holding the JSON result line of `bench.py --windows 7` of this commit and of its
parent, taken on the same box in the same session (`design_added_bytes_*` are counts from the tensor shapes, not measurements); they are stored under "nerf_bench" with the check the issue sets for them (the two
ms_per_step medians differ by no more than the larger of the two runs' own min-to-max window ranges)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


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


def confs():
    from i2sdf_amd import synthetic_conf
    nerf = synthetic_conf()
    idr = synthetic_conf()
    idr["rendering_network"] = dict(idr["rendering_network"], mode="idr", d_in=9)
    return {"nerf": nerf, "idr": idr}


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
    for mode, conf in confs().items():
        eng = RenderEngine(NetConfig.from_conf(conf), dev)
        eng.pack(eng.layout.init_flat(torch.Generator().manual_seed(3)).to(dev))
        fw = eng.sdf_forward_grad(rays=(cam, dirs, z, n), want_grad=True, save=True)
        nbar = torch.zeros(M, 3, device=dev)

        def both(eng=eng, fw=fw, nbar=nbar):
            with eng.chain(M):
                rgb, rs, pev = eng.rgb_forward(dirs, n, fw["feat"], M, save=True, fw=fw)
                eng.rgb_backward(rgb, cw, rs, M, nbar=nbar)

        routes.append((mode, both, args.calls))
        keep.append((eng, fw))
    res = alternate(routes, args.windows)
    res["idr_over_nerf_median"] = round(res["idr"]["median_ms"] / res["nerf"]["median_ms"], 4)
    res["points"] = M
    return res


def steps(args, dev):
    from i2sdf_amd import I2SDFLoss, I2SDFNetwork
    B = args.rays
    g = torch.Generator().manual_seed(5)
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 600.0
    K[0, 2], K[1, 2] = 320.0, 240.0
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.0, -2.0])
    uv = torch.stack([torch.randint(0, 640, (B,), generator=g), torch.randint(0, 480, (B,), generator=g)], -1).float().reshape(B, 1, 2)
    inp = {"uv": uv.to(dev), "intrinsics": K.repeat(B, 1, 1).to(dev), "pose": pose.repeat(B, 1, 1).to(dev)}
    gt = {"rgb": torch.rand(B, 3, generator=g).to(dev), "depth": (torch.rand(B, generator=g) * 3).to(dev),
          "depth_mask": torch.ones(B, dtype=torch.bool, device=dev),
          "normal": torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(dev), "normal_mask": torch.ones(B, dtype=torch.bool, device=dev)}
    routes, keep = [], []
    for mode, conf in confs().items():
        conf["use_normal"] = True
        torch.manual_seed(0)
        net = I2SDFNetwork(conf).to(dev).train()
        net.force_iters = args.sampler_iters
        loss_fn = I2SDFLoss(eikonal_weight=0.1, depth_weight=0.1, normal_weight=0.05)

        def step(net=net, loss_fn=loss_fn):
            out = net(inp)
            loss = loss_fn(out, gt, 0)["loss"]
            net.zero_grad(set_to_none=True)
            loss.backward()

        routes.append((mode, step, args.step_calls))
        keep.append(net)
    res = alternate(routes, args.windows)
    res["idr_over_nerf_median"] = round(res["idr"]["median_ms"] / res["nerf"]["median_ms"], 4)
    res["rays"], res["sampler_iters"] = B, args.sampler_iters
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
            return float(r["ms_per_step"]), float(max(w) - min(w))
        (a, ra), (b, rb) = ms(rec["this"]), ms(rec["parent"])
        out.update(ms_per_step_this=a, ms_per_step_parent=b, window_range_this=round(ra, 4), window_range_parent=round(rb, 4),
                   medians_differ_by=round(abs(a - b), 4), within_the_larger_window_range=abs(a - b) <= max(ra, rb))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--calls", type=int, default=20, help="entry-point pairs per window")
    ap.add_argument("--step-calls", type=int, default=5, help="training steps per window")
    ap.add_argument("--sampler-iters", type=int, default=2)
    ap.add_argument("--bench", nargs="*", default=[], metavar="NAME=FILE", help="this=FILE parent=FILE: bench.py result lines to record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idr_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("idr_timing.py needs a GPU: nothing is timed on the host")
    dev = torch.device("cuda")
    M = args.rays * 97
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows,
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; 'nerf' and 'idr' alternate",
           "rgb_forward_backward": entry_points(args, dev), "training_step": steps(args, dev),
           # DESIGN counts, not measurements: what the mode moves per radiance sample beyond 'nerf' mode, in bytes of global memory, counted from
           # the shapes of the tensors it adds or widens
           "design_added_bytes_per_point": {"saved side row, 40 instead of 32 floats: written by the forward, read by the weight gradients": 64,
                                     "normals read by the forward": 12, "ray origin / depth reads for x": 4,
                                     "nbar rows read and written by the backward": 24},
           "design_added_bytes_per_step": (64 + 12 + 4 + 24) * M,
           "layer0_reduction_columns": {"nerf": 288, "idr": 320}}
    if args.bench:
        res["nerf_bench"] = bench_record(args.bench)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
