#!/usr/bin/env python3
"""Time the all-device mesh path on one GPU: I2SDFNetwork.sdf_volume and i2sdf_amd.mesh.marching_cubes for the synthetic.yml
network on uniform_axes(R) and on a PCA-aligned grid of the same resolution (rot/trans as model/eval/recon.py:75-95 uses them).
Prints one JSON line.

    python scripts/mesh_timing.py [--resolution 512] [--reps 3]

Times are medians of `reps` runs after one warm-up, by events on the current stream; marching_cubes includes its one
host synchronisation (the vertex / face counts) and the allocation of its outputs."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from i2sdf_amd import I2SDFNetwork, synthetic_conf, uniform_axes, aligned_axes
from i2sdf_amd.mesh import marching_cubes
from oracle import i2sdf_oracle as orc


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms, out = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ocfg = orc.synthetic_cfg()
    net = I2SDFNetwork(synthetic_conf())
    net.load_state_dict(orc.perturb_params(orc.init_params(ocfg, seed=5), 0.02, seed=6))
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(0)
    rot, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    trans = torch.tensor([0.05, -0.1, 0.2])
    # an anisotropic cloud in the eigen-frame, like the PCA-aligned helper points of model/eval/recon.py:70-81
    helper = torch.randn(10000, 3, generator=g) * torch.tensor([0.5, 0.35, 0.25])
    grids = {"uniform": (uniform_axes(args.resolution), None, None),
             "aligned": (aligned_axes(helper, args.resolution), rot, trans)}
    res = {"resolution": args.resolution, "reps": args.reps, "device": torch.cuda.get_device_name()}
    for name, (ax, r, t) in grids.items():
        ms_vol, vol = timed(lambda: net.sdf_volume(ax, rot=r, trans=t), args.reps)
        s = ax.spacing
        ms_mc, m = timed(lambda: marching_cubes(vol, 0.0, s, ax.origin), args.reps)
        res[name] = {"shape": list(ax.shape_volume), "points": int(vol.numel()), "sdf_volume_ms": round(ms_vol, 3),
                     "marching_cubes_ms": round(ms_mc, 3), "vertices": int(m.verts.shape[0]), "faces": int(m.faces.shape[0])}
        del vol, m
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
