#!/usr/bin/env python3
"""Time the all-device mesh path on one GPU: I2SDFNetwork.sdf_volume and i2sdf_amd.mesh.marching_cubes for the synthetic.yml
network on uniform_axes(R) and on a PCA-aligned grid of the same resolution (rot/trans as model/eval/recon.py:75-95 uses them).
Prints one JSON line.  Its `high_res` record times I2SDFNetwork.extract_mesh_high_res(R) in total and, on the final high-res
mesh, the device mesh operations (face_components, largest_component, sample_surface) beside the host route the reference
takes for the same mesh: download + connected components of the face-adjacency graph (scipy.sparse.csgraph, what
trimesh's split runs, when scipy is importable; otherwise the numpy restatement of tests/meshops_ref.py, labelled as such).

    python scripts/mesh_timing.py [--resolution 512] [--reps 3] [--out profiles/mesh_high_res_timing.json]

Times are medians of `reps` runs after one warm-up, by events on the current stream; marching_cubes includes its one
host synchronisation (the vertex / face counts) and the allocation of its outputs."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from i2sdf_amd import I2SDFNetwork, synthetic_conf, uniform_axes, aligned_axes
from i2sdf_amd.mesh import face_components, largest_component, marching_cubes, sample_surface
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


def host_components(mesh, reps):
    """The reference's route to the components of a device mesh: download, face adjacency, connected components.  Wall-clock
    medians in ms (the host work is synchronous), the download included in the total."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import meshops_ref as M
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        how = "scipy.sparse.csgraph.connected_components"
    except ImportError:
        connected_components = None
        how = "numpy restatement (tests/meshops_ref.py); scipy not importable"
    t_down, t_adj, t_cc, n_comp = [], [], [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, faces = mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy()
        t1 = time.perf_counter()
        if connected_components is not None:
            pairs = M.adjacency_pairs(faces)
            t2 = time.perf_counter()
            g = coo_matrix((np.ones(len(pairs), bool), (pairs[:, 0], pairs[:, 1])), shape=(faces.shape[0],) * 2)
            n_comp, _ = connected_components(g, directed=False)
        else:
            t2 = t1
            n_comp = int(np.unique(M.face_components(faces)).shape[0])
        t3 = time.perf_counter()
        t_down.append(1e3 * (t1 - t0)); t_adj.append(1e3 * (t2 - t1)); t_cc.append(1e3 * (t3 - t2))
    med = lambda v: round(float(np.median(v)), 3)
    return {"method": how, "download_ms": med(t_down), "face_adjacency_ms": med(t_adj), "connected_components_ms": med(t_cc),
            "total_ms": med(np.array(t_down) + np.array(t_adj) + np.array(t_cc)), "components": int(n_comp),
            "note": "labels only: the areas, the choice of the largest component and the sub-mesh are not included on the host side"}


def high_res(net, args):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    draws = {"u_face": torch.rand(10000, generator=g).to(dev), "u_bary": torch.rand(10000, 2, generator=g).to(dev)}
    ms_total, out = timed(lambda: net.extract_mesh_high_res(args.resolution, draws=draws), args.reps)
    m, axes = out[0], out[3]
    rec = {"extract_mesh_high_res_ms": round(ms_total, 3), "shape": list(axes.shape_volume), "vertices": int(m.verts.shape[0]),
           "faces": int(m.faces.shape[0])}
    m = type(m)(m.verts.contiguous(), m.faces, m.normals.contiguous())
    ms, lab = timed(lambda: face_components(m), args.reps)
    rec["face_components_ms"] = round(ms, 3)
    rec["components"] = int(torch.unique(lab).numel())
    ms, big = timed(lambda: largest_component(m), args.reps)
    rec["largest_component_ms"] = round(ms, 3)
    rec["largest_component_faces"] = int(big.faces.shape[0])
    n = 1_000_000
    d2 = {"u_face": torch.rand(n, device=dev), "u_bary": torch.rand(n, 2, device=dev)}
    ms, _ = timed(lambda: sample_surface(m, n, draws=d2), args.reps)
    rec["sample_surface_1M_ms"] = round(ms, 3)
    rec["host_route"] = host_components(m, args.reps)
    rec["device_largest_component_faster_than_host_route"] = bool(rec["largest_component_ms"] < rec["host_route"]["total_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
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
    res["high_res"] = high_res(net, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
