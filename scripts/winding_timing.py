#!/usr/bin/env python3
"""Time the generalized winding number (include/i2sdf.h: "Winding number"; csrc/winding.hip) on one GPU, on the synthetic.yml net
(geometric init).  Prints one JSON line and writes it to `--out`.

    python scripts/winding_timing.py [--windows 7] [--out profiles/winding_timing.json]

  small_mesh       512 queries against 64 / 128 / 256 / 1024 / 4096 faces: route "brute" against route "bvh" (tree and moments built beforehand)
                   and against the two builds: what route "auto" decides on a bare mesh (i2sdf_amd.mesh.WINDING_BRUTE_MAX_FACES).
  mesh             the zero level on a 384^3 grid over [-0.7, 0.7]^3, extracted on the device.
  moments          winding_moments of that mesh's tree (the bottom-up pass and the per-node finish), beside build_bvh.
  near_surface     2^20 queries = sample_surface + N(0, 0.01) noise through the tree at beta = 2 and at beta = 3.
  uniform_box      2^20 queries uniform in the mesh's bounding box, the same.
  brute            every face for `--brute-queries` (4096) of the near-surface queries: 2^20 of them would take the same time per query
                   256 times over, so the figure is per 4096 queries and says so.
  agreement        on those 4096 queries: the largest |w(beta) - w(brute)|, and how many differ in `inside`.
Not timed: beta = inf through the tree (the exact sum in tree order: the brute route's work with scattered reads), and Morton-sorted
queries (not built).  A window is `calls` calls between two HIP events after a warm-up; the routes of a comparison alternate; median /
min / max and every window are recorded.  No figure is promised and there is no threshold: the numbers are a record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from view_embed_timing import alternate  # noqa: E402  (scripts/ is sys.path[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7, help="windows per route (at least 7); the median is reported, every window recorded")
    ap.add_argument("--resolution", type=int, default=384, help="grid points per axis of the extracted mesh")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--brute-queries", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("winding_timing.py needs a GPU: nothing is timed on the host")
    import i2sdf_amd as A
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows, "net": "synthetic.yml shapes, geometric init, seed 0",
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; the routes of a comparison alternate"}
    g = torch.Generator().manual_seed(4)
    res["small_mesh"] = {}
    for F in (64, 128, 256, 1024, 4096):
        centre = torch.rand(F, 1, 3, generator=g) * 2 - 1
        sv = (centre + 0.08 * torch.randn(F, 3, 3, generator=g)).reshape(-1, 3).to(dev)
        sf = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3).to(dev)
        sq = (torch.rand(512, 3, generator=g) * 2 - 1).to(dev)
        small = A.build_bvh((sv, sf))
        sm = A.winding_moments(small)
        r = alternate([("brute", lambda: A.winding_number((sv, sf), sq, route="brute"), 20),
                       ("bvh", lambda: A.winding_number(small, sq, moments=sm), 20),
                       ("build_bvh", lambda: A.build_bvh((sv, sf)), 20),
                       ("winding_moments", lambda: A.winding_moments(small), 20)], args.windows)
        r.update(faces=F, queries=512)
        res["small_mesh"][str(F)] = r
    net = A.I2SDFNetwork(A.synthetic_conf()).to(dev).eval()
    mesh = net.extract_mesh(A.uniform_axes(args.resolution, (-0.7, 0.7)))
    F = int(mesh.faces.shape[0])
    res["mesh"] = {"grid": f"{args.resolution}^3 over [-0.7, 0.7]^3", "faces": F, "verts": int(mesh.verts.shape[0])}
    bvh = A.build_bvh(mesh)
    mom = A.winding_moments(bvh)
    n = args.queries
    g = torch.Generator(device=dev).manual_seed(5)
    near = A.sample_surface(mesh, n, generator=g)[0] + 0.01 * torch.randn(n, 3, device=dev, generator=g)
    lo, hi = mesh.verts.min(0).values, mesh.verts.max(0).values
    box = lo + (hi - lo) * torch.rand(n, 3, device=dev, generator=g)
    res["moments"] = alternate([("winding_moments", lambda: A.winding_moments(bvh), 3), ("build_bvh", lambda: A.build_bvh(mesh), 3)], args.windows)
    res["moments"]["table_bytes"] = int(mom.buffer.numel())
    for name, q in (("near_surface", near), ("uniform_box", box)):
        res[name] = alternate([("beta_2", lambda: A.winding_number(bvh, q, 2.0, mom), 3), ("beta_3", lambda: A.winding_number(bvh, q, 3.0, mom), 3)],
                              args.windows)
        w = A.winding_number(bvh, q, 2.0, mom)
        res[name].update(queries=n, inside_fraction=float((w.abs() > 0.5).double().mean()), finite=bool(torch.isfinite(w).all()))
    sub = near[:args.brute_queries].contiguous()
    res["brute"] = alternate([("brute", lambda: A.winding_number(mesh, sub, route="brute"), 1),
                              ("beta_2", lambda: A.winding_number(bvh, sub, 2.0, mom), 1)], args.windows)
    res["brute"].update(queries=int(sub.shape[0]), faces=F)
    wb = A.winding_number(mesh, sub, route="brute")
    res["agreement"] = {"queries": int(sub.shape[0])}
    for beta in (2.0, 3.0):
        w = A.winding_number(bvh, sub, beta, mom)
        res["agreement"][f"beta_{beta:g}"] = {"max_abs_difference_to_brute": float((w - wb).abs().max()),
                                               "inside_differs": int(((w.abs() > 0.5) != (wb.abs() > 0.5)).sum())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
