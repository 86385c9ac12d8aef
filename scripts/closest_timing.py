#!/usr/bin/env python3
"""Time the closest-point query (include/i2sdf.h: "Closest point"; csrc/closest.hip) on one GPU, on the synthetic.yml net (geometric init).
Prints one JSON line and writes it to `--out`.

    python scripts/closest_timing.py [--windows 7] [--out profiles/closest_timing.json]

  small_mesh       512 queries against 64 / 256 / 1024 / 4096 faces, route "brute" against route "bvh" (tree built beforehand): what
                   route "auto" decides on a bare mesh (i2sdf_amd.mesh.CLOSEST_BRUTE_MAX_FACES is set from this).
  mesh             the zero level on a 384^3 grid over [-0.7, 0.7]^3, extracted on the device.
  near_surface     2^20 queries = sample_surface + N(0, 0.01) noise against the tree, with and without the sign.
  uniform_box      2^20 queries uniform in the mesh's bounding box against the tree.
  routes_on_...    2048 of those queries through both routes on that mesh (marching cubes emits slivers): the rows that differ, and
                   the faces outside the class for which the header derives the box slack.
  pseudonormals    the tables of that mesh (keys, two torch.sort, reduce).
  surface_scores   100 000 samples per side, the mesh against itself shifted by 0.01 (two tree builds, two sample passes, two queries).
Not timed: queries far outside the mesh (best-first with an infinite start bound visits much of the tree before the first leaf
tightens it), and Morton-sorted queries (not built: neighbouring lanes of a wave walk unrelated paths for uniform_box).
A window is `calls` calls between two HIP events after a warm-up; the routes of a comparison alternate; median / min / max and every window
are recorded.  No figure is promised and there is no threshold: the numbers are a record."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_timing.json"), help="also write the JSON line here ('' to skip)")
    args = ap.parse_args()
    if args.windows < 7:
        ap.error("at least 7 windows")
    if not torch.cuda.is_available():
        sys.exit("closest_timing.py needs a GPU: nothing is timed on the host")
    import i2sdf_amd as A
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device_name": torch.cuda.get_device_name(), "windows": args.windows, "net": "synthetic.yml shapes, geometric init, seed 0",
           "clock": "HIP events around a window of calls, ms per call; median / min / max and every window; the routes of a comparison alternate"}
    # small meshes: every query against every face, or a tree over them
    g = torch.Generator().manual_seed(4)
    res["small_mesh"] = {}
    for F in (64, 256, 1024, 4096):
        centre = torch.rand(F, 1, 3, generator=g) * 2 - 1
        sv = (centre + 0.08 * torch.randn(F, 3, 3, generator=g)).reshape(-1, 3).to(dev)
        sf = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3).to(dev)
        sq = (torch.rand(512, 3, generator=g) * 2 - 1).to(dev)
        small = A.build_bvh((sv, sf))
        a, b = A.closest_point((sv, sf), sq, route="brute"), A.closest_point(small, sq)
        assert torch.equal(a.dist, b.dist) and torch.equal(a.face, b.face)
        r = alternate([("brute", lambda: A.closest_point((sv, sf), sq, route="brute"), 20),
                       ("bvh", lambda: A.closest_point(small, sq), 20),
                       ("build_bvh", lambda: A.build_bvh((sv, sf)), 20)], args.windows)
        r.update(faces=F, queries=512)
        res["small_mesh"][str(F)] = r
    # a level set
    net = A.I2SDFNetwork(A.synthetic_conf()).to(dev).eval()
    mesh = net.extract_mesh(A.uniform_axes(args.resolution, (-0.7, 0.7)))
    F = int(mesh.faces.shape[0])
    res["mesh"] = {"grid": f"{args.resolution}^3 over [-0.7, 0.7]^3", "faces": F, "verts": int(mesh.verts.shape[0])}
    bvh = A.build_bvh(mesh)
    n = args.queries
    g = torch.Generator(device=dev).manual_seed(5)
    near = A.sample_surface(mesh, n, generator=g)[0] + 0.01 * torch.randn(n, 3, device=dev, generator=g)
    lo, hi = mesh.verts.min(0).values, mesh.verts.max(0).values
    box = lo + (hi - lo) * torch.rand(n, 3, device=dev, generator=g)
    res["pseudonormals"] = alternate([("pseudonormals", lambda: A.pseudonormals(mesh), 3)], args.windows)
    nm = A.pseudonormals(mesh)
    res["near_surface"] = alternate([("closest_point", lambda: A.closest_point(bvh, near), 3),
                                     ("closest_point_signed", lambda: A.closest_point(bvh, near, normals=nm), 3)], args.windows)
    r = A.closest_point(bvh, near, normals=nm)
    res["near_surface"].update(queries=n, noise_sigma=0.01, mean_dist=float(r.dist.double().mean()), inside_fraction=float((r.sdist < 0).double().mean()),
                               status=int(r.status.item()))
    res["uniform_box"] = alternate([("closest_point", lambda: A.closest_point(bvh, box), 3)], args.windows)
    r = A.closest_point(bvh, box)
    res["uniform_box"].update(queries=n, mean_dist=float(r.dist.double().mean()), status=int(r.status.item()))
    # the level set has the slivers marching cubes emits: both routes on a subsample, and how many faces lie outside the class for
    # which include/i2sdf.h derives the box slack (near queries: L^5 <= 2^16 M |ab x ac|^2, L the longest edge)
    sub = torch.cat([near[:1024], box[:1024]])
    a, b = A.closest_point(bvh, sub, normals=nm), A.closest_point(mesh, sub, normals=nm, route="brute")
    differ = sum(int((getattr(a, k).reshape(len(sub), -1).view(torch.int32) != getattr(b, k).reshape(len(sub), -1).view(torch.int32)).any(1).sum())
                 for k in ("dist", "point", "face", "bary", "sdist")) + int((a.feature != b.feature).sum())
    P = mesh.verts.double()[mesh.faces.long()]
    ab, ac = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n2 = torch.linalg.cross(ab, ac).pow(2).sum(1)
    L = torch.stack([ab.norm(dim=1), ac.norm(dim=1), (P[:, 2] - P[:, 1]).norm(dim=1)]).max(0).values
    M = float(mesh.verts.abs().max())
    res["routes_on_the_level_set"] = {"queries": int(len(sub)), "rows_that_differ_between_tree_and_brute": differ,
                                      "zero_area_faces": int((n2 == 0).sum()),
                                      "faces_outside_the_derived_class": int(((n2 > 0) & (L.pow(5) > 2.0 ** 16 * M * n2)).sum()),
                                      "smallest_sin2_of_a_face": float((n2 / (ab.pow(2).sum(1) * ac.pow(2).sum(1)))[n2 > 0].min())}
    del P, ab, ac, n2, L
    moved = A.Mesh(mesh.verts + 0.01, mesh.faces, mesh.normals)
    ns = 100000
    draws = {k: {"u_face": torch.rand(ns, device=dev, generator=g), "u_bary": torch.rand(ns, 2, device=dev, generator=g)} for k in ("pred", "trgt")}
    res["surface_scores"] = alternate([("surface_scores", lambda: A.surface_scores(mesh, moved, ns, draws=draws), 3)], args.windows)
    res["surface_scores"].update(samples_per_side=ns, scores={k: float(v) for k, v in A.surface_scores(mesh, moved, ns, draws=draws).items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    assert differ == 0, f"tree route and brute route differ in {differ} rows on the level set"


if __name__ == "__main__":
    main()
