#!/usr/bin/env python3
"""Generate tests/golden/g20_mesh_eval.npz: scikit-learn KDTree distances (the reference's call, utils/mesh_util.py:12-22) between
the vertex sets a.verts / b.verts of g18_mcubes.npz (5108 and 4440 points, two overlapping boxes' worth of surface; they are not
stored again), with and without voxel down-sampling at 0.1 (tests/pointops_ref.py: open3d's rule), and the five metrics of
mesh_util.py:evaluate at threshold 0.2 (numpy + scikit-learn; run once wherever scikit-learn is installed -- the tests only read
the file).

    python tests/golden/gen_mesh_eval.py

    {raw,ds}.dist1   fp64 distance of every b point (trgt) to its nearest a point (pred)
    {raw,ds}.dist2   fp64 distance of every a point (pred) to its nearest b point (trgt)
    {raw,ds}.metrics fp64 (Acc, Comp, Prec, Recal, F-score)
    ds.n             the down-sampled sizes (pred, trgt);  threshold, down_sample: the parameters
The generator asserts that no distance lies within 1e-6 (relative) of the threshold, so the thresholded counts of an fp32
implementation must match exactly, and that 0.1 < Prec, Recal < 0.9, so they say something.
"""
import os
import sys

import numpy as np
from sklearn.neighbors import KDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pointops_ref as P  # noqa: E402

THRESHOLD, DOWN_SAMPLE = 0.2, 0.1
KEYS = ("Acc", "Comp", "Prec", "Recal", "F-score")


def kdtree_nn(query, ref):
    d, i = KDTree(np.asarray(ref, np.float64)).query(np.asarray(query, np.float64))
    return d.reshape(-1), i.reshape(-1)


def main():
    z = np.load(os.path.join(HERE, "g18_mcubes.npz"))
    pred, trgt = z["a.verts"], z["b.verts"]
    out = {"threshold": np.float64(THRESHOLD), "down_sample": np.float64(DOWN_SAMPLE)}
    for tag, ds in (("raw", None), ("ds", DOWN_SAMPLE)):
        p, t = pred, trgt
        if ds:
            p, _ = P.voxel_down_sample(p, ds)
            t, _ = P.voxel_down_sample(t, ds)
            out["ds.n"] = np.int64([p.shape[0], t.shape[0]])
        dist1, _ = kdtree_nn(t, p)
        dist2, _ = kdtree_nn(p, t)
        for d in (dist1, dist2):
            assert not (np.abs(d - THRESHOLD) <= 1e-6 * THRESHOLD).any(), "a distance sits on the threshold"
        m = P.metrics(dist1, dist2, THRESHOLD)
        assert 0.1 < m["Prec"] < 0.9 and 0.1 < m["Recal"] < 0.9, m
        out[f"{tag}.dist1"], out[f"{tag}.dist2"] = dist1.astype(np.float64), dist2.astype(np.float64)
        out[f"{tag}.metrics"] = np.float64([m[k] for k in KEYS])
        print(f"{tag}: {p.shape[0]} pred / {t.shape[0]} trgt points, " + ", ".join(f"{k} {m[k]:.4f}" for k in KEYS))
    path = os.path.join(HERE, "g20_mesh_eval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
