#!/usr/bin/env python3
"""Generate tests/golden/g19_mesh_components.npz: face-component labels from scipy.sparse.csgraph.connected_components (what
trimesh's split runs) on the face-adjacency graph, canonicalised to the smallest face index of each component (numpy + scipy;
run once wherever scipy is installed -- the GPU tests only read the file).

    python tests/golden/gen_mesh_components.py

    a, b, c    the three volumes of g18_mcubes.npz meshed by tests/mcubes_ref.py (only the labels are stored; the tests mesh again)
    bowtie     two tetrahedra that share exactly one vertex          -> 2 components
    hinge      two tetrahedra that share one edge                    -> 1 component
    fan        three triangles on one edge (a non-manifold edge)     -> 1 component under the library's rule
Each small case stores {tag}.verts / .faces; every case stores {tag}.labels (F,) int32.
"""
import os
import sys

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mcubes_ref  # noqa: E402

TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)


def small_cases():
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    # bow-tie: the second tetrahedron uses vertex 3 of the first as its vertex 0
    bow_v = np.concatenate([base, base[1:] + np.float32([0, 0, 1])])
    bow_f = np.concatenate([TET, np.array([3, 4, 5, 6], np.int32)[TET]])
    # hinge: the second tetrahedron shares the edge (2, 3)
    hin_v = np.concatenate([base, np.float32([[-1, 1, 1], [0, 2, 2]])])
    hin_f = np.concatenate([TET, np.array([2, 3, 4, 5], np.int32)[TET]])
    fan_v = np.float32([[0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 1, 0], [-1, -1, 0]])
    fan_f = np.int32([[0, 1, 2], [0, 1, 3], [1, 0, 4]])
    return {"bowtie": (bow_v, bow_f), "hinge": (hin_v, hin_f), "fan": (fan_v, fan_f)}


def scipy_labels(faces):
    """Components of the graph whose nodes are faces and whose edges join every two faces that share an unordered vertex pair."""
    f = np.asarray(faces, np.int64)
    F = f.shape[0]
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    owner = np.tile(np.arange(F), 3)
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, owner = e[order], owner[order]
    same = np.nonzero((e[1:] == e[:-1]).all(axis=1))[0]
    g = coo_matrix((np.ones(same.shape[0], bool), (owner[same], owner[same + 1])), shape=(F, F))
    n, lab = connected_components(g, directed=False)
    first = np.full(n, F, np.int64)
    np.minimum.at(first, lab, np.arange(F))
    return n, first[lab].astype(np.int32)


def main():
    z = np.load(os.path.join(HERE, "g18_mcubes.npz"))
    out = {}
    for tag in "abc":
        _, faces, _ = mcubes_ref.marching_cubes(z[f"{tag}.vol"], float(z[f"{tag}.level"]), z[f"{tag}.spacing"])
        n, out[f"{tag}.labels"] = scipy_labels(faces)
        print(f"{tag}: {faces.shape[0]} faces, {n} components")
    for tag, (v, f) in small_cases().items():
        n, lab = scipy_labels(f)
        out.update({f"{tag}.verts": v, f"{tag}.faces": f, f"{tag}.labels": lab})
        print(f"{tag}: {f.shape[0]} faces, {n} components")
    path = os.path.join(HERE, "g19_mesh_components.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
