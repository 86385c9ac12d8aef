#!/usr/bin/env python3
"""Derive the marching-cubes case tables (csrc/mcubes_tables.inc) from first principles.

    python i2sdf_amd/csrc/gen_mc_tables.py            # rewrites mcubes_tables.inc, prints the largest triangle count

Conventions (shared with csrc/mcubes.hip and the numpy restatement in tests/mcubes_ref.py):
  corner c in 0..7 sits at (c & 1, (c >> 1) & 1, (c >> 2) & 1) = (dx, dy, dz) from the cell's lattice point (i, j, k);
  the case byte has bit c set iff v(corner c) > level (NaN is "not above");
  edge e = 4 * axis + q runs along `axis` from its low corner; q = b0 + 2 * b1 holds the offsets along the other two axes
  in increasing axis order (x edges: q = dy + 2 dz, y edges: q = dx + 2 dz, z edges: q = dx + 2 dy).
The rule: on each of the six cube faces the crossing segments depend only on that face's four corners; an ambiguous face
(diagonal corners alike) keeps its above-level corners apart (each segment cuts one above corner off).  Every segment is
directed so that, traced into closed loops, the loops' right-hand normal points towards the above side; each loop is
fan-triangulated from its first vertex whose diagonals all cross the cube's interior (fan_apex).  Neighbouring cells see the same four corners on a shared face, so they cut it
into the same segments and the mesh has no cracks.
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mcubes_tables.inc")


def corner_pos(c: int) -> np.ndarray:
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edge_corners(e: int):
    """(low corner, high corner) of edge e."""
    axis, q = e // 4, e % 4
    others = [a for a in range(3) if a != axis]
    lo = ((q & 1) << others[0]) | (((q >> 1) & 1) << others[1])
    return lo, lo | (1 << axis)


EDGES = [edge_corners(e) for e in range(12)]


def edge_axis(e: int) -> int:
    return e // 4


def edge_mid(e: int) -> np.ndarray:
    a, b = EDGES[e]
    return 0.5 * (corner_pos(a) + corner_pos(b))


def cube_faces():
    """The six faces as (axis, side, outward normal, corners in cyclic order, edges)."""
    out = []
    for axis in range(3):
        u, w = [a for a in range(3) if a != axis]
        for side in (0, 1):
            base = side << axis
            ring = [base, base | (1 << u), base | (1 << u) | (1 << w), base | (1 << w)]
            edges = [e for e in range(12) if edge_axis(e) != axis and all(((c >> axis) & 1) == side for c in EDGES[e])]
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            out.append((axis, side, n, ring, edges))
    return out


FACES = cube_faces()


def crossing_edges(case: int):
    return [e for e in range(12) if ((case >> EDGES[e][0]) & 1) != ((case >> EDGES[e][1]) & 1)]


def face_segments(face, bits):
    """Directed segments (edge_from, edge_to) of one cube face; `bits` maps a corner to its above flag and is only read on the
    face's four corners."""
    _, _, n, ring, edges = face
    above = {c: (bits >> c) & 1 for c in ring}
    cross = [e for e in edges if above[EDGES[e][0]] != above[EDGES[e][1]]]
    if not cross:
        return []
    if len(cross) == 2:
        pairs = [tuple(cross)]
    else:                                           # ambiguous face: cut each above corner off on its own
        pairs = []
        for c in ring:
            if above[c]:
                pairs.append(tuple(e for e in cross if c in EDGES[e]))
    segs = []
    for e1, e2 in pairs:
        # m points from the segment towards the above side within the face: the above ends of its two edges minus the below ends
        hi = [a if above[a] else b for a, b in (EDGES[e1], EDGES[e2])]
        lo = [b if above[a] else a for a, b in (EDGES[e1], EDGES[e2])]
        m = sum(corner_pos(c) for c in hi) - sum(corner_pos(c) for c in lo)
        d = edge_mid(e2) - edge_mid(e1)
        # a loop of right-hand normal N runs along N x n_face where it crosses a face of outward normal n_face
        segs.append((e1, e2) if float(np.dot(d, np.cross(m, n))) > 0 else (e2, e1))
    return segs


def case_loops(case: int):
    """Closed loops of crossing edges (each starting at its smallest edge, loops in order of their smallest edge)."""
    nxt = {}
    for f in FACES:
        for a, b in face_segments(f, case):
            assert a not in nxt, (case, a)
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        loops.append(loop)
    return loops


def same_face(a: int, b: int) -> bool:
    return any(a in f[4] and b in f[4] for f in FACES)


def fan_apex(loop) -> int:
    """First loop position whose fan diagonals all pass through the cube's interior: a diagonal between two points of one face
    could be drawn by the neighbouring cell too, and the two cells would then cover the face twice."""
    n = len(loop)
    for s in range(n):
        if not any(same_face(loop[s], loop[(s + i) % n]) for i in range(2, n - 1)):
            return s
    raise AssertionError(f"no interior fan for loop {loop}")


def case_triangles(case: int):
    tris = []
    for loop in case_loops(case):
        s = fan_apex(loop)
        r = loop[s:] + loop[:s]
        for i in range(1, len(r) - 1):
            tris.append((r[0], r[i], r[i + 1]))
    return tris


def tables():
    """(tri_table int8 (256, max_tri, 3) padded with -1, n_tri int (256,), max_tri)."""
    all_tris = [case_triangles(c) for c in range(256)]
    max_tri = max(len(t) for t in all_tris)
    tab = np.full((256, max_tri, 3), -1, dtype=np.int8)
    ntri = np.zeros(256, dtype=np.int32)
    for c, t in enumerate(all_tris):
        ntri[c] = len(t)
        if t:
            tab[c, :len(t)] = np.array(t, dtype=np.int8)
    return tab, ntri, max_tri


def render() -> str:
    tab, ntri, max_tri = tables()
    lines = ["// Generated by i2sdf_amd/csrc/gen_mc_tables.py -- do not edit; rerun the script instead.",
             "// Edge e = 4*axis + q from its low corner (see the script for the corner / edge conventions).",
             f"#define I2SDF_MC_MAX_TRI {max_tri}",
             "// low corner of each edge (the lattice point that owns the edge's vertex is the cell's point + this corner's offset)",
             "static __constant__ const unsigned char kMcEdgeLo[12] = {" + ", ".join(str(EDGES[e][0]) for e in range(12)) + "};",
             "static __constant__ const unsigned char kMcNumTri[256] = {"]
    for r in range(0, 256, 32):
        lines.append("  " + ", ".join(str(int(v)) for v in ntri[r:r + 32]) + ",")
    lines.append("};")
    lines.append(f"static __constant__ const signed char kMcTriTable[256][{max_tri * 3}] = {{")
    for c in range(256):
        lines.append("  {" + ", ".join(str(int(v)) for v in tab[c].reshape(-1)) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}: largest triangle count of any case = {tables()[2]}")
