"""CPU: the marching-cubes case tables (i2sdf_amd/csrc/gen_mc_tables.py -> mcubes_tables.inc) and the numpy restatement of the
device kernels (tests/mcubes_ref.py) against scikit-image's meshes (tests/golden/g18_mcubes.npz, made by gen_mcubes.py)."""
import os

import numpy as np
import pytest

import mcubes_ref as R

G = R.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_include_file_is_the_generators_output():
    with open(os.path.join(ROOT, "i2sdf_amd", "csrc", "mcubes_tables.inc")) as f:
        assert f.read() == G.render(), "mcubes_tables.inc is stale: rerun i2sdf_amd/csrc/gen_mc_tables.py"
    assert R.MAX_TRI == 5


@pytest.mark.parametrize("case", range(256))
def test_case_uses_exactly_the_crossing_edges_in_closed_loops_wound_towards_above(case):
    tris = G.case_triangles(case)
    assert len(tris) == R.NUM_TRI[case]
    used = sorted({e for t in tris for e in t})
    assert used == G.crossing_edges(case)
    above = [(case >> c) & 1 for c in range(8)]
    for loop in G.case_loops(case):
        # consecutive loop edges share a cube face (the loop runs on the cube surface)
        for a, b in zip(loop, loop[1:] + loop[:1]):
            assert any(a in f[4] and b in f[4] for f in G.FACES), (case, loop)
        # right-hand normal of the loop (at the edge midpoints) against the loop edges' below -> above directions
        P = [G.edge_mid(e) for e in loop]
        area = 0.5 * sum(np.cross(P[i], P[(i + 1) % len(P)]) for i in range(len(P)))
        up = sum(G.corner_pos(hi if above[hi] else lo) - G.corner_pos(lo if above[hi] else hi) for lo, hi in (G.EDGES[e] for e in loop))
        assert float(np.dot(area, up)) > 0, (case, loop)
    # the fan triangles keep the loop's orientation: every directed edge of the case appears once, every undirected one
    # inside a loop twice (once per direction)
    de = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(de)) == len(de)


@pytest.mark.parametrize("face", range(6))
def test_face_segments_depend_only_on_the_faces_four_corners(face):
    f = G.FACES[face]
    ring = f[3]
    others = [c for c in range(8) if c not in ring]
    for bits in range(16):
        on_face = sum(((bits >> u) & 1) << c for u, c in enumerate(ring))
        segs = {tuple(G.face_segments(f, on_face))}
        for rest in range(16):
            case = on_face | sum(((rest >> u) & 1) << c for u, c in enumerate(others))
            segs.add(tuple(G.face_segments(f, case)))
            # ... and the case's triangles cross this face exactly along these segments
            tris = G.case_triangles(case)
            fe = set(f[4])
            on = {(a, b) for t in tris for a, b in zip(t, t[1:] + t[:1]) if a in fe and b in fe}
            for a, b in G.face_segments(f, case):
                assert (a, b) in on or any((a, b) in zip(lp, lp[1:] + lp[:1]) for lp in G.case_loops(case))
        assert len(segs) == 1


def _fixture(golden, tag):
    z = golden("g18_mcubes")
    return z, z[f"{tag}.vol"], float(z[f"{tag}.level"]), z[f"{tag}.spacing"].astype(np.float64)


@pytest.mark.parametrize("tag,vol_tol,ang_mean,ang_max", [("a", 1e-4, 1.0, 5.0), ("b", 5e-4, 1.25, 5.0)])
def test_restatement_against_scikit_image(golden, tag, vol_tol, ang_mean, ang_max):
    """Smooth volumes: the same vertices as scikit-image (one per crossing edge, same interpolation), the same face count, a
    closed mesh of the same Euler characteristic, area / signed volume / normals close.  The triangulations differ by the
    quad diagonals of the two case tables (an O(spacing^2) effect on the volume, ~2e-4 on the 7.5-cell-thick torus of (b)),
    and scikit-image's normals are the gradient of the volume's INDEX space (spacing only scales its vertices): they are
    compared after dividing by the spacing.  On (b) ours are within 0.2 deg mean of the torus's exact normal, scikit-image's
    about 1 deg (checked below)."""
    z, vol, level, sp = _fixture(golden, tag)
    v, f, n = R.marching_cubes(vol, level, sp)
    sv, sf, sn = z[f"{tag}.verts"], z[f"{tag}.faces"], z[f"{tag}.normals"]
    ko, ks = R.edge_keys(vol.shape, v, sp, (0, 0, 0)), R.edge_keys(vol.shape, sv, sp, (0, 0, 0))
    assert np.array_equal(np.sort(ks), ko), "vertex sets differ"
    idx = np.searchsorted(ko, ks)
    assert np.abs(v[idx].astype(np.float64) - sv).max() <= 1e-5 * sp.min()
    assert f.shape == sf.shape and f.dtype == np.int32
    area, svol, euler, closed, directed = R.mesh_stats(v, f)
    s_area, s_svol, s_euler, s_closed, _ = R.mesh_stats(sv, sf)
    assert closed and directed and s_closed and euler == s_euler
    assert abs(area / s_area - 1) <= 1e-4
    assert abs(svol / s_svol - 1) <= vol_tol and svol > 0           # SDF negative inside: positive signed volume
    g = sn / sp
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((n[idx] * g).sum(1), -1, 1)))
    assert ang.mean() <= ang_mean and ang.max() <= ang_max, (ang.mean(), ang.max())
    if tag == "b":
        c = (np.array(vol.shape) - 1) / 2 * sp
        x, y, zz = (v.astype(np.float64) - c).T
        rho = np.hypot(x, y)
        Rt = float(z["b.torus_R"])
        q = np.stack([x * (1 - Rt / rho), y * (1 - Rt / rho), zz], 1)
        exact = -q / np.linalg.norm(q, axis=1, keepdims=True)
        ang = np.degrees(np.arccos(np.clip((n * exact).sum(1), -1, 1)))
        assert ang.mean() <= 0.25 and ang.max() <= 1.0, (ang.mean(), ang.max())


def test_restatement_on_ambiguous_cells_is_closed_and_oriented(golden):
    z, vol, level, sp = _fixture(golden, "c")
    v, f, n = R.marching_cubes(vol, level, sp)
    area, svol, euler, closed, directed = R.mesh_stats(v, f)
    assert closed and directed
    assert len(np.unique(f)) == len(v)                               # every vertex is used
    assert svol > 0                                                  # positive border: the surface encloses the "below" side


def test_restatement_empty_and_degenerate():
    v, f, n = R.marching_cubes(np.ones((3, 4, 5), np.float32))
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    vol = np.pad(np.random.default_rng(1).integers(-1, 2, (6, 5, 7)).astype(np.float32), 1, constant_values=1.0)
    v, f, n = R.marching_cubes(vol, 0.0)                              # many values equal the level exactly
    area, svol, euler, closed, directed = R.mesh_stats(v, f)
    assert closed and directed
