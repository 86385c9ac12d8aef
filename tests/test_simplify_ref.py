"""CPU: the numpy restatement tests/simplify_ref.py of the mesh-simplification law (include/i2sdf.h, "Mesh simplification") held to
properties that do not depend on it: `average` is a plain fp64 cell mean; on a cube the quadric representative keeps faces, edges and
corners where the mean rounds them off; the clustered icosphere is a closed surface of Euler number 2; a mesh shifted by +1000 gives the
same result up to the fp32 rounding of its coordinates; and the restatement tells five mutations of the law apart."""
import numpy as np
import pytest

import pointops_ref as P
import raycast_ref as R
import simplify_ref as S

F32, D = np.float32, np.float64


@pytest.fixture(scope="module")
def cube32():
    v, f = S.cube(32)
    return v, f, {c: S.simplify(v, f, 0.2, c, detail=True) for c in ("quadric", "average")}


@pytest.fixture(scope="module")
def ico5():
    return R.icosphere(5)


def test_average_is_a_plain_cell_mean_and_voxel_down_sample(cube32, ico5):
    for (v, f), h in ((cube32[:2], 0.2), (ico5, 0.25), (R.soup(500, seed=4), 0.3)):
        res = S.simplify(v, f, h, "average", detail=True)
        mean, cell = S.plain_cell_mean(v, h)
        assert np.array_equal(cell, res["cell"])
        # two fp64 sums of the same <= V terms in different orders: |difference| <= 2 V 2^-53 sum |x|, then one fp32 rounding each
        err = np.abs(res["cell_verts"].astype(D) - mean).max()
        assert err <= 2.0 ** -23 * np.abs(v).max(), err
        down, counts = P.voxel_down_sample(v, h)
        assert np.array_equal(down.view(np.int32), res["cell_verts"].view(np.int32))             # every cell, bit for bit
        assert np.array_equal(res["verts"].view(np.int32), down[np.unique(cell[f][res["face_map"]])].view(np.int32))
        assert not res["fallback"].any()


def test_quadric_keeps_the_cube_where_the_mean_rounds_it_off(cube32):
    v, f, res = cube32
    assert v.shape == (6146, 3) and f.shape == (12288, 3)
    q, a = res["quadric"], res["average"]
    assert len(q["verts"]) == 602 and len(q["faces"]) == 1200 and np.array_equal(q["faces"], a["faces"])
    topo = S.topology(q["verts"], q["faces"])
    assert topo["watertight"] and topo["oriented"] and topo["manifold_edges"] == 1800 and topo["euler"] == 2
    assert int(q["fallback"].sum()) == 0                      # the cap that keeps the comparison honest: no cell fell back to the mean
    dq, da = S.cube_surface_distance(q["verts"]).max(), S.cube_surface_distance(a["verts"]).max()
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], D)
    near = lambda p: max(np.linalg.norm(p.astype(D) - c, axis=1).min() for c in corners)
    cq, ca = near(q["verts"]), near(a["verts"])
    print(f"cube 32x32, h = 0.2: largest distance to the surface quadric {dq:.2e}, average {da:.2e} (ratio {da / dq:.0f}); "
          f"farthest true corner from its nearest vertex: quadric {cq:.2e}, average {ca:.2e}")
    assert da >= 100.0 * dq and ca >= 100.0 * cq
    # the bias scales with reg
    q6 = S.simplify(v, f, 0.2, "quadric", reg=1e-6)
    assert S.cube_surface_distance(q6["verts"]).max() < 1e-2 * dq and int(q6["fallback"].sum()) == 0


def test_icosphere_clusters_into_a_closed_surface(ico5):
    v, f = ico5
    assert v.shape == (10242, 3) and f.shape == (20480, 3)
    res = S.simplify(v, f, 0.25)
    topo = S.topology(res["verts"], res["faces"])
    print(f"icosphere(5), h = 0.25: {len(res['verts'])} cells, {len(res['faces'])} faces, {topo}")
    assert len(res["verts"]) == 314 and len(res["faces"]) == 624
    assert topo["euler"] == 2 and topo["watertight"] and topo["oriented"] and topo["manifold_edges"] == 936
    fine = S.simplify(v, f, 0.1)
    t2 = S.topology(fine["verts"], fine["faces"])
    print(f"icosphere(5), h = 0.1: {len(fine['verts'])} cells, {len(fine['faces'])} faces, {t2}, fallback share {fine['fallback'].mean():.4f}")
    assert t2["boundary_edges"] == 0 and t2["nonmanifold_edges"] > 0 and not t2["watertight"]      # clustering does not preserve manifoldness
    assert fine["fallback"].mean() < 0.05
    # the maps
    assert (res["vertex_map"] >= 0).all() and res["vertex_map"].max() == len(res["verts"]) - 1
    assert np.array_equal(res["vertex_map"][f[res["face_map"]]], res["faces"])


def test_a_shift_by_1000_changes_nothing_but_the_rounding(ico5):
    # coordinates that stay exact under the shift (multiples of 2^-10 below 2, + 1000 fits 24 bits): the grid, the quadrics about the
    # cell centre and the solve then see the same numbers up to the rounding of lo and cc, and the output differs by the fp32 rounding
    # of a coordinate near 1000 (2^-14 an ulp) plus the amplified rounding of the solve
    for (v, f), h in ((S.cube(16), 0.25), (ico5, 0.25)):
        v = (np.round(v.astype(D) * 1024) / 1024).astype(F32)
        a = S.simplify(v, f, h)
        b = S.simplify(S.shift(v, 1000.0), f, h)
        assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["vertex_map"], b["vertex_map"])
        assert np.array_equal(a["face_map"], b["face_map"]) and np.array_equal(a["fallback"], b["fallback"])
        err = np.abs((b["verts"].astype(D) - 1000.0) - a["verts"].astype(D)).max()
        assert err <= 2.0 ** -14, err                            # one fp32 ulp at 1000 is 2^-14 (half of it the rounding, the rest slack)


def test_the_restatement_tells_the_mutations_apart(ico5):
    v, f = ico5
    base = S.simplify(v, f, 0.25)
    radius = lambda r: np.abs(np.linalg.norm(r["verts"].astype(D), axis=1) - 1.0).max()
    once = S.simplify(v, f, 0.25, mutate="once_per_cell")
    print(f"icosphere(5), h = 0.25: max | |p| - 1 | per corner {radius(base):.2e}, once per cell {radius(once):.2e}")
    assert radius(base) < radius(once)                           # the header's choice is the better one here
    assert not np.array_equal(base["verts"], once["verts"])
    rnd = S.simplify(v, f, 0.25, mutate="round_for_floor")
    assert len(rnd["verts"]) != len(base["verts"]) or not np.array_equal(rnd["faces"], base["faces"])
    # faces: a folded sheet (opposite duplicates) and rotated duplicates
    sv, sf = S.folded_sheet(6)
    keep = S.simplify(sv, sf, 0.2)
    merged = S.simplify(sv, sf, 0.2, mutate="merge_opposite")
    assert len(keep["faces"]) == 2 * len(merged["faces"]) > 0
    dv, df = R.icosphere(2)
    dup = S.duplicated_shuffled(df)
    a, b = S.simplify(dv, dup, 0.2), S.simplify(dv, dup, 0.2, mutate="largest_face_kept")
    assert len(a["faces"]) == len(b["faces"]) and not np.array_equal(a["face_map"], b["face_map"])
    assert (a["face_map"] <= b["face_map"][np.argsort(np.argsort(a["face_map"]))]).all() or a["face_map"].sum() < b["face_map"].sum()
    # the clamp: at h = 0.1 some cells hold a sliver of the sphere whose minimiser lies outside them
    c0, c1 = S.simplify(v, f, 0.1, detail=True), S.simplify(v, f, 0.1, mutate="no_clamp", detail=True)
    assert c0["cell_fallback"].any() and not c1["cell_fallback"].any()
    assert not np.array_equal(c0["cell_verts"], c1["cell_verts"])
    half = 0.05 * (1 + 1e-6)
    assert (np.abs(c0["cell_verts"].astype(D) - c0["centres"]) <= half).all() and not (np.abs(c1["cell_verts"].astype(D) - c1["centres"]) <= half).all()
    assert set(S.MUTATIONS) == {"once_per_cell", "merge_opposite", "largest_face_kept", "no_clamp", "round_for_floor"}


def test_clean_and_topology_restatements():
    v, f = R.icosphere(2)
    t = S.topology(v, f)
    assert t["watertight"] and t["oriented"] and t["euler"] == 2 and t["edges"] == 480 and t["referenced_vertices"] == 162
    cv, cf = S.cube_without_top(8)
    t = S.topology(cv, cf)
    assert not t["watertight"] and t["oriented"] and t["boundary_edges"] == 32 and t["euler"] == 1
    flipped = f.copy()
    flipped[5] = flipped[5, [0, 2, 1]]
    t = S.topology(v, flipped)
    assert t["watertight"] and not t["oriented"] and t["misoriented_edges"] == 3
    # clean: a soup of the icosphere's faces (every vertex repeated per face) with -0.0, a degenerate, a zero-area and duplicates mixed in
    sv = v[f].reshape(-1, 3).copy()
    sv[sv == 0.0] = -0.0
    sf = np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)
    extra = np.array([[0, 0, 1], [0, 3, 0]], np.int32)                       # repeated indices
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], F32)                 # three points on a line: exactly zero ab x ac
    sv2 = np.concatenate([sv, line, np.array([[9, 9, 9]], F32)], 0)          # ... and an unreferenced vertex
    n0 = len(sv)
    sf2 = np.concatenate([sf[:10], extra, sf[10:], [[n0, n0 + 1, n0 + 2]], sf[[4, 7]][:, [1, 2, 0]], sf[[9]][:, [0, 2, 1]]], 0).astype(np.int32)
    res = S.clean(sv2, sf2)
    assert len(res["verts"]) == 162 and len(res["faces"]) == len(f) + 1       # the opposite duplicate stays
    t = S.topology(res["verts"], res["faces"])
    assert t["repeated_index_faces"] == 0 and t["nonmanifold_edges"] == 3
    assert np.array_equal(res["verts"][res["faces"]].reshape(-1, 3) == 0, sv2[sf2[res["face_map"]]].reshape(-1, 3) == 0)
    assert np.array_equal(np.abs(res["verts"][res["faces"]]), np.abs(sv2[sf2[res["face_map"]]]))
    assert res["vertex_map"][-1] == -1 and (res["vertex_map"][:n0] >= 0).all()
    untouched = S.clean(sv2, sf2, merge_vertices=False, degenerate=False, zero_area=False, duplicated=False)
    assert len(untouched["faces"]) == len(sf2) and len(untouched["verts"]) == len(sv2) - 1
