"""CPU: the numpy restatement of the closest-point law (tests/closest_ref.py) against an independent formulation of the distance,
against closed forms, against the exact convex test (sharp wedge) and against crossing parity (non-convex star); and the mutations
of the law the suite must tell from it."""
import numpy as np
import pytest

import closest_ref as CR
import raycast_ref as R

D = np.float64


def _fixtures():
    yield "icosphere2", R.icosphere(2)
    yield "soup", R.soup(300, seed=3)
    yield "wedge", CR.wedge()
    yield "bumpy", CR.bumpy_sphere(2)
    v, f = R.flat_grid(6)
    yield "grid+1000", ((v.astype(D) + 1000.0).astype(np.float32), f)


@pytest.mark.parametrize("name,mesh", list(_fixtures()), ids=[n for n, _ in _fixtures()])
def test_rule_equals_an_independent_formulation(name, mesh):
    v, f = mesh
    q = CR.queries(v, f, 250, seed=1, special=False)
    got = CR.closest(v, f, q)
    ind = CR.independent_d2(v, f, q)
    want = np.nanmin(ind, 1)
    rel = np.abs(got["d2"] - want) / want
    assert (np.abs(got["d2"] - want) <= 1e-12 * want).all(), (name, rel.max())
    srt = np.sort(ind, 1)
    clear = srt[:, 1] - srt[:, 0] > 1e-9
    assert clear.sum() > 30                     # (on the wedge most closest points lie on an edge two faces share)
    assert np.array_equal(got["face"][clear], np.nanargmin(ind, 1)[clear]), name
    assert (got["face"] >= 0).all() and got["status"] == 0


def test_icosphere_distance_lies_between_the_spheres():
    v, f = R.icosphere(2)
    P = v[f].astype(D)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    r_in = (np.abs((P[:, 0] * n).sum(1)) / np.linalg.norm(n, axis=1)).min()
    assert 0.0 < 1.0 - r_in <= 0.0178
    g = np.random.default_rng(2)
    p = g.normal(size=(500, 3))
    p *= (g.uniform(1.05, 4.0, (500, 1)) / np.linalg.norm(p, axis=1, keepdims=True))
    p = p.astype(np.float32)
    got = CR.closest(v, f, p)
    r = np.linalg.norm(p.astype(D), axis=1)
    d = np.sqrt(got["d2"])
    # (the vertices are fp32 roundings of unit vectors: 1e-7 of room on the outer sphere)
    assert (d >= r - 1.0 - 1e-7).all() and (d <= r - r_in + 1e-12).all(), ((r - 1 - d).max(), (d - (r - r_in)).max())


def test_the_seven_regions_of_one_triangle():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    q = np.array([[0.5, 0.5, 1.0], [1.0, -1.0, 0.5], [2.0, 2.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, -1.0, 2.0], [3.0, -0.5, 0.0],
                  [-0.5, 3.0, 0.0]], np.float32)
    got = CR.closest(v, f, q)
    assert got["feature"].tolist() == [CR.FACE, CR.EDGE_AB, CR.EDGE_BC, CR.EDGE_CA, CR.VERT_A, CR.VERT_B, CR.VERT_C]
    want_c = [[0.5, 0.5, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0], [2, 0, 0], [0, 2, 0]]
    assert np.array_equal(got["point"], np.array(want_c, np.float32))
    assert np.allclose(got["d2"], [1.0, 1.25, 2.0, 1.0, 6.0, 1.25, 1.25], rtol=0, atol=1e-15)
    assert np.array_equal(got["bary"], np.array([[0.5, 0.25], [0.5, 0.5], [0, 0.5], [0.5, 0], [1, 0], [0, 1], [0, 0]], np.float32))
    # the point is the weighted sum of the vertices
    w = np.concatenate([got["bary"], 1 - got["bary"].sum(1, keepdims=True)], 1).astype(D)
    assert np.allclose(w @ v.astype(D), got["c"], atol=1e-15)


def test_max_dist_misses_and_status_bits():
    v, f = R.icosphere(1)
    q = np.array([[0, 0, 1.5], [0, 0, 3.0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    got = CR.closest(v, f, q, max_dist=0.7)
    assert got["face"][0] >= 0 and got["face"][1:3].tolist() == [-1, -1] and got["status"] == CR.BAD_POINT
    assert np.isinf(got["dist"][1:3]).all() and not got["point"][1:3].any() and not got["bary"][1:3].any()
    e = CR.closest(v, np.zeros((0, 3), np.int32), q)
    assert (e["face"] == -1).all() and np.isinf(e["dist"]).all() and e["status"] == CR.BAD_POINT
    vb, fb = CR.with_bad_faces(v, f)
    b = CR.closest(vb, fb, q[:2])
    assert b["status"] == CR.BAD_FACE and np.array_equal(b["dist"], CR.closest(v, f, q[:2])["dist"])


def _wedge_queries():
    g = np.random.default_rng(4)
    v, f = CR.wedge()
    far = g.uniform([-0.3, -0.4, -0.3], [1.3, 0.4, 1.3], (800, 3))
    P = v[f].astype(D)
    w = g.dirichlet([1, 1, 1], 800)
    k = g.integers(0, len(f), 800)
    near = (P[k] * w[:, :, None]).sum(1) + g.normal(0, 0.03, (800, 3))
    return np.concatenate([far, near]).astype(np.float32)


def test_sign_on_the_sharp_wedge_is_the_exact_convex_test():
    v, f = CR.wedge()
    q = _wedge_queries()
    inside, well = CR.wedge_inside(q)
    nm = CR.pseudonormals(v, f)
    got = CR.closest(v, f, q, normals=nm)
    assert len(q) == 1600 and well.sum() > 1500 and 100 < inside.sum() < 1500
    assert int(((got["sdist"] < 0) != inside)[well].sum()) == 0
    assert np.array_equal(np.abs(got["sdist"]), got["dist"])
    mut = CR.closest(v, f, q, normals=nm, mutate="face_normal_everywhere")
    assert int(((mut["sdist"] < 0) != inside)[well].sum()) > 50          # the fixture tells the face normal from the pseudonormal


def test_sign_on_a_non_convex_star_is_the_crossing_parity():
    v, f = CR.bumpy_sphere(2)
    g = np.random.default_rng(7)
    q = g.uniform(-1.7, 1.7, (600, 3)).astype(np.float32)
    inside, well = CR.parity_inside(v, f, q, seed=8)
    got = CR.closest(v, f, q, normals=CR.pseudonormals(v, f))
    assert well.sum() > 550 and 50 < inside.sum() < 500
    assert int(((got["sdist"] < 0) != inside)[well].sum()) == 0


def test_tables_are_sums_over_the_faces_that_may_be_closest():
    v, f = R.icosphere(1)
    vn, en = CR.pseudonormals(v, f)
    # on a sphere every pseudonormal points outward, and a manifold edge's entry is the same from both faces
    assert ((vn * v).sum(1) > 0).all()
    mid = (v[f] + v[np.roll(f, -1, 1)]) / 2
    assert ((en * mid).sum(2) > 0).all()
    vb, fb = CR.with_bad_faces(v, f)
    vn2, en2 = CR.pseudonormals(vb, fb)
    good, _ = CR.countable_faces(vb, fb)
    assert np.array_equal(vn2[:len(v)], vn) and not vn2[len(v):].any() and not en2[~good].any()
    lookup = {tuple(t): e for t, e in zip(f.tolist(), en)}
    assert all(np.array_equal(en2[i], lookup[tuple(fb[i].tolist())]) for i in np.nonzero(good)[0])


def test_the_suite_tells_the_mutations_from_the_law():
    seen = {}
    v, f = CR.duplicated(*R.icosphere(1))
    q = CR.queries(v, f, 100, seed=3)
    law = CR.closest(v, f, q)
    seen["largest_face_wins"] = int((CR.closest(v, f, q, mutate="largest_face_wins")["face"] != law["face"]).sum())
    v, f = R.icosphere(1)
    onv = v[:10]
    seen["max_dist_exclusive"] = int((CR.closest(v, f, onv, 0.0, mutate="max_dist_exclusive")["face"] != CR.closest(v, f, onv, 0.0)["face"]).sum())
    assert (CR.closest(v, f, onv, 0.0)["face"] >= 0).all()
    seen["unclamped_plane"] = int((CR.closest(v, f, q, mutate="unclamped_plane")["dist"] != CR.closest(v, f, q)["dist"]).sum())
    vb, fb = CR.with_bad_faces(v, f)
    ql = np.array([[0.5, 0.5, 0.5], [1, 1, 1], [0.8, 0.8, 0.8]], np.float32)
    seen["degenerate_kept"] = int((CR.closest(vb, fb, ql, mutate="degenerate_kept")["dist"] != CR.closest(vb, fb, ql)["dist"]).sum())
    wv, wf = CR.wedge()
    wq = _wedge_queries()
    nm = CR.pseudonormals(wv, wf)
    seen["face_normal_everywhere"] = int((CR.closest(wv, wf, wq, normals=nm, mutate="face_normal_everywhere")["sdist"]
                                          != CR.closest(wv, wf, wq, normals=nm)["sdist"]).sum())
    assert set(seen) == set(CR.MUTATIONS)
    assert all(n > 0 for n in seen.values()), seen


@pytest.mark.parametrize("max_dist", [0.0, 0.05, 0.4])
def test_max_dist_only_cuts_the_unbounded_result(max_dist):
    v, f = CR.with_bad_faces(*R.icosphere(1))
    q = CR.queries(v, f, 200, seed=9)
    nm = CR.pseudonormals(v, f)
    a, b = CR.closest(v, f, q, max_dist, normals=nm), CR.limit(CR.closest(v, f, q, normals=nm), max_dist)
    for k in ("dist", "point", "face", "bary", "feature", "sdist"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert 0 < (a["face"] >= 0).sum() < len(q)
