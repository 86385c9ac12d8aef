"""CPU: the numpy restatement of the ray-casting law (tests/raycast_ref.py; include/i2sdf.h, "Ray casting") against closed forms, its
watertightness in fp32, and its power to tell the law from four near misses of it."""
import numpy as np
import pytest

import raycast_ref as R

F32 = np.float32


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_sphere_depth_is_approached_as_the_icosphere_is_refined():
    g = np.random.default_rng(1)
    o = np.tile(np.array([[0.3, 0.1, -0.2]]), (400, 1))
    d = _unit(g.normal(size=(400, 3)))
    b = (o * d).sum(1)
    t_true = -b + np.sqrt(b * b - (o * o).sum(1) + 1.0)       # |o + t d| = 1 from inside
    errs = []
    for s in (0, 1, 2, 3):
        v, f = R.icosphere(s)
        out = R.trace(v, f, o, d, dt=F32)
        assert out["hit"].all() and out["status"] == 0
        e = t_true - out["t"]
        assert (e > -1e-5).all()                               # the inscribed polyhedron is never farther than the sphere
        errs.append(float(np.abs(e).max()))
    assert errs[0] > errs[1] > errs[2] > errs[3] and errs[3] < 0.02, errs
    assert errs[3] < errs[2] / 3 and errs[2] < errs[1] / 3     # second order in the edge length: about 4 per subdivision


def test_plane_depth_barycentrics_and_units_of_the_direction():
    v, f = R.flat_grid()
    o = np.array([[0.1, -0.3, -1.0], [0.1, -0.3, -1.0], [0.1, -0.3, 2.0]])
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 4.0], [0.0, 0.0, -0.5]])
    out = R.trace(v, f, o, d, dt=F32)
    assert out["hit"].all() and np.array_equal(out["t"], np.array([1.5, 0.375, 3.0], F32))      # t in units of d
    for i in range(3):
        A, B, C = v[f[out["face"][i]]].astype(np.float64)
        u, w = out["bary"][i].astype(np.float64)
        p = u * A + w * B + (1 - u - w) * C
        assert np.abs(p - (o[i] + out["t"][i] * d[i])).max() < 1e-6
    miss = R.trace(v, f, o[:1], d[:1], t_max=1.25, dt=F32)
    assert not miss["hit"][0] and miss["face"][0] == -1 and miss["t"][0] == F32(1.25) and (miss["bary"] == 0).all()
    assert R.trace(v, f, o[:1], d[:1], t_max=1.5, dt=F32)["hit"][0]                              # t <= t_max counts


def test_back_faces_are_those_whose_right_hand_normal_points_along_the_ray():
    v, f = R.soup(200, seed=3)
    g = np.random.default_rng(4)
    o, d = g.uniform(-1, 1, (300, 3)), g.normal(size=(300, 3))
    Rr = R.ray_shear(o.astype(F32), d.astype(F32), F32)
    for k in range(0, 200, 7):
        A, B, C = v[f[k]]
        ok, _, _, _, det = R.tri_hit(Rr, A, B, C, F32(-np.inf), F32(np.inf), "none", F32)
        nd = np.cross(B.astype(np.float64) - A, C.astype(np.float64) - A) @ d.T
        assert (np.sign(det[ok]) == -np.sign(nd[ok])).all()
    # an outward-wound sphere seen from inside shows only back faces
    sv, sf = R.icosphere(1)
    n = np.cross(sv[sf[:, 1]] - sv[sf[:, 0]], sv[sf[:, 2]] - sv[sf[:, 0]])
    assert ((n * sv[sf].mean(1)).sum(1) > 0).all()
    inside = R.trace(sv, sf, np.zeros((50, 3)), _unit(g.normal(size=(50, 3))), cull="back", dt=F32)
    assert not inside["hit"].any()
    outside = R.trace(sv, sf, np.tile([[0.0, 0.0, 3.0]], (5, 1)), np.tile([[0.0, 0.0, -1.0]], (5, 1)), cull="back", dt=F32)
    assert outside["hit"].all() and (outside["t"] < 2.3).all()


def test_bad_rays_bad_faces_and_zero_area_faces():
    v, f = R.flat_grid(4)
    v = np.concatenate([v, [[np.nan, 0, 0]]]).astype(F32)
    f = np.concatenate([f, [[0, 1, 99], [0, 1, len(v) - 1], [0, 0, 6], [0, 6, 12]]]).astype(np.int32)   # out of range, NaN, repeated, collinear
    o = np.array([[0.1, 0.2, -1.0]] * 5)
    d = np.array([[0, 0, 1.0], [0, 0, 0], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, 1.0]])
    o[4, 0] = np.inf
    out = R.trace(v, f, o, d, dt=F32)
    assert out["status"] == (R.BAD_RAY | R.BAD_FACE) and out["hit"].tolist() == [True, False, False, False, False]
    assert out["face"][0] < 32
    assert R.trace(v, f[:32], o[:1], d[:1], t_min=np.nan, dt=F32)["status"] == R.BAD_RAY
    # rays through the diagonal 0 - 6 - 12 hit the grid faces, never the degenerate ones laid over them
    t = np.linspace(-0.9, -0.1, 9)
    oo = np.stack([t, t, np.full(9, -1.0)], 1)
    deg = R.trace(v, f[-2:], oo, np.tile([[0, 0, 1.0]], (9, 1)), dt=F32)
    assert not deg["hit"].any()


def _watertight_cases():
    sv, sf = R.icosphere(2)
    tg = R.watertight_targets(sv, sf)
    o = np.tile([[0.31, -0.17, 0.23]], (len(tg), 1))
    yield "icosphere", sv, sf, o, tg - o
    gv, gf = R.flat_grid()
    tg = R.watertight_targets(gv, gf, interior_only=True)
    o = np.tile([[0.37, -0.53, -1.3]], (len(tg), 1))
    yield "grid_oblique", gv, gf, o, tg - o
    o = tg - np.array([[0.0, 0.0, 1.5]])
    yield "grid_axis", gv, gf, o, np.tile([[0.0, 0.0, 1.0]], (len(tg), 1))


def test_the_restatement_is_watertight_in_fp32():
    counts = {}
    for name, v, f, o, d in _watertight_cases():
        out = R.trace(v, f, o, d, dt=F32)
        counts[name] = len(o)
        assert out["hit"].all(), (name, int((~out["hit"]).sum()))
    assert counts["icosphere"] == 162 + 4 * 480 and counts["grid_oblique"] == counts["grid_axis"] > 2000, counts


def test_ties_go_to_the_smaller_face_and_the_mutation_is_detected():
    _, v, f, o, d = list(_watertight_cases())[2]               # axis-parallel rays at interior vertices and edge points
    law = R.trace(v, f, o, d, dt=F32)
    mut = R.trace(v, f, o, d, dt=F32, mutate="largest_face_wins")
    T, _ = R.all_hits(v, f, o, d, 0.0, np.inf, dt=np.float32)
    T = np.where(np.isnan(T), np.inf, T)
    tied = (T == T.min(1, keepdims=True)).sum(1) >= 2           # (two faces at an edge may also differ in the last place of T / det)
    assert tied.sum() >= 15 * 15                                # at every interior vertex the arithmetic is exact: six faces at t = 1.5
    assert np.array_equal(law["t"], mut["t"]) and np.array_equal(law["t"], T.min(1)) and (law["t"][:225] == F32(1.5)).all()
    assert (law["face"][tied] < mut["face"][tied]).all() and np.array_equal(law["face"][~tied], mut["face"][~tied])
    assert np.array_equal(law["face"], T.argmin(1))             # the first face among the tied ones
    perm = np.random.default_rng(0).permutation(len(f))
    shuf = R.trace(v, f[perm], o, d, dt=F32)
    assert np.array_equal(shuf["t"], law["t"]) and not np.array_equal(perm[shuf["face"]], law["face"])     # the INDEX decides, not the face


def test_t_min_is_exclusive_and_the_mutation_is_detected():
    v, f = R.flat_grid()
    o, d = np.array([[0.1, 0.3, -1.0]]), np.array([[0.0, 0.0, 1.0]])
    assert R.trace(v, f, o, d, dt=F32)["t"][0] == F32(1.5)
    assert not R.trace(v, f, o, d, t_min=1.5, dt=F32)["hit"][0]
    assert R.trace(v, f, o, d, t_min=1.5, dt=F32, mutate="t_min_inclusive")["hit"][0]
    assert R.trace(v, f, o, d, t_min=np.nextafter(F32(1.5), F32(0)), dt=F32)["hit"][0]


def test_the_fp64_recomputation_decides_a_ray_in_an_edges_plane_and_the_mutation_is_detected():
    """Two faces share the edge BC; the ray (0, 0, -1) + t (0, 0, 1) passes the edge's plane at a distance of 2^-24 of the products:
    Cx By = -(1 + 2^-12)^2 rounds to -(1 + 2^-11) = Cy Bx, so fp32 sees U = 0 on BOTH faces.  Exactly, U = -2^-24 on the first face
    (outside) and +2^-24 on the second (inside): with the recomputation one face is hit, without it both claim the ray."""
    e = 2.0 ** -12
    B, C = (-(1 + 2 * e), -(1 + e), 0.0), (1 + e, 1.0, 0.0)
    v = np.array([(1.0, -1.0, 0.0), B, C, (-1.0, 1.0, 0.0)], F32)
    f = np.array([[0, 1, 2], [3, 2, 1]], np.int32)
    o, d = np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])
    o[0, 2] = -1.0
    Rr = R.ray_shear(o.astype(F32), d.astype(F32), F32)
    hits = {m: [bool(R.tri_hit(Rr, *v[f[k]], F32(0), F32(np.inf), "none", F32, m)[0][0]) for k in range(2)] for m in (None, "no_fp64")}
    assert hits[None] == [False, True] and hits["no_fp64"] == [True, True]
    assert R.trace(v, f, o, d, dt=F32)["face"][0] == 1 and R.trace(v, f, o, d, dt=F32, mutate="no_fp64")["face"][0] == 0
    # exactly in the plane (all of it representable): both faces see U = 0, the tie goes to face 0, with and without the recomputation
    v2 = np.array([(1.0, -1.0, 0.0), (-1.0, -1.0, 0.0), (1.0, 1.0, 0.0), (-1.0, 1.0, 0.0)], F32)
    both = R.all_hits(v2, f, o, d, 0.0, np.inf, dt=np.float32)[0]
    assert np.array_equal(both, [[1.0, 1.0]]) and R.trace(v2, f, o, d, dt=F32)["face"][0] == 0


def test_det_zero_is_rejected_and_why_accepting_it_could_not_be_told_apart():
    """U, V, W of one sign sum to 0 only when all three are 0 (a sum of same-signed floats never cancels), and then T = 0 and t = 0 / 0 is
    NaN, which fails t_min < t.  So `det == 0 accepted` is the one mutation of the four that no input can expose through the result:
    this test holds the law's side (degenerate faces are never hit, with finite and infinite bounds) and checks that reason."""
    v = np.array([(-1, -1, 0), (1, 1, 0), (0, 0, 0), (1, 1, 0)], F32)
    f = np.array([[0, 1, 2], [0, 1, 1], [0, 3, 1]], np.int32)       # collinear, repeated, repeated through two indices
    t = np.linspace(-0.75, 0.75, 7)
    o = np.stack([t, t, np.full(7, -1.0)], 1)
    d = np.tile([[0.0, 0.0, 1.0]], (7, 1))
    for mutate in (None, "det_zero_ok"):
        for bounds in ((0.0, np.inf), (-np.inf, np.inf)):
            assert not R.trace(v, f, o, d, *bounds, dt=F32, mutate=mutate)["hit"].any()
    Rr = R.ray_shear(o.astype(F32), d.astype(F32), F32)
    _, tt, _, _, det = R.tri_hit(Rr, *v[f[0]], F32(-np.inf), F32(np.inf), "none", F32, "det_zero_ok")
    assert (det == 0).all() and np.isnan(tt).all()


def test_keys_and_topology():
    v, f = R.soup(300, seed=5)
    keys = R.morton_keys(v, f)
    assert len(np.unique(keys)) == 300 and (keys >> 62 == 0).all() and np.array_equal(keys & 0xffffffff, np.arange(300))
    sk = np.sort(keys)
    child = R.karras(sk)
    bx, seen = R.boxes(v, f, sk, child)
    assert (seen == 1).all()                                    # every leaf is reached exactly once
    internal = child[child >= 0]
    assert sorted(internal.tolist()) == list(range(1, 299))     # every internal node but the root is somebody's child, once
    P = v[f]
    assert np.array_equal(np.minimum(bx[0, 0, 0], bx[0, 1, 0]), P.min((0, 1))) and np.array_equal(np.maximum(bx[0, 0, 1], bx[0, 1, 1]), P.max((0, 1)))
    # Morton order: x is the highest bit -- the root splits the soup by x
    cx = P.mean(1)[:, 0]
    left = bx[0, 0]
    assert left[1, 0] < P.max((0, 1))[0] - 0.5 and cx.min() >= left[0, 0]
    for F in (1, 2, 3):
        c = R.karras(np.sort(R.morton_keys(v, f[:F])))
        assert c.shape == (F - 1, 2)
    assert R.karras(np.sort(R.morton_keys(v, f[:2]))).tolist() == [[-1, -2]]
    bad = f.copy()
    bad[7] = (0, 1, 10 ** 6)
    kb = R.morton_keys(v, bad)
    assert kb[7] >> 32 == 1 << 30 and np.sort(kb)[-1] == kb[7]
