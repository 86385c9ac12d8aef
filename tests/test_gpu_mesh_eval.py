"""GPU: scoring meshes on the device (csrc/pointops.hip; i2sdf_amd.mesh.voxel_down_sample / nearest_neighbors / evaluate) against
the numpy restatement (tests/pointops_ref.py), the committed scikit-learn KDTree distances (tests/golden/g20_mesh_eval.npz) and
torch.cdist in fp64.

Bars.  Distances are fp32 from fp32 differences: difference, square, sum of three and square root each round once, which bounds
the relative error of a distance by about 3.5 * 2^-24 = 2.1e-7; the bar is rtol 1e-6 (a factor of 5).  The returned index must be
a nearest neighbour up to the same bar: its fp64 distance <= (1 + 1e-6) x the true minimum.  Voxel sets, orders and counts are
integers and must be equal; the means follow a pinned order of additions: at most 1 fp32 ulp is allowed, 0 is expected and what
is seen is printed."""
import time

import numpy as np
import pytest
import torch

import pointops_ref as P

pytestmark = pytest.mark.gpu

RTOL = 1e-6
KEYS = ("Acc", "Comp", "Prec", "Recal", "F-score")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _room(n, seed, noise=0.0, size=(5.0, 4.0, 3.0)):
    """n seeded fp32 points on the six walls of a size[0] x size[1] x size[2] room (area-weighted), plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    sx, sy, sz = size
    areas = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    wall = rng.choice(6, size=n, p=areas / areas.sum())
    p = rng.random((n, 3)) * np.array(size)
    axis, side = wall // 2, wall % 2
    p[np.arange(n), axis] = side * np.array(size)[axis]
    if noise:
        p = p + rng.normal(0.0, noise, (n, 3))
    return p.astype(np.float32)


def _ulps(a, b):
    """Largest distance in fp32 ulps between two fp32 arrays (through the order-preserving integer image of a float)."""
    def image(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(image(a) - image(b)).max()) if np.asarray(a).size else 0


def _check_down_sample(pts, voxel, what):
    from i2sdf_amd.mesh import voxel_down_sample
    want_p, want_c = P.voxel_down_sample(pts, voxel)
    got_p, got_c = voxel_down_sample(_cuda(pts), voxel)
    assert got_p.dtype == torch.float32 and got_c.dtype == torch.int32 and got_p.is_cuda and got_c.is_cuda
    assert tuple(got_p.shape) == want_p.shape and tuple(got_c.shape) == want_c.shape, (got_p.shape, want_p.shape)
    assert np.array_equal(got_c.cpu().numpy(), want_c)                     # same voxels, same order, same counts
    gp = got_p.cpu().numpy()
    u = _ulps(gp, want_p)
    print(f"down-sample {what}: {pts.shape[0]} -> {gp.shape[0]} points, means differ by at most {u} fp32 ulp (0 expected, 1 allowed)")
    assert u <= 1
    again_p, again_c = voxel_down_sample(_cuda(pts), voxel)
    assert torch.equal(again_p, got_p) and torch.equal(again_c, got_c)     # bitwise, run to run
    return gp, want_p


# ---------------------------------------------------------------------------------------------- down-sample
@pytest.mark.parametrize("tag", ["a", "b"])
def test_down_sample_fixture(golden, tag):
    z = golden("g20_mesh_eval")
    gp, _ = _check_down_sample(golden("g18_mcubes")[f"{tag}.verts"], float(z["down_sample"]), f"fixture {tag}")
    assert gp.shape[0] == int(z["ds.n"][0 if tag == "a" else 1])


def test_down_sample_room():
    _check_down_sample(_room(200_000, seed=11, noise=0.004), 0.02, "room, voxel 0.02")


def test_down_sample_points_on_voxel_faces():
    """Coordinates on a lattice of 1/8 with voxel 1/4: (p - lo) / voxel is a whole number for every other lattice value, exactly,
    so half of the coordinates lie exactly on a voxel face (and belong to the upper voxel)."""
    rng = np.random.default_rng(12)
    pts = (rng.integers(0, 64, (50_000, 3)) / 8.0).astype(np.float32)
    pts[0] = 0.0
    t = (pts.astype(np.float64) + 0.125) / 0.25
    assert (t == np.floor(t)).mean() > 0.4
    _check_down_sample(pts, 0.25, "lattice on voxel faces")
    _check_down_sample(pts - np.float32(3.5), 0.25, "lattice on voxel faces, negative coordinates")


def test_down_sample_single_point_and_single_voxel():
    from i2sdf_amd.mesh import voxel_down_sample
    one = np.float32([[0.3, -1.7, 2.9]])
    gp, _ = _check_down_sample(one, 0.02, "single point")
    assert np.array_equal(gp, one)
    blob = (np.random.default_rng(13).random((30_000, 3)) * 0.4 + 1.0).astype(np.float32)
    blob[0] = 1.0                                                          # the minimum: the voxel is [0.5, 1.5)^3
    gp, _ = _check_down_sample(blob, 1.0, "all points in one voxel")
    assert gp.shape == (1, 3)
    out, counts = voxel_down_sample(torch.empty(0, 3, device="cuda"), 0.02)
    assert out.shape == (0, 3) and counts.shape == (0,) and counts.dtype == torch.int32


def test_down_sample_refuses_bad_input():
    from i2sdf_amd.lib import I2SDFError
    from i2sdf_amd.mesh import voxel_down_sample
    pts = _room(1000, seed=14)
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy()
        p[500, 1] = bad
        with pytest.raises(I2SDFError, match="finite"):
            voxel_down_sample(_cuda(p), 0.02)
    wide = pts.copy()
    wide[7, 0] = 1.0e6                                                     # 1e6 / 1e-3 = 1e9 voxels along x: beyond 21 bits
    with pytest.raises(I2SDFError, match="21 bits"):
        voxel_down_sample(_cuda(wide), 1e-3)
    ok, _ = voxel_down_sample(_cuda(wide), 1.0)                            # (2^20 voxels along x fit)
    assert ok.shape[0] > 1
    dev = _cuda(pts)
    for bad_size in (0.0, -0.02, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            voxel_down_sample(dev, bad_size)
    for bad_pts in (dev.double(), dev[:, :2], dev.reshape(-1), dev.cpu(), pts):
        with pytest.raises(ValueError):
            voxel_down_sample(bad_pts, 0.02)


# ---------------------------------------------------------------------------------------------- nearest neighbour
def _cdist_nn(query, ref):
    """fp64 reference on the GPU: torch.cdist in chunks of queries (the direct form: the matrix-multiplication form loses the
    small distances to cancellation) -> (dist (Q,) fp64, index (Q,) int64) numpy.  The direct form runs one workgroup of 256
    threads per pair and a launch holds fewer than 2^32 threads: a chunk is at most 2^23 pairs."""
    q = query.double() if torch.is_tensor(query) else _cuda(query).double()
    r = ref.double() if torch.is_tensor(ref) else _cuda(ref).double()
    chunk = max(1, min(2048, (1 << 23) // r.shape[0]))
    dist = torch.empty(q.shape[0], dtype=torch.float64, device="cuda")
    index = torch.empty(q.shape[0], dtype=torch.int64, device="cuda")
    for a in range(0, q.shape[0], chunk):
        d = torch.cdist(q[a:a + chunk], r, compute_mode="donot_use_mm_for_euclid_dist")
        dist[a:a + chunk], index[a:a + chunk] = d.min(dim=1)
    return dist.cpu().numpy(), index.cpu().numpy()


def _check_nn(query, ref, want_dist, what, want_index=None):
    """query, ref: numpy fp32.  want_dist: the true fp64 minimum distances."""
    from i2sdf_amd.mesh import nearest_neighbors
    dist, index = nearest_neighbors(_cuda(query), _cuda(ref))
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (query.shape[0],)
    d, i = dist.cpu().numpy().astype(np.float64), index.cpu().numpy().astype(np.int64)
    assert (i >= 0).all() and (i < ref.shape[0]).all()
    err = np.abs(d - want_dist) / np.maximum(want_dist, 1e-300)
    err[(want_dist == 0) & (d == 0)] = 0.0
    own = np.linalg.norm(query.astype(np.float64) - ref.astype(np.float64)[i], axis=1)        # fp64 distance of the returned index
    excess = float((own / np.maximum(want_dist, 1e-300))[want_dist > 0].max()) - 1.0 if (want_dist > 0).any() else 0.0
    print(f"nearest neighbour {what}: {query.shape[0]} x {ref.shape[0]}, dist rel err max {err.max():.2e} (bar {RTOL:.0e}), "
          f"returned index's fp64 distance exceeds the minimum by at most {excess:.2e} (bar {RTOL:.0e})")
    assert err.max() <= RTOL
    assert (own <= (1.0 + RTOL) * want_dist).all()
    if want_index is not None:
        assert np.array_equal(i, want_index)
    return d, i


@pytest.mark.parametrize("tag", ["raw", "ds"])
def test_nn_fixture_against_kdtree(golden, tag):
    v, z = golden("g18_mcubes"), golden("g20_mesh_eval")
    p, t = v["a.verts"], v["b.verts"]
    if tag == "ds":
        p, _ = P.voxel_down_sample(p, float(z["down_sample"]))
        t, _ = P.voxel_down_sample(t, float(z["down_sample"]))
    _check_nn(t, p, z[f"{tag}.dist1"], f"fixture {tag} trgt -> pred")
    _check_nn(p, t, z[f"{tag}.dist2"], f"fixture {tag} pred -> trgt")


@pytest.fixture(scope="module")
def rooms():
    """Two seeded clouds of 2e5 points on the walls of the same 5 x 4 x 3 room: `a` nearly on them, `b` with 3 cm of noise."""
    return _room(200_000, seed=21, noise=0.002), _room(200_000, seed=22, noise=0.03)


def test_nn_large_against_cdist(rooms):
    a, b = rooms
    want, _ = _cdist_nn(a, b)
    _check_nn(a, b, want, "rooms a -> b")


def test_nn_duplicates_and_ties_take_the_smallest_index():
    rng = np.random.default_rng(23)
    # a shuffled 16^3 lattice, every point stored three times at scattered positions
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    ref = np.concatenate([g, g, g])[rng.permutation(3 * g.shape[0])]
    # queries on the points (distance 0, three candidates), on edge / face / cell centres (2, 4, 8 x 3 exact ties in fp32), and
    # outside the lattice
    q = np.concatenate([g[rng.choice(g.shape[0], 2000)], g[rng.choice(g.shape[0], 2000)] + np.float32([0.5, 0, 0]),
                        g[rng.choice(g.shape[0], 2000)] + np.float32([0.5, 0.5, 0]), g[rng.choice(g.shape[0], 2000)] + np.float32(0.5),
                        g[rng.choice(g.shape[0], 500)] + np.float32([-3.5, 20.5, 0.5])]).astype(np.float32)
    want_d, want_i = P.nearest_neighbors(q, ref)
    _check_nn(q, ref, want_d, "lattice with duplicates", want_index=want_i)


def test_nn_queries_outside_the_bounding_box(rooms):
    a, _ = rooms
    rng = np.random.default_rng(24)
    ref = a[:50_000]
    # up to 2 m outside the room on every side, some just outside, some exactly on the box
    q = (rng.random((20_000, 3)) * np.array([9.0, 8.0, 7.0]) - 2.0).astype(np.float32)
    inside = ((q >= ref.min(0)) & (q <= ref.max(0))).all(1)
    q = q[~inside]
    q = np.concatenate([q, ref.min(0)[None], ref.max(0)[None], ref.max(0)[None] + np.float32(1e-6)])
    want, _ = _cdist_nn(q, ref)
    _check_nn(q, ref, want, "queries outside the box")


def test_nn_far_queries_are_exact_and_cheap(rooms):
    """Queries 100 box diagonals away, mixed with ordinary ones: a search whose work grows with (distance / cell)^3 would visit
    ~1e12 cells per far query; the second pass answers them exactly in ordinary time."""
    from i2sdf_amd.mesh import nearest_neighbors
    a, b = rooms
    rng = np.random.default_rng(25)
    diag = float(np.linalg.norm(b.max(0) - b.min(0)))
    dirs = rng.normal(size=(300, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    far = (b.mean(0) + 100.0 * diag * dirs).astype(np.float32)
    far[:3] = b.mean(0) + 100.0 * diag * np.eye(3)                          # along the axes: many near-ties
    q = np.concatenate([a[:3000], far])[rng.permutation(3300)]
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nearest_neighbors(_cuda(q), _cuda(b), _stats=stats)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    n_fb = dict(s for s in stats if s[0] == "fallback_count")["fallback_count"]
    print(f"far queries: {seconds:.3f} s for {q.shape[0]} queries, {n_fb} answered by the second pass")
    assert n_fb >= 300 and seconds < 60.0
    want, _ = _cdist_nn(q, b)
    _check_nn(q, b, want, "far queries mixed with ordinary ones")


def test_nn_degenerate_references():
    rng = np.random.default_rng(26)
    q = (rng.random((5000, 3)) * 4.0 - 1.0).astype(np.float32)
    plane = (rng.random((20_000, 3)) * 2.0).astype(np.float32)
    plane[:, 2] = 0.75                                                      # coplanar
    line = plane.copy()
    line[:, 1] = -0.25                                                      # collinear
    same = np.tile(np.float32([[0.5, 1.5, -2.0]]), (1000, 1))               # all identical
    single = np.float32([[3.0, 3.0, 3.0]])                                  # R = 1
    for what, ref in (("coplanar", plane), ("collinear", line), ("identical", same), ("single point", single)):
        want_d, want_i = P.nearest_neighbors(q, ref)
        _check_nn(q, ref, want_d, what, want_index=want_i if what in ("identical", "single point") else None)


def test_nn_empty_and_bad_input():
    from i2sdf_amd.lib import I2SDFError
    from i2sdf_amd.mesh import nearest_neighbors
    ref = _cuda(_room(1000, seed=27))
    d, i = nearest_neighbors(torch.empty(0, 3, device="cuda"), ref)
    assert d.shape == (0,) and i.shape == (0,) and d.dtype == torch.float32 and i.dtype == torch.int32 and d.is_cuda
    with pytest.raises(ValueError):
        nearest_neighbors(ref, torch.empty(0, 3, device="cuda"))
    for bad in (ref.double(), ref[:, :2], ref.cpu()):
        with pytest.raises(ValueError):
            nearest_neighbors(bad, ref)
        with pytest.raises(ValueError):
            nearest_neighbors(ref, bad)
    for bad in (float("nan"), float("inf")):
        broken = ref.clone()
        broken[17, 2] = bad
        with pytest.raises(I2SDFError, match="finite"):
            nearest_neighbors(ref, broken)
        with pytest.raises(I2SDFError, match="finite"):
            nearest_neighbors(broken, ref)


def test_nn_is_bitwise_reproducible(rooms):
    from i2sdf_amd.mesh import nearest_neighbors
    a, b = rooms
    q, r = _cuda(a[:50_000]), _cuda(b[:50_000])
    d0, i0 = nearest_neighbors(q, r)
    d1, i1 = nearest_neighbors(q, r)
    assert torch.equal(d0, d1) and torch.equal(i0, i1)


# ---------------------------------------------------------------------------------------------- evaluate
@pytest.mark.parametrize("tag", ["raw", "ds"])
def test_evaluate_fixture(golden, tag):
    from i2sdf_amd.mesh import evaluate
    v, z = golden("g18_mcubes"), golden("g20_mesh_eval")
    thr = float(z["threshold"])
    got = evaluate(_cuda(v["a.verts"]), _cuda(v["b.verts"]), threshold=thr, down_sample=float(z["down_sample"]) if tag == "ds" else None)
    want = dict(zip(KEYS, z[f"{tag}.metrics"].tolist()))
    assert list(got) == list(KEYS) and all(type(x) is float for x in got.values())
    n_pred, n_trgt = z[f"{tag}.dist2"].shape[0], z[f"{tag}.dist1"].shape[0]
    print(f"evaluate fixture {tag}: " + ", ".join(f"{k} {got[k]:.9g} (golden {want[k]:.9g})" for k in KEYS))
    assert round(got["Prec"] * n_pred) == int((z[f"{tag}.dist2"] < thr).sum()) and got["Prec"] == want["Prec"]
    assert round(got["Recal"] * n_trgt) == int((z[f"{tag}.dist1"] < thr).sum()) and got["Recal"] == want["Recal"]
    assert abs(got["Acc"] - want["Acc"]) <= RTOL * want["Acc"] and abs(got["Comp"] - want["Comp"]) <= RTOL * want["Comp"]
    assert got["F-score"] == pytest.approx(2 * got["Prec"] * got["Recal"] / (got["Prec"] + got["Recal"]), rel=1e-14)
    assert got["F-score"] == pytest.approx(want["F-score"], rel=1e-14)


def test_evaluate_large_counts_inside_the_threshold_band(rooms):
    from i2sdf_amd.mesh import evaluate
    a, b = rooms
    pred, trgt = a[:100_000], b[:100_000]
    thr = 0.025            # 1e5 points on 94 m^2 of wall lie about 3 cm apart and trgt carries 3 cm of noise: about half the points
    got = evaluate(_cuda(pred), _cuda(trgt), threshold=thr, down_sample=None)
    dist1, _ = _cdist_nn(trgt, pred)
    dist2, _ = _cdist_nn(pred, trgt)
    for key, mean_key, d in (("Prec", "Acc", dist2), ("Recal", "Comp", dist1)):
        lo, hi = int((d < thr * (1 - RTOL)).sum()), int((d < thr * (1 + RTOL)).sum())
        count = got[key] * d.shape[0]
        print(f"evaluate rooms {key}: count {count:.1f} in [{lo}, {hi}] of {d.shape[0]}; {mean_key} {got[mean_key]:.9g} (fp64 {d.mean():.9g})")
        assert hi - lo <= 1e-5 * d.shape[0], "the band around the threshold holds too many points to show anything"
        assert abs(count - round(count)) < 1e-6 and lo <= round(count) <= hi
        assert 0.1 < got[key] < 0.9
        assert abs(got[mean_key] - d.mean()) <= RTOL * d.mean()


def test_evaluate_mesh_and_tensor_arguments(golden):
    from i2sdf_amd.mesh import Mesh, evaluate
    v = golden("g18_mcubes")
    a = Mesh(_cuda(v["a.verts"]), _cuda(v["a.faces"]), _cuda(v["a.normals"]))
    b = (_cuda(v["b.verts"]), _cuda(v["b.faces"]))
    want = evaluate(a.verts, b[0], threshold=0.2, down_sample=0.1)
    assert evaluate(a, b, threshold=0.2, down_sample=0.1) == want
    assert evaluate(a, b[0], threshold=0.2, down_sample=0.1) == want
    assert evaluate(a, b, threshold=0.2, down_sample=0.1) == want            # and again: bitwise, run to run
    import i2sdf_amd
    assert i2sdf_amd.evaluate is evaluate and callable(i2sdf_amd.voxel_down_sample) and callable(i2sdf_amd.nearest_neighbors)
    nothing = evaluate(a, b, threshold=1e-9, down_sample=0)                  # nothing within the threshold: 0 / 0
    assert nothing["Prec"] == 0.0 and nothing["Recal"] == 0.0 and np.isnan(nothing["F-score"])
    with pytest.raises(ValueError):
        evaluate(a, torch.empty(0, 3, device="cuda"))
    with pytest.raises(ValueError):
        evaluate(a.verts.cpu(), b)
    with pytest.raises(ValueError):
        evaluate(a.verts.double(), b)


def test_evaluate_marching_cubes_mesh_against_itself():
    from i2sdf_amd.mesh import evaluate, marching_cubes
    ax = [torch.arange(64, dtype=torch.float64, device="cuda") * 0.05 - 1.6] * 3
    x, y, z = torch.meshgrid(*ax, indexing="ij")
    m = marching_cubes((torch.sqrt(x * x + y * y + z * z) - 1.1).float(), 0.0, (0.05,) * 3, (-1.6,) * 3)
    assert m.verts.shape[0] > 1000
    for ds in (0.02, None):
        got = evaluate(m, m, down_sample=ds)
        assert got == {"Acc": 0.0, "Comp": 0.0, "Prec": 1.0, "Recal": 1.0, "F-score": 1.0}


@pytest.mark.parametrize("n", [1, 3, 49, 1000, 453_112])
def test_evaluate_fractions_are_true_quotients(n):
    """Prec and Recal are count / n by a true division (49 * (1 / 49) is not 1 in fp64)."""
    from i2sdf_amd.mesh import evaluate
    pts = torch.rand(n, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    got = evaluate(pts, pts, down_sample=None)
    assert got == {"Acc": 0.0, "Comp": 0.0, "Prec": 1.0, "Recal": 1.0, "F-score": 1.0}
    if n >= 49:
        k = n // 7
        part = evaluate(pts, pts[:k] , threshold=1e-12, down_sample=None)      # exactly k pred points have a trgt point at distance 0
        assert part["Recal"] == 1.0 and part["Prec"] == k / n
