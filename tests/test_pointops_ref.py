"""CPU: the numpy restatement of the point-set operations (tests/pointops_ref.py) against the committed scikit-learn KDTree
distances (tests/golden/g20_mesh_eval.npz), and its tie, duplicate and ordering rules on cases small enough to read."""
import numpy as np
import pytest

import pointops_ref as P

KEYS = ("Acc", "Comp", "Prec", "Recal", "F-score")


def _sets(golden, tag):
    v, z = golden("g18_mcubes"), golden("g20_mesh_eval")
    p, t = v["a.verts"], v["b.verts"]
    if tag == "ds":
        p, _ = P.voxel_down_sample(p, float(z["down_sample"]))
        t, _ = P.voxel_down_sample(t, float(z["down_sample"]))
    return p, t, z


@pytest.mark.parametrize("tag", ["raw", "ds"])
def test_brute_force_matches_the_kdtree_distances(golden, tag):
    p, t, z = _sets(golden, tag)
    if tag == "ds":
        assert [p.shape[0], t.shape[0]] == z["ds.n"].tolist() == [694, 1308]
    d1, i1 = P.nearest_neighbors(t, p)
    d2, i2 = P.nearest_neighbors(p, t)
    np.testing.assert_allclose(d1, z[f"{tag}.dist1"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d2, z[f"{tag}.dist2"], rtol=1e-12, atol=0)
    # the returned index is the point at that distance
    np.testing.assert_allclose(np.linalg.norm(t.astype(np.float64) - p.astype(np.float64)[i1], axis=1), d1, rtol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(p.astype(np.float64) - t.astype(np.float64)[i2], axis=1), d2, rtol=1e-12)
    thr = float(z["threshold"])
    got = P.metrics(d1, d2, thr)
    want = dict(zip(KEYS, z[f"{tag}.metrics"]))
    assert got["Prec"] == want["Prec"] and got["Recal"] == want["Recal"] and got["F-score"] == want["F-score"]
    np.testing.assert_allclose([got["Acc"], got["Comp"]], [want["Acc"], want["Comp"]], rtol=1e-12)
    ev = P.evaluate(v_a(golden), v_b(golden), threshold=thr, down_sample=float(z["down_sample"]) if tag == "ds" else None)
    assert ev == got


def v_a(golden):
    return golden("g18_mcubes")["a.verts"]


def v_b(golden):
    return golden("g18_mcubes")["b.verts"]


def test_fixture_has_no_distance_on_the_threshold(golden):
    z = golden("g20_mesh_eval")
    thr = float(z["threshold"])
    for tag in ("raw", "ds"):
        for k in ("dist1", "dist2"):
            d = z[f"{tag}.{k}"]
            assert d.dtype == np.float64 and not (np.abs(d - thr) <= 1e-6 * thr).any()
        m = dict(zip(KEYS, z[f"{tag}.metrics"]))
        assert 0.1 < m["Prec"] < 0.9 and 0.1 < m["Recal"] < 0.9


def test_nearest_neighbour_ties_and_duplicates():
    ref = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]])
    q = np.float32([[0, 0, 0], [1, 0, 0], [0, 2, 0], [9, 9, 9], [0.5, 0.5, 0]])
    d, i = P.nearest_neighbors(q, ref, chunk=2)
    assert i.tolist() == [0, 0, 2, 5, 0]                       # equal distances: the smallest index; duplicates: the first
    np.testing.assert_allclose(d, [1.0, 0.0, 1.0, np.sqrt(48.0), np.sqrt(0.5)], rtol=1e-15)
    d1, i1 = P.nearest_neighbors(q, ref[:1])
    assert i1.tolist() == [0] * 5
    with pytest.raises(ValueError):
        P.nearest_neighbors(q, ref[:0])
    d0, i0 = P.nearest_neighbors(q[:0], ref)
    assert d0.shape == (0,) and i0.shape == (0,)


def test_voxel_down_sample_rule():
    # lo = min - voxel / 2: with voxel 1 and a minimum of 0 the voxel borders sit at -0.5, 0.5, 1.5, ...; a point exactly on a
    # border belongs to the upper voxel
    pts = np.float32([[0, 0, 0], [0.49, 0, 0], [0.5, 0, 0], [1.49, 0, 0], [1.5, 0, 0], [0, 0.5, 0], [0.25, 0, 0.5], [0.25, 0, 0]])
    means, counts = P.voxel_down_sample(pts, 1.0)
    idx = P.voxel_indices(pts, 1.0)
    assert idx.tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]]
    # ascending (ix, iy, iz): (0,0,0) (0,0,1) (0,1,0) (1,0,0) (2,0,0)
    assert counts.tolist() == [3, 1, 1, 2, 1] and counts.dtype == np.int32 and means.dtype == np.float32
    want = np.float64([[(0 + np.float64(np.float32(0.49)) + 0.25) / 3, 0, 0], [0.25, 0, 0.5], [0, 0.5, 0],
                       [(0.5 + np.float64(np.float32(1.49))) / 2, 0, 0], [1.5, 0, 0]]).astype(np.float32)
    assert np.array_equal(means, want)
    # one point, and all points in one voxel
    m1, c1 = P.voxel_down_sample(pts[3:4], 0.02)
    assert np.array_equal(m1, pts[3:4]) and c1.tolist() == [1]
    m2, c2 = P.voxel_down_sample(pts, 100.0)
    assert c2.tolist() == [8] and m2.shape == (1, 3)
    m0, c0 = P.voxel_down_sample(pts[:0], 1.0)
    assert m0.shape == (0, 3) and c0.shape == (0,)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.voxel_down_sample(pts, bad)
    with pytest.raises(ValueError):
        P.voxel_down_sample(np.float32([[0, 0, 0], [1e6, 0, 0]]), 1e-3)     # 1e9 voxels along x: beyond 21 bits
    with pytest.raises(ValueError):
        P.voxel_down_sample(np.float32([[0, 0, np.nan]]), 1.0)


def test_voxel_sums_run_left_to_right_in_original_order():
    """A long run (beyond the vectorised part) and short runs give the sequential fp64 sum, whatever way the restatement takes."""
    rng = np.random.default_rng(3)
    big = (rng.random((500, 3)) * 0.45).astype(np.float32)                  # all in voxel (0, 0, 0) of size 1 ...
    big[0] = 0.0
    small = (rng.random((40, 3)) * 0.45 + np.float32([3, 0, 0])).astype(np.float32)
    pts = np.concatenate([big[:250], small, big[250:]])                     # ... interleaved with another voxel's points
    means, counts = P.voxel_down_sample(pts, 1.0)
    assert counts.tolist() == [500, 40]
    for m, grp in ((0, big), (1, small)):
        s = np.zeros(3, np.float64)
        for row in grp.astype(np.float64):
            s = s + row
        assert np.array_equal(means[m], (s / grp.shape[0]).astype(np.float32))


def test_metrics_edge_cases():
    m = P.metrics(np.float64([1.0, 2.0]), np.float64([3.0]), 0.5)
    assert m["Prec"] == 0.0 and m["Recal"] == 0.0 and np.isnan(m["F-score"]) and m["Acc"] == 3.0 and m["Comp"] == 1.5
    m = P.metrics(np.float64([0.0, 0.0]), np.float64([0.0]), 0.05)
    assert m == {"Acc": 0.0, "Comp": 0.0, "Prec": 1.0, "Recal": 1.0, "F-score": 1.0}
    assert set(m) == set(KEYS)
