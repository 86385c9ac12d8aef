"""CPU: the numpy restatement of the mesh operations (tests/meshops_ref.py) against scipy's connected components on the
face-adjacency graph (live when scipy is importable, and always through the committed labels of g19_mesh_components.npz),
and its surface sampling against hand-computed draws."""
import numpy as np
import pytest

import mcubes_ref
import meshops_ref as M

SMALL = ["bowtie", "hinge", "fan"]


def _case(golden, tag):
    z = golden("g19_mesh_components")
    if tag in SMALL:
        return z[f"{tag}.verts"], z[f"{tag}.faces"], z[f"{tag}.labels"]
    v = golden("g18_mcubes")
    verts, faces, _ = mcubes_ref.marching_cubes(v[f"{tag}.vol"], float(v[f"{tag}.level"]), v[f"{tag}.spacing"])
    return verts, faces, z[f"{tag}.labels"]


@pytest.mark.parametrize("tag", ["a", "b", "c"] + SMALL)
def test_components_equal_the_committed_scipy_labels(golden, tag):
    _, faces, want = _case(golden, tag)
    got = M.face_components(faces)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(M.canonical(got), got)
    assert len(np.unique(want)) == {"a": 1, "b": 1, "c": 35, "bowtie": 2, "hinge": 1, "fan": 1}[tag]


@pytest.mark.parametrize("tag", ["a", "b", "c"] + SMALL)
def test_components_equal_scipy_live(golden, tag):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix
    _, faces, _ = _case(golden, tag)
    pairs = M.adjacency_pairs(faces)
    F = faces.shape[0]
    g = coo_matrix((np.ones(len(pairs), bool), (pairs[:, 0], pairs[:, 1])), shape=(F, F))
    _, lab = csgraph.connected_components(g, directed=False)
    assert np.array_equal(M.canonical(lab), M.canonical(M.face_components(faces)))
    assert np.array_equal(M.canonical(lab), M.face_components(faces))


def test_components_do_not_depend_on_the_face_order(golden):
    _, faces, want = _case(golden, "c")
    perm = np.random.default_rng(0).permutation(faces.shape[0])
    got = M.face_components(faces[perm])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    # the component of new face i is the old component of perm[i]; canonical labels = smallest NEW index per component
    assert np.array_equal(got, M.canonical(want[perm]))
    assert M.face_components(np.zeros((0, 3), np.int32)).shape == (0,)


def test_sample_surface_by_hand():
    """Two right triangles with legs 1 (areas 0.5 each, cdf 0.5, 1.0): pick 0.1 -> face 0; pick exactly 0.5 = cdf[0] (u = 0.5) ->
    still face 0 (side='left'); pick 0.999 -> face 1; draws with a + b > 1 are reflected to (|a - 1|, |b - 1|)."""
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]])
    faces = np.int32([[0, 1, 2], [3, 4, 5]])
    assert np.array_equal(M.face_areas(verts, faces), np.float32([0.5, 0.5]))
    assert np.array_equal(M.area_cdf(verts, faces), [0.5, 1.0])
    u_face = np.float32([0.1, 0.5, 0.25, 0.999])
    u_bary = np.float32([[0.25, 0.5], [0.75, 0.75], [0.0, 0.0], [0.5, 0.25]])
    pts, face, cdf = M.sample_surface(verts, faces, u_face, u_bary)
    assert face.tolist() == [0, 0, 0, 1]                                    # pick 0.5 == cdf[0] takes the LEFT face
    want = np.float64([[0.25, 0.5, 0], [0.25, 0.25, 0], [0, 0, 0], [0.5, 0.25, 1.0]])
    assert np.array_equal(pts, want)
    # a zero-area face in the middle is never picked; a pick beyond the total is clamped
    verts2 = np.concatenate([verts, np.float32([[5, 5, 5]])])
    faces2 = np.int32([[0, 1, 2], [6, 6, 6], [3, 4, 5]])
    _, face2, _ = M.sample_surface(verts2, faces2, np.float32([0.5, 0.50001, 0.9999999]), np.zeros((3, 2), np.float32))
    assert face2.tolist() == [0, 2, 2]


def test_largest_component_and_compaction(golden):
    verts, faces, labels = _case(golden, "bowtie")
    verts = verts.copy()
    verts[4:] *= np.float32(1.5)                                            # the second tetrahedron (faces 4..7) is the larger one
    v, f, _ = M.largest_component(verts, faces)
    assert f.shape == (4, 3) and v.shape == (4, 3)
    assert np.array_equal(v, verts[[3, 4, 5, 6]]) and f.max() == 3
    ids, areas = M.component_areas(verts, faces, labels)
    assert ids.tolist() == [0, 4] and areas[1] > areas[0]


def test_pca_frame_is_a_right_handed_eigen_frame():
    g = np.random.default_rng(1)
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    p = (g.standard_normal((5000, 3)) * [0.2, 0.5, 1.0]) @ q.T + [0.3, -0.2, 0.1]
    vecs, mean = M.pca_frame(p)
    assert np.allclose(vecs @ vecs.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(vecs), 1.0)
    d = p - mean
    s = vecs @ (d.T @ d) @ vecs.T
    assert np.abs(s - np.diag(np.diag(s))).max() <= 1e-9 * np.abs(s).max()
