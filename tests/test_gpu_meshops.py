"""GPU: the device mesh operations (csrc/meshops.hip; i2sdf_amd.mesh.face_components / largest_component / sample_surface,
grid.pca_frame, I2SDFNetwork.extract_mesh_high_res) against the numpy restatement (tests/meshops_ref.py) and the committed scipy
labels (tests/golden/g19_mesh_components.npz)."""
import numpy as np
import pytest
import torch

import mcubes_ref
import meshops_ref as M

pytestmark = pytest.mark.gpu

SMALL = ["bowtie", "hinge", "fan"]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_components(faces, n_verts, want=None):
    """faces: (F,3) int32 numpy.  Exact equality with `want` (default: the restatement) + the invariants."""
    from i2sdf_amd.mesh import face_components
    got = face_components(_cuda(faces), n_verts)
    assert got.dtype == torch.int32 and got.shape == (faces.shape[0],)
    got = got.cpu().numpy()
    want = M.face_components(faces) if want is None else want
    assert np.array_equal(got, want)
    assert (got <= np.arange(got.shape[0])).all()
    assert np.array_equal(got[got], got)
    pairs = M.adjacency_pairs(faces)
    assert np.array_equal(got[pairs[:, 0]], got[pairs[:, 1]])
    return got


def _fixture_mesh(golden, tag):
    z = golden("g19_mesh_components")
    if tag in SMALL:
        return z[f"{tag}.verts"], z[f"{tag}.faces"], z[f"{tag}.labels"]
    v = golden("g18_mcubes")
    verts, faces, _ = mcubes_ref.marching_cubes(v[f"{tag}.vol"], float(v[f"{tag}.level"]), v[f"{tag}.spacing"])
    return verts, faces, z[f"{tag}.labels"]


SPHERES = (((1.2, 1.2, 1.2), 0.9), ((3.4, 2.6, 4.0), 0.5), ((1.5, 3.0, 4.5), 0.2))
SPACING = 0.05


def _three_spheres():
    """Device Mesh of three disjoint spheres (radii 0.9 / 0.5 / 0.2) on a 96 x 80 x 112 grid of spacing 0.05."""
    from i2sdf_amd.mesh import marching_cubes
    ax = [torch.arange(n, dtype=torch.float64, device="cuda") * SPACING for n in (96, 80, 112)]
    x, y, z = torch.meshgrid(*ax, indexing="ij")
    vol = None
    for (cx, cy, cz), r in SPHERES:
        d = torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r
        vol = d if vol is None else torch.minimum(vol, d)
    return marching_cubes(vol.float(), 0.0, (SPACING,) * 3)


@pytest.mark.parametrize("tag", ["a", "b", "c"] + SMALL)
def test_components_fixtures(golden, tag):
    verts, faces, want = _fixture_mesh(golden, tag)
    _check_components(faces, verts.shape[0], want)          # scipy's labels, committed
    _check_components(faces, verts.shape[0])                # the restatement


def test_components_three_spheres_and_permuted():
    m = _three_spheres()
    faces = m.faces.cpu().numpy()
    got = _check_components(faces, m.verts.shape[0])
    assert np.unique(got).shape[0] == 3
    perm = np.random.default_rng(0).permutation(faces.shape[0])
    got_p = _check_components(faces[perm], m.verts.shape[0])
    assert np.array_equal(got_p, M.canonical(got[perm]))     # labels permute accordingly
    # n_verts = None (only non-negative indices required) and a Mesh argument give the same labels
    from i2sdf_amd.mesh import face_components
    assert torch.equal(face_components(m.faces), face_components(m))


def test_components_empty():
    from i2sdf_amd.mesh import face_components, largest_component, Mesh
    e = torch.empty(0, 3, dtype=torch.int32, device="cuda")
    assert face_components(e, 0).shape == (0,)
    v = torch.empty(0, 3, device="cuda")
    out = largest_component(Mesh(v, e, v))
    assert out.faces.shape == (0, 3) and out.verts.shape == (0, 3)


def test_components_many_at_scale():
    """The three-sphere mesh replicated with vertex offsets to >= 2 M faces, faces permuted: the component of every face is known
    by construction (replica, sphere), so the expected labels are the smallest face index of each known id."""
    m = _three_spheres()
    faces = m.faces.cpu().numpy()
    V, F = m.verts.shape[0], faces.shape[0]
    small = _check_components(faces, V)
    ids = np.unique(small, return_inverse=True)[1]
    K = -(-2_000_000 // F)
    big = (faces[None].astype(np.int64) + (np.arange(K) * V)[:, None, None]).reshape(-1, 3).astype(np.int32)
    comp = (ids[None] + 3 * np.arange(K)[:, None]).reshape(-1)
    perm = np.random.default_rng(1).permutation(big.shape[0])
    big, comp = big[perm], comp[perm]
    assert big.shape[0] >= 2_000_000
    from i2sdf_amd.mesh import face_components
    got = face_components(_cuda(big), K * V).cpu().numpy()
    assert np.array_equal(got, M.canonical(comp))
    assert (got <= np.arange(got.shape[0])).all() and np.array_equal(got[got], got)
    pairs = M.adjacency_pairs(big)
    assert np.array_equal(got[pairs[:, 0]], got[pairs[:, 1]])
    assert np.unique(got).shape[0] == 3 * K


def test_components_one_giant():
    """A gyroid-like volume: >= 2 M faces, almost all in one component (every union ends at few roots)."""
    from i2sdf_amd.mesh import marching_cubes
    shape, periods = (320, 304, 336), 3.0
    ax = [torch.arange(n, dtype=torch.float32, device="cuda") * (2 * np.pi * periods / 320) for n in shape]
    x, y, z = torch.meshgrid(*ax, indexing="ij")
    vol = torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)
    m = marching_cubes(vol, 0.0)
    del vol, x, y, z
    faces = m.faces.cpu().numpy()
    assert faces.shape[0] >= 2_000_000, faces.shape
    got = _check_components(faces, m.verts.shape[0])
    assert np.bincount(got).max() >= 0.9 * faces.shape[0]


def test_largest_component_three_spheres():
    from i2sdf_amd.mesh import largest_component
    m = _three_spheres()
    verts, faces, normals = (t.cpu().numpy() for t in m)
    labels = M.face_components(faces)
    ids = np.unique(labels)
    areas64 = np.array([M.face_areas(verts, faces[labels == i], np.float64).sum() for i in ids])
    top = np.sort(areas64)[::-1]
    assert ids.shape[0] == 3 and (top[0] - top[1]) / top[0] > 1e-3                 # a clear winner (fp64 face areas): fp32 face areas cannot change it
    got = largest_component(m)
    wv, wf, wn = M.largest_component(verts, faces, normals)
    assert np.array_equal(got.faces.cpu().numpy(), wf)
    assert np.array_equal(got.verts.cpu().numpy(), wv) and np.array_equal(got.normals.cpu().numpy(), wn)   # gathered: bitwise
    area, _, euler, closed, _ = mcubes_ref.mesh_stats(wv, wf)
    assert closed and euler == 2
    gv, gf = got.verts.cpu().numpy(), got.faces.cpu().numpy()
    got_area = M.face_areas(gv, gf, np.float64).sum()
    assert abs(got_area - top[0]) <= 1e-12 * top[0]
    assert abs(got_area - 4 * np.pi * 0.9 ** 2) <= 0.01 * 4 * np.pi * 0.9 ** 2      # the largest sphere's (chords: a little less)


def _decade_mesh():
    """The three-sphere mesh three times, scaled by 1, 0.1 and 0.01 about the origin: face areas over more than four decades."""
    m = _three_spheres()
    V = m.verts.shape[0]
    verts = torch.cat([m.verts * s for s in (1.0, 0.1, 0.01)]).contiguous()
    faces = torch.cat([m.faces + k * V for k in range(3)]).contiguous()
    return verts, faces


def test_sample_surface_recorded_draws():
    from i2sdf_amd.mesh import sample_surface
    verts_t, faces_t = _decade_mesh()
    verts, faces = verts_t.cpu().numpy(), faces_t.cpu().numpy()
    n = 100_000
    g = np.random.default_rng(2)
    u_face, u_bary = g.random(n, dtype=np.float32), g.random((n, 2), dtype=np.float32)
    area = M.face_areas(verts, faces)
    assert area.max() / area[area > 0].min() >= 1e4
    pts, fi = sample_surface((verts_t, faces_t), n, draws={"u_face": _cuda(u_face), "u_bary": _cuda(u_bary)})
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and fi.shape == (n,) and fi.dtype == torch.int32
    pts, fi = pts.cpu().numpy(), fi.cpu().numpy().astype(np.int64)
    assert fi.min() >= 0 and fi.max() < faces.shape[0]
    cdf = M.area_cdf(verts, faces)
    pick = u_face.astype(np.float64) * cdf[-1]
    tol = 1e-6 * cdf[-1]
    lo = np.where(fi > 0, cdf[np.maximum(fi - 1, 0)], 0.0)
    assert (lo - tol <= pick).all() and (pick <= cdf[fi] + tol).all()               # every sample
    _, want_fi, _ = M.sample_surface(verts, faces, u_face, u_bary)
    print(f"sample_surface: {int((want_fi != fi).sum())} of {n} face indices differ from the restatement's (allowed at CDF edges)")
    diag = np.linalg.norm(verts.max(axis=0).astype(np.float64) - verts.min(axis=0))
    want = M.points_on_faces(verts, faces, fi, u_bary)
    err = np.abs(pts - want).max()
    print(f"sample_surface: max point error {err:.3e} (bar {1e-6 * diag:.3e})")
    assert err <= 1e-6 * diag                                                       # every sample
    # all three scales are drawn from, in proportion to their area (1 : 1e-2 : 1e-4)
    share = np.bincount(fi // (faces.shape[0] // 3), minlength=3) / n
    assert abs(share[1] - 1e-2 / 1.0101) < 3e-3 and share[2] < 1e-3


def test_sample_surface_points_lie_in_their_triangles():
    """Barycentric coordinates of every returned point within [-1e-6, 1 + 1e-6] and the point in the triangle's plane.  On a
    unit-size mesh: fp32 coordinates of magnitude 1 resolve barycentrics to ~1e-7 only when the triangles are of that size too
    (on the four-decade mesh above a triangle can be 1e4 times smaller than its coordinates)."""
    from i2sdf_amd.mesh import sample_surface
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    n = 20_000
    g = np.random.default_rng(3)
    u_face, u_bary = g.random(n, dtype=np.float32), g.random((n, 2), dtype=np.float32)
    pts, fi = sample_surface((_cuda(verts), _cuda(faces)), n, draws={"u_face": _cuda(u_face), "u_bary": _cuda(u_bary)})
    pts, fi = pts.cpu().numpy().astype(np.float64), fi.cpu().numpy()
    assert np.bincount(fi, minlength=4).min() > 0.1 * n
    v = verts.astype(np.float64)[faces[fi]]
    e1, e2, d = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], pts - v[:, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.abs(np.einsum("ij,ij->i", d, nrm)).max() <= 1e-6 * np.sqrt(3.0)
    # d = a e1 + b e2 in the plane: 2x2 normal equations
    g11, g12, g22 = (np.einsum("ij,ij->i", p, q) for p, q in ((e1, e1), (e1, e2), (e2, e2)))
    r1, r2 = np.einsum("ij,ij->i", d, e1), np.einsum("ij,ij->i", d, e2)
    det = g11 * g22 - g12 * g12
    a, b = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    for c in (a, b, 1.0 - a - b):
        assert c.min() >= -1e-6 and c.max() <= 1.0 + 1e-6, (c.min(), c.max())


def test_sample_surface_edge_cases():
    from i2sdf_amd.mesh import sample_surface
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [5, 5, 5]])
    faces = np.int32([[6, 6, 6], [0, 1, 2], [6, 6, 6], [0, 0, 1], [3, 4, 5], [6, 6, 6]])     # zero-area faces first, between, last
    vt, ft = _cuda(verts), _cuda(faces)
    p, f = sample_surface((vt, ft), 0)
    assert p.shape == (0, 3) and f.shape == (0,)
    n = 50_000
    g = np.random.default_rng(4)
    u_face = np.maximum(g.random(n, dtype=np.float32), np.float32(1e-7))     # (a draw of exactly 0 picks face 0 whatever its area, as in trimesh)
    u_face[:3] = [0.5, 0.99999994, 1e-7]
    u_bary = g.random((n, 2), dtype=np.float32)
    p, f = sample_surface((vt, ft), n, draws={"u_face": _cuda(u_face), "u_bary": _cuda(u_bary)})
    f = f.cpu().numpy()
    assert set(np.unique(f).tolist()) == {1, 4}                              # zero-area faces are never picked
    assert f[0] == 1 and f[1] == 4 and f[2] == 1                             # pick exactly on the edge cdf[1] = 0.5: the left face
    _, want, _ = M.sample_surface(verts, faces, u_face, u_bary)
    assert np.array_equal(f, want)
    # every area zero: cdf is 0 everywhere, searchsorted gives face 0
    p, f = sample_surface((vt, _cuda(np.int32([[6, 6, 6], [0, 0, 1]]))), 16, draws={"u_face": _cuda(u_face[:16]), "u_bary": _cuda(u_bary[:16])})
    assert f.cpu().tolist() == [0] * 16 and torch.equal(p, torch.full((16, 3), 5.0, device="cuda"))
    # without draws: torch.rand on the device with the given generator
    gen = torch.Generator(device="cuda").manual_seed(5)
    p1, f1 = sample_surface((vt, ft), 1000, generator=gen)
    gen.manual_seed(5)
    p2, f2 = sample_surface((vt, ft), 1000, generator=gen)
    assert torch.equal(p1, p2) and torch.equal(f1, f2) and set(np.unique(f1.cpu().numpy()).tolist()) == {1, 4}


def test_pca_frame():
    from i2sdf_amd.grid import pca_frame
    g = np.random.default_rng(6)
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    p = ((g.standard_normal((10000, 3)) * [0.25, 0.4, 0.7]) @ q.T + [0.3, -0.2, 0.1]).astype(np.float32)
    p64 = p.astype(np.float64)
    d = p64 - p64.mean(axis=0)
    S = d.T @ d
    ev = np.linalg.eigvalsh(S)
    assert (ev[1:] / ev[:-1]).min() >= 1.1                                   # separated eigenvalues: the order is well defined
    vecs, s_mean = pca_frame(_cuda(p))
    assert vecs.is_cuda and vecs.dtype == torch.float32 and vecs.shape == (3, 3) and s_mean.shape == (3,)
    v = vecs.cpu().numpy().astype(np.float64)
    assert np.abs(v @ v.T - np.eye(3)).max() <= 1e-6
    assert abs(np.linalg.det(v) - 1.0) <= 1e-5
    D = v @ S @ v.T
    assert np.abs(D - np.diag(np.diag(D))).max() <= 1e-5 * np.abs(D).max()
    wv, wm = M.pca_frame(p)
    assert np.abs(v - wv).max() <= 1e-5 and np.abs(s_mean.cpu().numpy() - wm).max() <= 1e-5
    # the left-handed branch too: a mirrored cloud
    v2, _ = pca_frame(_cuda(p * np.float32([1, 1, -1])))
    w2, _ = M.pca_frame(p * np.float32([1, 1, -1]))
    v2 = v2.cpu().numpy().astype(np.float64)
    assert abs(np.linalg.det(v2) - 1.0) <= 1e-5 and np.abs(v2 - w2).max() <= 1e-5


def _draws(n, seed):
    g = np.random.default_rng(seed)
    return {"u_face": _cuda(g.random(n, dtype=np.float32)), "u_bary": _cuda(g.random((n, 2), dtype=np.float32))}


@pytest.mark.parametrize("take_components", [True, False])
def test_extract_mesh_high_res(take_components):
    from test_gpu_mcubes import _synthetic_net
    from i2sdf_amd import uniform_axes, aligned_axes
    from i2sdf_amd.grid import pca_frame
    from i2sdf_amd.mesh import largest_component, sample_surface
    net = _synthetic_net()
    n_pts, res = 10000, 64
    dr = _draws(n_pts, 7)
    m, vecs, s_mean, axes = net.extract_mesh_high_res(res, take_components=take_components, n_points=n_pts, draws=dr)
    assert m.faces.shape[0] > 100
    # the same chain written out with the public pieces
    low = net.extract_mesh(uniform_axes(100, (-2.0, 2.0)), 0.0)
    low_all = low
    if take_components:
        low = largest_component(low)
    pts, _ = sample_surface(low, n_pts, draws=dr)
    wvecs, wmean = pca_frame(pts)
    helper = ((pts - wmean).unsqueeze(1) * wvecs.unsqueeze(0)).sum(dim=2)
    wax = aligned_axes(helper, res)
    want = net.extract_mesh(wax, 0.0, rot=wvecs.t(), trans=wmean)
    assert torch.equal(vecs, wvecs) and torch.equal(s_mean, wmean)
    for a, b in zip(axes.xyz, wax.xyz):
        assert np.array_equal(a, b)
    for x, y in zip(m, want):
        assert torch.equal(x, y)
    sdf = net.sdf_grid(m.verts.contiguous())
    assert float(sdf.abs().max()) <= 0.25 * axes.spacing[0], float(sdf.abs().max())
    # steps 2-4 restated on the downloaded low-res mesh
    lv, lf, ln = (t.cpu().numpy() for t in low_all)
    if take_components:
        lv, lf, ln = M.largest_component(lv, lf, ln)
    rp, _, _ = M.sample_surface(lv, lf, dr["u_face"].cpu().numpy(), dr["u_bary"].cpu().numpy())
    rv, rm = M.pca_frame(rp.astype(np.float32))                          # (the reference casts its sample to fp32 before the PCA)
    ev, em = np.abs(vecs.cpu().numpy() - rv).max(), np.abs(s_mean.cpu().numpy() - rm).max()
    print(f"extract_mesh_high_res(take_components={take_components}): vecs differ by {ev:.3e}, s_mean by {em:.3e} from the restatement")
    assert ev <= 1e-5 and em <= 1e-5


def test_extract_mesh_high_res_empty():
    from test_gpu_mcubes import _synthetic_net
    net = _synthetic_net()
    m, vecs, s_mean, axes = net.extract_mesh_high_res(32, level=1e6, low_resolution=16)
    assert m.faces.shape == (0, 3) and m.verts.shape == (0, 3) and vecs is None and s_mean is None and axes is None


def test_runs_are_bitwise_identical():
    from test_gpu_mcubes import _synthetic_net
    from i2sdf_amd.grid import pca_frame
    from i2sdf_amd.mesh import face_components, largest_component, sample_surface
    m = _three_spheres()
    perm = torch.from_numpy(np.random.default_rng(8).permutation(m.faces.shape[0])).cuda()
    shuffled = type(m)(m.verts, m.faces[perm].contiguous(), m.normals)
    dr = _draws(50_000, 9)
    runs = []
    for _ in range(2):
        pts, fi = sample_surface(shuffled, 50_000, draws=dr)
        runs.append([face_components(shuffled), *largest_component(shuffled), pts, fi, *pca_frame(pts)])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    net = _synthetic_net()
    dr = _draws(10000, 10)
    a = net.extract_mesh_high_res(48, draws=dr)
    b = net.extract_mesh_high_res(48, draws=dr)
    for x, y in zip([*a[0], a[1], a[2]], [*b[0], b[1], b[2]]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1])
def test_cumsum_f64_at_the_scan_boundaries(n, permuted):
    """i2sdf_mesh_cumsum_f64 around a wave, a workgroup, a chunk of 1024 items and the size at which the second level of chunk sums
    appears.  The items are the integers 0..7 in fp32: every partial sum is a whole number far below 2^53, so the fp64 running sum
    is exact in any order of additions and the result must equal numpy's bit for bit.  The workspace is the size the library asks
    for, with a canary behind it."""
    from i2sdf_amd import lib as L
    lib = L.load()
    rng = np.random.default_rng(1000 * n + permuted)
    x = rng.integers(0, 8, n).astype(np.float32)
    order = rng.permutation(n).astype(np.int64) if permuted else None
    want = np.cumsum((x[order] if permuted else x).astype(np.float64))
    size = int(lib.i2sdf_mesh_scan_workspace_bytes(n))
    assert size > 0
    ws = torch.full((size + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    cdf = torch.full((n + 8,), -1.0, dtype=torch.float64, device="cuda")
    dx, dorder = _cuda(x), (_cuda(order) if permuted else None)
    rc = lib.i2sdf_mesh_cumsum_f64(L.ptr(dx), n, L.ptr(dorder) if permuted else None, n, L.ptr(cdf), L.ptr(ws), L.stream_ptr())
    assert rc == 0
    got = cdf.cpu().numpy()
    assert np.array_equal(got[:n].view(np.int64), want.view(np.int64))
    assert (got[n:] == -1.0).all()                                  # nothing written behind the n sums
    assert bool((ws[size:] == 0xA5).all()), "bytes behind i2sdf_mesh_scan_workspace_bytes(n) were written"


def test_argument_errors():
    """A face index equal to n_verts is reported, not dereferenced.  The vertex buffer has slack rows behind n_verts, so that
    even a broken validation would read memory this test owns."""
    from i2sdf_amd import lib as L
    from i2sdf_amd.mesh import Mesh, compact, face_components, largest_component, sample_surface
    lib = L.load()
    n = 4
    buf = torch.zeros(n + 8, 3, device="cuda")
    buf[:n] = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    verts = buf[:n]
    good = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=torch.int32, device="cuda")
    bad = good.clone()
    bad[2, 1] = n
    assert face_components(good, n).tolist() == [0, 0, 0, 0]
    # the C ABI: the kernel sets the status word, i2sdf_mesh_status turns it into I2SDF_EINVAL
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    keys = torch.empty(12, dtype=torch.int64, device="cuda")
    st = L.stream_ptr()
    assert lib.i2sdf_mesh_edge_keys(L.ptr(good), 4, n, L.ptr(keys), L.ptr(status), st) == 0
    assert lib.i2sdf_mesh_status(L.ptr(status), st) == 0
    assert lib.i2sdf_mesh_edge_keys(L.ptr(bad), 4, n, L.ptr(keys), L.ptr(status), st) == 0
    assert lib.i2sdf_mesh_status(L.ptr(status), st) == -1
    status.zero_()
    area = torch.empty(4, device="cuda")
    assert lib.i2sdf_mesh_face_areas(L.ptr(verts), n, L.ptr(bad), 4, L.ptr(area), L.ptr(status), st) == 0
    assert lib.i2sdf_mesh_status(L.ptr(status), st) == -1 and float(area[2]) == 0.0 and float(area[0]) == 0.5
    assert lib.i2sdf_mesh_edge_keys(L.ptr(good), 2 ** 31, n, L.ptr(keys), L.ptr(status), st) == -1          # F beyond int32
    assert lib.i2sdf_mesh_edge_keys(L.ptr(good), 4, 2 ** 31, L.ptr(keys), L.ptr(status), st) == -1          # n_verts beyond int32
    assert lib.i2sdf_mesh_scan_workspace_bytes(2 ** 31) == 0 and lib.i2sdf_mesh_scan_workspace_bytes(5) > 0
    assert lib.i2sdf_mesh_status(None, st) == -1
    with pytest.raises(L.I2SDFError, match=r"\(-1\)"):
        face_components(bad, n)
    with pytest.raises(L.I2SDFError, match=r"\(-1\)"):
        face_components(torch.tensor([[0, 1, -1]], dtype=torch.int32, device="cuda"))
    nrm = torch.zeros(n, 3, device="cuda")
    with pytest.raises(L.I2SDFError, match=r"\(-1\)"):
        largest_component(Mesh(verts, bad, nrm))
    with pytest.raises(L.I2SDFError, match=r"\(-1\)"):
        sample_surface((verts, bad), 64)
    # wrong dtypes / host tensors
    with pytest.raises(ValueError):
        face_components(good.long(), n)
    with pytest.raises(ValueError):
        face_components(good.cpu(), n)
    with pytest.raises(ValueError):
        largest_component(Mesh(verts.double(), good, nrm))
    with pytest.raises(ValueError):
        largest_component(Mesh(verts.cpu(), good, nrm))
    with pytest.raises(ValueError):
        sample_surface((verts, good.cpu()), 4)
    with pytest.raises(ValueError):
        sample_surface((verts, good), 4, draws={"u_face": torch.zeros(4)})
    with pytest.raises(ValueError):
        sample_surface((verts, good), 4, draws={"u_face": torch.zeros(5, device="cuda")})
    with pytest.raises(ValueError):
        sample_surface((verts, torch.empty(0, 3, dtype=torch.int32, device="cuda")), 4)
    with pytest.raises(ValueError):
        compact(Mesh(verts, good, nrm), torch.ones(3, dtype=torch.bool, device="cuda"))
    sub = compact(Mesh(verts, good, nrm), torch.tensor([False, True, False, False], device="cuda"))
    assert sub.faces.tolist() == [[0, 1, 2]] and torch.equal(sub.verts, verts[[0, 1, 3]])
