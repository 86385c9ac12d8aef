"""GPU: mesh simplification, cleaning and the topology report (csrc/simplify.hip, i2sdf_amd.mesh) held to the numpy restatement
tests/simplify_ref.py -- bit for bit: the law is + - * / sqrt in fp64 in a written order, so there is no tolerance anywhere in this file.
  1. simplify_vertex_clustering against the restatement in vertices, faces, the three maps and normals, through the C ABI with canaries
     around every buffer the new entry points write and through the front end; two runs bitwise equal; `average` = voxel_down_sample;
  2. a NaN vertex and a face index out of range are refused through the status word, nothing is dereferenced;
  3. clean against the restatement, and on a marching-cubes level set: no repeated index, no zero-area face, and closest_point through
     the tree and through the brute route then agree bit for bit;
  4. topology against the restatement on every fixture, and what it says about the icosphere, the cap, the open cube, a flipped face;
  5. extract_mesh(simplify=h) is the three calls made by hand, simplify=None is the call without the keyword."""
import numpy as np
import pytest
import torch

import pointops_ref as P
import raycast_ref as R
import simplify_ref as S
import winding_ref as W

pytestmark = pytest.mark.gpu

F32, D = np.float32, np.float64
CANARY = 64
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mesh(v, f, n=None):
    m = (_cuda(np.asarray(v, F32).reshape(-1, 3)), _cuda(np.asarray(f, np.int32).reshape(-1, 3)))
    return m if n is None else m + (_cuda(np.asarray(n, F32).reshape(-1, 3)),)


class Guard:
    """buffers with canaries on both sides; check() after the work"""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype, what):
        n = int(np.prod(shape))
        fill = {torch.float32: -7.5, torch.uint8: 0xA5}.get(dtype, -77)
        buf = torch.full((n + 2 * CANARY,), fill, dtype=dtype, device="cuda")
        self.items.append((buf, n, fill, what))
        return buf[CANARY:CANARY + n].view(shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, n, fill, what in self.items:
            assert bool((buf[:CANARY] == fill).all()) and bool((buf[CANARY + n:] == fill).all()), f"canary of {what} overwritten"


def _raw_simplify(v, f, h, contraction="quadric", reg=1e-3, normals=None):
    """the front end's sequence of C calls with every output of the new entry points in a guarded buffer -> the dict of S.simplify
    (+ status): bad faces are reported, not raised"""
    from i2sdf_amd import lib as L
    lib = L.load()
    g = Guard()
    vt, ft = _mesh(v, f)
    nt = None if normals is None else _cuda(np.asarray(normals, F32))
    V, F = vt.shape[0], ft.shape[0]
    st = L.stream_ptr()
    i32, i64 = torch.int32, torch.int64
    pstatus = torch.zeros(2, dtype=i32, device="cuda")
    status = g.new((1,), i32, "status")
    status.zero_()
    bounds = torch.empty(8, dtype=i32, device="cuda")
    keys = torch.empty(V, dtype=i64, device="cuda")
    heads = torch.empty(V, dtype=i32, device="cuda")
    L.check(lib.i2sdf_points_bounds(L.ptr(vt), V, L.ptr(bounds), L.ptr(pstatus), st))
    L.check(lib.i2sdf_points_voxel_keys(L.ptr(vt), V, L.ptr(bounds), float(h), L.ptr(keys), L.ptr(pstatus), st))
    skeys, perm = torch.sort(keys, stable=True)
    L.check(lib.i2sdf_points_voxel_heads(L.ptr(skeys), V, L.ptr(heads), st))
    scan = torch.cumsum(heads, 0, dtype=i32)
    M = int(scan[-1])
    assert int(pstatus[0]) == 0
    vcell = g.new((V,), i32, "vertex_cell")
    cstart = g.new((M + 1,), i32, "cell_start")
    L.check(lib.i2sdf_simplify_vertex_cells(L.ptr(skeys), L.ptr(perm), L.ptr(scan), V, M, L.ptr(vcell), L.ptr(cstart), st), "vertex_cells")
    ckeys = g.new((3 * F,), i32, "corner_keys")
    cruns = g.new((M, 2), i32, "corner_runs")
    L.check(lib.i2sdf_simplify_corner_keys(L.ptr(ft), F, V, L.ptr(vcell), M, L.ptr(ckeys), L.ptr(status), st), "corner_keys")
    sck, cperm = torch.sort(ckeys, stable=True)
    L.check(lib.i2sdf_simplify_corner_runs(L.ptr(sck), F, M, L.ptr(cruns), st), "corner_runs")
    cell_v = g.new((M, 3), torch.float32, "cell verts")
    cell_n = None if nt is None else g.new((M, 3), torch.float32, "cell normals")
    cell_fb = g.new((M,), torch.uint8, "fallback")
    L.check(lib.i2sdf_simplify_cells(L.ptr(vt), L.ptr(nt), V, L.ptr(ft), F, L.ptr(bounds), float(h), float(reg), L.SIMPLIFY_CONTRACTIONS[contraction],
                                     L.ptr(skeys), L.ptr(perm), L.ptr(cstart), L.ptr(cperm), L.ptr(cruns), M, L.ptr(cell_v), L.ptr(cell_n),
                                     L.ptr(cell_fb), st), "cells")
    mapped = g.new((F, 3), i32, "mapped faces")
    hi, lo = g.new((F,), i64, "key_hi"), g.new((F,), i64, "key_lo")
    L.check(lib.i2sdf_simplify_face_keys(None, V, L.ptr(ft), F, L.ptr(vcell), M, L.SIMPLIFY_DROP_REPEATED, L.ptr(mapped), L.ptr(hi), L.ptr(lo),
                                         L.ptr(status), st), "face_keys")
    slo, p1 = torch.sort(lo, stable=True)
    shi, p2 = torch.sort(hi[p1], stable=True)
    slo, fperm = slo[p2].contiguous(), p1[p2].contiguous()
    keep = g.new((F,), torch.uint8, "keep")
    first = g.new((F,), i32, "first")
    L.check(lib.i2sdf_simplify_run_heads(L.ptr(shi), L.ptr(slo), L.ptr(fperm), F, L.ptr(keep), L.ptr(first), st), "run_heads")
    g.check()
    if F:
        assert bool((keep <= 1).all()) and int(first[0]) == 0
    keep_h = keep.cpu().numpy().astype(bool)
    mapped_h, cell_h = mapped.cpu().numpy().astype(np.int64), vcell.cpu().numpy().astype(np.int64)
    table_n = None if cell_n is None else cell_n.cpu().numpy()
    ov, of, on, used, new = S.compact(cell_v.cpu().numpy(), table_n, mapped_h, keep_h)
    return dict(verts=ov, faces=of, normals=on, vertex_map=np.where(used[cell_h], new[cell_h], -1).astype(np.int32),
                face_map=np.nonzero(keep_h)[0].astype(np.int32), fallback=cell_fb.cpu().numpy().astype(bool)[used], status=int(status.item()),
                cell_verts=cell_v.cpu().numpy())


def _same(got, want, what):
    assert got["verts"].shape == want["verts"].shape, (what, got["verts"].shape, want["verts"].shape)
    assert np.array_equal(got["verts"].view(np.int32), want["verts"].view(np.int32)), what
    assert np.array_equal(got["faces"], want["faces"]) and got["faces"].dtype == np.int32, what
    for k in ("vertex_map", "face_map", "fallback"):
        if k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert (got["normals"] is None) == (want["normals"] is None), what
    if want["normals"] is not None:
        assert np.array_equal(got["normals"].view(np.int32), want["normals"].view(np.int32)), what


def _host(res):
    m = res.mesh
    out = dict(verts=m.verts.cpu().numpy(), faces=m.faces.cpu().numpy(), normals=None if m.normals is None else m.normals.cpu().numpy(),
               vertex_map=res.vertex_map.cpu().numpy(), face_map=res.face_map.cpu().numpy())
    if hasattr(res, "fallback"):
        out["fallback"] = res.fallback.cpu().numpy()
    return out


def _fixtures():
    sv, sf = R.soup(4)
    i3, i2 = R.icosphere(3), R.icosphere(2)
    c8 = S.cube(8)
    return {"ico3_h0.1": (*i3, 0.1, True), "ico3_h0.25": (*i3, 0.25, True), "ico3_h3": (*i3, 3.0, False), "ico3_one_cell": (*i3, 5.0, False), "cube8": (*c8, 0.4, True),
            "soup3000": (*R.soup(3000), 0.2, False), "dup_shuffled": (i2[0], S.duplicated_shuffled(i2[1]), 0.2, False),
            "folded": (*S.folded_sheet(6), 0.2, False), "unreferenced": (*S.with_unreferenced(*i2), 0.25, True),
            "F0": (sv, sf[:0], 0.1, False), "F1": (sv, sf[:1], 0.1, True), "F2": (sv, sf[:2], 0.1, False)}


NAMES = ["ico3_h0.1", "ico3_h0.25", "ico3_h3", "ico3_one_cell", "cube8", "soup3000", "dup_shuffled", "folded", "unreferenced", "F0", "F1", "F2"]


def _case(name, by):
    if (name, by) not in _CACHE:
        v, f, h, with_normals = _fixtures()[name]
        n = S.vertex_normals(v) if with_normals else None
        v = S.shift(v, by)
        _CACHE[(name, by)] = (v, f, h, n, {c: S.simplify(v, f, h, c, normals=n, detail=True) for c in ("quadric", "average")})
    return _CACHE[(name, by)]


# ------------------------------------------------------------------------------------------------ 1. the law
@pytest.mark.parametrize("by", [0.0, 1000.0])
@pytest.mark.parametrize("name", NAMES)
def test_simplify_against_the_restatement(name, by):
    import i2sdf_amd as A
    v, f, h, n, want = _case(name, by)
    for c in ("quadric", "average"):
        raw = _raw_simplify(v, f, h, c, normals=n)
        assert raw["status"] == 0
        assert np.array_equal(raw["cell_verts"].view(np.int32), want[c]["cell_verts"].view(np.int32)), (name, c)      # every cell, referenced or not
        _same(raw, want[c], f"{name}+{by:g} {c} raw")
        res = A.simplify_vertex_clustering(_mesh(v, f, n), h, c)
        assert isinstance(res, A.SimplifyResult) and res.fallback.dtype == torch.bool and res.vertex_map.dtype == torch.int32
        got = _host(res)
        _same(got, want[c], f"{name}+{by:g} {c}")
        again = _host(A.simplify_vertex_clustering(_mesh(v, f, n), h, c))
        _same(again, got, f"{name}+{by:g} {c} second run")
    # With lo = min - h / 2 the unit sphere at h = 3 spans (p - lo) / h in [0.5, 1.17]: two cells an axis, eight cells, twelve faces --
    # not one cell.  It is one cell from h = 4 on; h = 5 is the case where everything collapses.
    if name == "ico3_h3" and by == 0.0:
        assert len(got["verts"]) == 8 and len(got["faces"]) == 12
    if name == "ico3_one_cell":
        assert len(got["faces"]) == 0 and len(got["verts"]) == 0 and (got["vertex_map"] == -1).all()
    # `average` is voxel_down_sample: the rows of the cells that survive
    down, _ = A.voxel_down_sample(_cuda(v), h)
    rows = np.unique(want["average"]["cell"][f.astype(np.int64)][want["average"]["face_map"]])
    assert np.array_equal(got["verts"].view(np.int32), down.cpu().numpy()[rows].view(np.int32))
    assert np.array_equal(down.cpu().numpy().view(np.int32), P.voxel_down_sample(v, h)[0].view(np.int32))
    q = want["quadric"]
    print(f"{name}+{by:g}: {len(f)} -> {len(q['faces'])} faces, {len(v)} -> {len(q['verts'])} vertices, {int(q['fallback'].sum())} fallbacks")


def test_empty_mesh_and_reg():
    import i2sdf_amd as A
    e = A.simplify_vertex_clustering((torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda")), 0.1)
    assert e.mesh.verts.shape == (0, 3) and e.mesh.faces.shape == (0, 3) and e.vertex_map.shape == (0,) and e.fallback.shape == (0,)
    v, f = R.icosphere(3)                                       # (curved: the regulariser moves the minimiser; on the cube's planes it does not)
    want = S.simplify(v, f, 0.25, reg=1e-6)
    _same(_host(A.simplify_vertex_clustering(_mesh(v, f), 0.25, reg=1e-6)), want, "reg = 1e-6")
    assert not np.array_equal(want["verts"], S.simplify(v, f, 0.25)["verts"])


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_nan_vertex_and_bad_face_index_are_refused():
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    v, f = R.icosphere(2)
    bad_v = v.copy()
    bad_v[17, 1] = np.nan
    with pytest.raises(I2SDFError, match="not finite"):
        A.simplify_vertex_clustering(_mesh(bad_v, f), 0.2)
    with pytest.raises(I2SDFError, match="21 bits"):
        A.simplify_vertex_clustering(_mesh(v, f), 1e-7)
    V = len(v)
    for bad in ([0, 1, V], [-1, 2, 3], [0, 1, 2 ** 31 - 1], [-2 ** 31, 4, 5]):
        bf = np.concatenate([f[:40], [bad], f[40:]], 0).astype(np.int32)
        raw = _raw_simplify(v, bf, 0.2)                         # canaries intact, the status bit set, the other faces as without it
        assert raw["status"] == 1
        want = S.simplify(v, f, 0.2)
        assert np.array_equal(raw["verts"].view(np.int32), want["verts"].view(np.int32))
        assert np.array_equal(raw["face_map"], np.where(want["face_map"] >= 40, want["face_map"] + 1, want["face_map"]))
        for call in (lambda m: A.simplify_vertex_clustering(m, 0.2), lambda m: A.simplify_vertex_clustering(m, 0.2, "average"), A.clean,
                     lambda m: A.topology(m).as_dict()):
            with pytest.raises(I2SDFError, match="outside"):
                call(_mesh(v, bf))
    torch.cuda.synchronize()
    assert A.topology(_mesh(v, f)).watertight                   # the device is still well


# ------------------------------------------------------------------------------------------------ 3. clean
@pytest.mark.parametrize("name", ["soup_of_ico", "dup_shuffled", "folded", "unreferenced", "F0", "F2"])
def test_clean_against_the_restatement(name):
    import i2sdf_amd as A
    if name == "soup_of_ico":
        iv, f0 = R.icosphere(2)
        v = iv[f0].reshape(-1, 3).copy()
        v[::2][v[::2] == 0.0] = -0.0                            # -0.0 = +0.0
        f = np.arange(3 * len(f0), dtype=np.int32).reshape(-1, 3)
        line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [9, 9, 9]], F32)
        n0 = len(v)
        v = np.concatenate([v, line], 0)
        f = np.concatenate([f[:10], [[0, 0, 1], [0, 3, 0]], f[10:], [[n0, n0 + 1, n0 + 2]], f[[4, 7]][:, [1, 2, 0]], f[[9]][:, [0, 2, 1]]], 0).astype(np.int32)
    else:
        v, f = _fixtures()[name][:2]
    n = S.vertex_normals(v)
    for kw in (dict(), dict(merge_vertices=False), dict(degenerate=False, zero_area=False), dict(duplicated=False), dict(zero_area=False),
               dict(merge_vertices=False, degenerate=False, zero_area=False, duplicated=False)):
        want = S.clean(v, f, n, **kw)
        res = A.clean(_mesh(v, f, n), **kw)
        assert isinstance(res, A.CleanResult)
        _same(_host(res), want, f"{name} {kw}")
        _same(_host(A.clean(_mesh(v, f), **kw)), S.clean(v, f, None, **kw), f"{name} {kw} without normals")
    if name == "soup_of_ico":
        res = A.clean(_mesh(v, f))
        assert res.mesh.verts.shape[0] == 162 and res.mesh.faces.shape[0] == 321 and res.mesh.normals is None


def test_clean_on_a_level_set_then_closest_point_routes_agree():
    import i2sdf_amd as A
    torch.manual_seed(0)
    net = A.I2SDFNetwork(A.synthetic_conf()).cuda().eval()      # 64 wide, geometric init: a sphere of radius about 0.6
    mesh = net.extract_mesh(A.uniform_axes(64, (-1.0, 1.0)))
    assert mesh.faces.shape[0] > 2000
    v, f, n = mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.normals.cpu().numpy()
    # a level set has its slivers only where a crossing lands on a lattice point: plant some, so that the test does not depend on luck
    f = np.concatenate([f, f[:5][:, [0, 0, 1]], f[5:9]], 0).astype(np.int32)
    v = np.concatenate([v, v[f[20]].mean(0, keepdims=True), v[f[20, :1]]], 0)                   # a copy of a vertex: merged
    n = np.concatenate([n, n[:2]], 0)
    f = np.concatenate([f, [[f[20, 0], len(v) - 1, f[20, 1]]]], 0).astype(np.int32)             # (a, a', b): zero area once merged or not
    res = A.clean(_mesh(v, f, n))
    _same(_host(res), S.clean(v, f, n), "level set")
    cv, cf = res.mesh.verts.cpu().numpy().astype(D), res.mesh.faces.cpu().numpy().astype(np.int64)
    assert len(cf) < len(f)
    assert ((cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 2] != cf[:, 0])).all()
    e, g = cv[cf[:, 1]] - cv[cf[:, 0]], cv[cf[:, 2]] - cv[cf[:, 0]]
    cross = np.stack([e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1], e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2], e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]], 1)
    assert (cross != 0.0).any(1).all()
    t = A.topology(res.mesh)
    assert t.as_dict() == {k: S.topology(cv, cf)[k] for k in S.TOPO_KEYS} and t.as_dict()["repeated_index_faces"] == 0
    gq = torch.Generator(device="cuda").manual_seed(5)
    q = (torch.rand(1500, 3, device="cuda", generator=gq) * 1.6 - 0.8).contiguous()
    a = A.closest_point(res.mesh[:2], q, route="bvh")
    b = A.closest_point(res.mesh[:2], q, route="brute")
    for x, y, name in zip(a[:5], b[:5], ("dist", "point", "face", "bary", "feature")):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name


# ------------------------------------------------------------------------------------------------ 4. topology
def _topo_fixtures():
    iv, ifc = R.icosphere(2)
    flipped = ifc.copy()
    flipped[5] = flipped[5, [0, 2, 1]]
    rep = np.concatenate([ifc[:30], [[3, 3, 4], [7, 8, 7]], ifc[30:]], 0).astype(np.int32)
    out = {k: v[:2] for k, v in _fixtures().items()}
    out.update(ico2=(iv, ifc), cap=W.cap(3), open_cube=S.cube_without_top(8), flipped=(iv, flipped), repeated=(iv, rep))
    return out


@pytest.mark.parametrize("name", NAMES + ["ico2", "cap", "open_cube", "flipped", "repeated"])
def test_topology_against_the_restatement(name):
    import i2sdf_amd as A
    v, f = _topo_fixtures()[name]
    want = S.topology(v, f)
    t = A.topology(_mesh(v, f))
    assert isinstance(t, A.MeshTopology) and t.counts.dtype == torch.int64 and t.counts.is_cuda
    got = t.as_dict()
    assert got == {k: want[k] for k in S.TOPO_KEYS}, (name, got, want)
    assert t.watertight == want["watertight"] and t.oriented == want["oriented"]
    assert A.topology(_mesh(v, f)).as_dict() == got
    print(f"{name}: {got}")
    if name in ("ico2", "ico3_h0.25"):
        assert t.watertight and t.oriented and got["euler"] == 2
    if name in ("cap", "open_cube"):
        assert not t.watertight and t.oriented and got["boundary_edges"] > 0
    if name == "flipped":
        assert t.watertight and not t.oriented and got["misoriented_edges"] == 3
    if name == "repeated":
        assert got["repeated_index_faces"] == 2 and t.watertight and got["euler"] == 2
    if name == "folded":
        assert not t.watertight and got["nonmanifold_edges"] > 0 and got["boundary_edges"] == 0      # inner edges carry four faces


def test_topology_of_the_simplified_icosphere():
    import i2sdf_amd as A
    v, f = R.icosphere(5)
    res = A.simplify_vertex_clustering(_mesh(v, f), 0.25)
    t = A.topology(res.mesh)
    assert res.mesh.verts.shape[0] == 314 and res.mesh.faces.shape[0] == 624
    assert t.watertight and t.oriented and t.as_dict()["euler"] == 2 and t.as_dict()["manifold_edges"] == 936
    _same(_host(res), S.simplify(v, f, 0.25), "icosphere(5)")


# ------------------------------------------------------------------------------------------------ 5. the network
def test_extract_mesh_simplify_is_the_three_calls():
    import i2sdf_amd as A
    torch.manual_seed(0)
    net = A.I2SDFNetwork(A.synthetic_conf()).cuda().eval()
    ax = A.uniform_axes(32, (-1.0, 1.0))
    plain = net.extract_mesh(ax)
    none = net.extract_mesh(ax, simplify=None)
    for a, b in zip(plain, none):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    h = 3.0 * float(ax.spacing[0])
    for c in ("quadric", "average"):
        byhand = A.simplify_vertex_clustering(A.clean(plain).mesh, h, c).mesh
        got = net.extract_mesh(ax, simplify=h, contraction=c)
        assert isinstance(got, A.Mesh) and 0 < got.faces.shape[0] < plain.faces.shape[0] // 4
        for a, b in zip(got, byhand):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rot = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    got = net.extract_mesh(ax, rot=rot, trans=torch.tensor([0.5, 0.0, -0.25]), simplify=h)
    byhand = A.simplify_vertex_clustering(A.clean(net.extract_mesh(ax, rot=rot, trans=torch.tensor([0.5, 0.0, -0.25]))).mesh, h).mesh
    for a, b in zip(got, byhand):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = S.topology(got.verts.cpu().numpy(), got.faces.cpu().numpy())
    assert A.topology(got).as_dict() == {k: want[k] for k in S.TOPO_KEYS}
