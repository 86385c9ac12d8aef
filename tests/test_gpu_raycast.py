"""GPU: ray casting against meshes (csrc/bvh.hip, i2sdf_amd.mesh / i2sdf_amd.trace) held to the numpy restatement tests/raycast_ref.py.
  1. the tree a build leaves on the device IS the restatement's: keys, child links, leaf order, every box bitwise, every leaf once;
  2. the BVH route equals the brute route -- and the restatement's fp32 law -- bit for bit, with canaries around every output;
  3. against the restatement in fp64 on well-posed rays;
  4. watertightness on the device, both routes;
  5. `occluded` is the closest-hit flag;
  6. the mesh tracer as `intersect_func` of get_incident_radiance / trace_surface / render_surface / RenderingLayer."""
import numpy as np
import pytest
import torch

import raycast_ref as R
from test_raycast_ref import _watertight_cases

pytestmark = pytest.mark.gpu

F32 = np.float32
CANARY = 64
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mesh(v, f):
    return _cuda(np.asarray(v, F32)), _cuda(np.asarray(f, np.int32))


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * CANARY,), fill, dtype=dtype, device="cuda")
    return buf, buf[CANARY:CANARY + n]


def _raw_trace(route, v, f, o, d, t0, t1, cull="none", any_hit=False, bvh=None):
    """the C ABI with guarded outputs -> dict of numpy arrays (t, face, bary, hit, status); canaries checked"""
    from i2sdf_amd import lib as L
    from i2sdf_amd import mesh as M
    lib = L.load()
    n = len(o)
    vt, ft = _mesh(v, f)
    ot, dt_ = _cuda(np.asarray(o, F32)), _cuda(np.asarray(d, F32))
    t0t = _cuda(np.broadcast_to(np.asarray(t0, F32), (n,)).copy())
    t1t = _cuda(np.broadcast_to(np.asarray(t1, F32), (n,)).copy())
    bufs = {"t": _guarded(n, torch.float32, -7.5), "face": _guarded(n, torch.int32, -77), "bary": _guarded(2 * n, torch.float32, -7.5),
            "hit": _guarded(n, torch.uint8, 201), "status": _guarded(1, torch.int32, -77)}
    p = {k: L.ptr(w) for k, (_, w) in bufs.items()}
    args = (L.ptr(ot), L.ptr(dt_), L.ptr(t0t), L.ptr(t1t), n, L.RAYCAST_CULL[cull], int(any_hit), p["t"], p["face"], p["bary"], p["hit"],
            p["status"], L.stream_ptr())
    if route == "bvh":
        bvh = bvh or M.build_bvh((vt, ft))
        L.check(lib.i2sdf_bvh_trace(L.ptr(bvh.buffer), len(f), *args), "i2sdf_bvh_trace")
    else:
        L.check(lib.i2sdf_mesh_trace_brute(L.ptr(vt), len(v), L.ptr(ft), len(f), *args), "i2sdf_mesh_trace_brute")
    torch.cuda.synchronize()
    out = {}
    for k, (buf, w) in bufs.items():
        fill = buf[0].item()
        assert bool((buf[:CANARY] == fill).all()) and bool((buf[CANARY + w.numel():] == fill).all()), f"{route}: canary of {k} overwritten"
        if any_hit and k in ("t", "face", "bary"):
            assert bool((w == fill).all()), f"{route}: any_hit wrote {k}"
            continue
        out[k] = w.cpu().numpy()
    if "bary" in out:
        out["bary"] = out["bary"].reshape(n, 2)
    assert set(np.unique(out["hit"]).tolist()) <= {0, 1}
    out["hit"] = out["hit"].astype(bool)
    out["status"] = int(out["status"][0])
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, what):
    for k in ("t", "face", "bary", "hit"):
        assert np.array_equal(_bits(a[k]), _bits(np.asarray(b[k], a[k].dtype))), f"{what}: {k} differs in {int((_bits(a[k]) != _bits(np.asarray(b[k], a[k].dtype))).sum())} places"
    assert a["status"] == b["status"], (what, a["status"], b["status"])


# ------------------------------------------------------------------------------------------------ 1. the tree
def _tree_meshes():
    sv, sf = R.soup(400, seed=7)
    for F in (1, 2, 3, 64, 65):
        yield f"soup{F}", sv, sf[:F]
    for s, F in ((2, 320), (3, 1280)):
        v, f = R.icosphere(s)
        assert len(f) == F
        yield f"ico{F}", v, f
    yield "identical5000", sv, np.tile(sf[:1], (5000, 1))
    a, af = R.soup(200, seed=8)
    yield "two_clusters", np.concatenate([a, a + F32(1e4)]), np.concatenate([af, af + len(a)])
    bad = sf[:100].copy()
    bad[3], bad[50] = (0, 1, 10 ** 6), (-1, 2, 3)
    nv = sv.copy()
    nv[3 * 70] = np.nan
    yield "bad_faces", nv, bad


@pytest.mark.parametrize("name,v,f", list(_tree_meshes()), ids=[m[0] for m in _tree_meshes()])
def test_the_tree_on_the_device_is_the_restatements(name, v, f):
    from i2sdf_amd import lib as L
    lib = L.load()
    vt, ft = _mesh(v, f)
    F = len(f)
    nbytes = int(lib.i2sdf_bvh_bytes(F))
    buf, w = _guarded(nbytes, torch.uint8, 201)
    assert w.data_ptr() % 16 == 0
    kbuf, keys = _guarded(F, torch.int64, -77)
    st = L.stream_ptr()
    L.check(lib.i2sdf_bvh_keys(L.ptr(vt), len(v), L.ptr(ft), F, L.ptr(w), L.ptr(keys), st), "i2sdf_bvh_keys")
    want_keys = R.morton_keys(v, f)
    assert np.array_equal(keys.cpu().numpy(), want_keys)
    skeys = torch.sort(keys, stable=True)[0].contiguous()
    L.check(lib.i2sdf_bvh_build(L.ptr(vt), len(v), L.ptr(ft), F, L.ptr(skeys), L.ptr(w), st), "i2sdf_bvh_build")
    torch.cuda.synchronize()
    for b, n in ((buf, nbytes), (kbuf, F)):
        fill = b[0].item()
        assert bool((b[:CANARY] == fill).all()) and bool((b[CANARY + n:] == fill).all())
    raw = w.cpu().numpy()
    sk = np.sort(want_keys)
    nodes = raw[256:256 + 64 * F].view(np.int32).reshape(F, 16)[:max(F - 1, 0)]
    leaves = raw[256 + 64 * F:256 + 112 * F].view(np.int32).reshape(F, 12)
    child = R.karras(sk)
    assert np.array_equal(nodes[:, 12:14], child)
    want_box, seen = R.boxes(v, f, sk, child)
    assert (seen == 1).all()
    got_box = nodes[:, :12].reshape(-1, 2, 2, 3)
    assert np.array_equal(got_box, want_box.view(np.int32)), f"{int((got_box != want_box.view(np.int32)).any((1, 2, 3)).sum())} nodes differ"
    order = (sk & 0xffffffff).astype(np.int64)
    fv = R.valid_faces(v, f)
    assert np.array_equal(leaves[:, 9], np.where(fv[order], order, -1))
    ok = fv[order]
    assert np.array_equal(leaves[ok, :9], v[f[order[ok]]].reshape(-1, 9).view(np.int32))
    flags = int(raw[32:36].view(np.int32)[0])
    assert flags == (0 if fv.all() else R.BAD_FACE)


# ------------------------------------------------------------------------------------------------ 2. routes
def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _rays_around(n, seed, scale=1.0):
    """origins inside and outside the unit ball, directions towards a point near the centre (half of them) or anywhere"""
    g = np.random.default_rng(seed)
    o = _unit(g.normal(size=(n, 3))) * np.where(np.arange(n) % 2 == 0, g.uniform(0, 0.5, n), g.uniform(1.5, 3.0, n))[:, None]
    aim = g.uniform(-0.7, 0.7, (n, 3))
    d = np.where((np.arange(n) % 4 < 3)[:, None], aim - o, g.normal(size=(n, 3)))
    d = d * g.uniform(0.3, 3.0, (n, 1))                        # directions are not unit
    return (o * scale).astype(F32), (d * scale).astype(F32)


def _route_cases():
    for s in (2, 3):
        v, f = R.icosphere(s)
        o, d = _rays_around(389, s)
        yield f"ico{s}", v, f, o, d, 0.0, np.inf
    sv, sf = R.soup(3000)
    o, d = _rays_around(2000, 5)
    yield "soup3000", sv, sf, o, d, 0.0, np.inf
    cases = list(_watertight_cases())
    for name, v, f, o, d in cases[1:]:
        yield name, v, f, o, d, 0.0, np.inf
    _, gv, gf, o, d = cases[2]
    perm = np.random.default_rng(9).permutation(2 * len(gf))
    yield "grid_twice_shuffled", gv, np.concatenate([gf, gf])[perm], o, d, 0.0, np.inf
    # faces that are never hit, mixed in
    mv, mf = R.soup(300, seed=6)
    mv = np.concatenate([mv, [[np.nan, 0, 0], [np.inf, 0, 0]]]).astype(F32)
    extra = np.array([[0, 1, 10 ** 6], [-5, 1, 2], [0, 1, len(mv) - 2], [3, 4, len(mv) - 1], [6, 6, 7], [9, 10, 9], [12, 12, 12]], np.int32)
    mf = np.concatenate([mf[:100], extra, mf[100:]])
    o, d = _rays_around(500, 7)
    yield "never_hit_faces", mv, mf, o, d, 0.0, np.inf
    # axis-parallel rays, with zero components, from origins that lie on box planes (vertex coordinates)
    g = np.random.default_rng(8)
    o = sv[g.integers(0, len(sv), 600)].copy()
    o[::2, 2] -= 3.0
    d = np.eye(3, dtype=F32)[g.integers(0, 3, 600)] * g.choice([-1.0, 1.0, 0.25], (600, 1)).astype(F32)
    d[::2] = (0, 0, 1)
    d[1::4, 1] = 0.5                                           # one zero component left
    yield "axis_rays_on_box_planes", sv, sf, o, d, -np.inf, np.inf
    # rays that hit nothing by decree
    o, d = _rays_around(200, 10)
    o[3, 1], d[10, 2], d[20], o[30, 0] = np.nan, np.inf, 0.0, -np.inf
    t0, t1 = np.zeros(200, F32), np.full(200, np.inf, F32)
    t0[40], t1[50], t1[60] = np.nan, np.nan, -1.0
    yield "nan_rays", sv, sf, o, d, t0, t1
    # windows that cut the first hit off: from it on, or up to just before it
    o, d = _rays_around(400, 11)
    first = R.trace(sv, sf, o, d, dt=F32)
    t0 = np.where(first["hit"] & (np.arange(400) % 2 == 0), first["t"], 0).astype(F32)           # t_min is exclusive: the first hit goes
    t1 = np.where(first["hit"] & (np.arange(400) % 2 == 1), np.nextafter(first["t"], F32(0)), np.inf).astype(F32)
    yield "windows", sv, sf, o, d, t0, t1
    yield "no_faces", sv, sf[:0], o, d, 0.0, np.inf


def _route_case(name):
    if "cases" not in _CACHE:
        _CACHE["cases"] = {c[0]: c[1:] for c in _route_cases()}
    return _CACHE["cases"][name]


def _law(name, cull):
    key = ("law", name, cull)
    if key not in _CACHE:
        v, f, o, d, t0, t1 = _route_case(name)
        _CACHE[key] = R.trace(v, f, o, d, t0, t1, cull, F32)
    return _CACHE[key]


ROUTE_CASES = ("ico2", "ico3", "soup3000", "grid_oblique", "grid_axis", "grid_twice_shuffled", "never_hit_faces", "axis_rays_on_box_planes",
               "nan_rays", "windows", "no_faces")


@pytest.mark.parametrize("cull", ["none", "back"])
@pytest.mark.parametrize("name", ROUTE_CASES)
def test_bvh_route_equals_brute_route_and_the_law_bit_for_bit(name, cull):
    v, f, o, d, t0, t1 = _route_case(name)
    brute = _raw_trace("brute", v, f, o, d, t0, t1, cull)
    bvh = _raw_trace("bvh", v, f, o, d, t0, t1, cull)
    _same(bvh, brute, f"{name}/{cull}: bvh against brute")
    _same(brute, _law(name, cull), f"{name}/{cull}: brute against the restatement")
    miss = ~brute["hit"]
    t1n = np.broadcast_to(np.asarray(t1, F32), (len(o),))
    assert (brute["face"][miss] == -1).all() and (brute["bary"][miss] == 0).all() and np.array_equal(_bits(brute["t"][miss]), _bits(t1n[miss].copy()))
    if name == "grid_twice_shuffled" and cull == "none":           # (from below, every face of the sheet is a back face)
        assert brute["hit"].all()
    if name == "windows" and cull == "none":
        first = R.trace(v, f, o, d, dt=F32)
        assert (first["hit"].sum() > 100) and (brute["face"][first["hit"]] != first["face"][first["hit"]]).all()
    # occluded is the closest-hit flag, by both routes (5.)
    for route in ("brute", "bvh"):
        anyh = _raw_trace(route, v, f, o, d, t0, t1, cull, any_hit=True)
        assert np.array_equal(anyh["hit"], brute["hit"]) and anyh["status"] == brute["status"], (name, route)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 389, 2000])
def test_ray_counts(n):
    v, f = R.icosphere(3)
    o, d = _rays_around(2000, 12)
    o, d = o[:n], d[:n]
    brute = _raw_trace("brute", v, f, o, d, 0.0, np.inf)
    bvh = _raw_trace("bvh", v, f, o, d, 0.0, np.inf)
    _same(bvh, brute, f"{n} rays")
    _same(brute, R.trace(v, f, o, d, dt=F32), f"{n} rays, restatement")


def test_front_end_routes_bounds_and_occluded():
    import i2sdf_amd as A
    v, f = R.icosphere(2)
    o, d = _rays_around(389, 13)
    vt, ft = _mesh(v, f)
    ot, dt_ = _cuda(o), _cuda(d)
    bvh = A.build_bvh((vt, ft))
    assert isinstance(bvh, A.MeshBVH) and A.build_bvh(bvh) is bvh
    law = R.trace(v, f, o, d, 0.25, 2.0, "back", F32)
    t0 = torch.full((389,), 0.25, device="cuda")
    for mesh, route, lo in ((bvh, "auto", 0.25), ((vt, ft), "bvh", t0), ((vt, ft), "brute", 0.25), (A.Mesh(vt, ft, vt), "auto", t0.double())):
        got = A.ray_mesh_intersect(mesh, ot, dt_.double(), lo, 2.0, cull="back", route=route)
        assert got.hit.dtype == torch.bool and got.face.dtype == torch.int32 and tuple(got.bary.shape) == (389, 2)
        out = {"t": got.t.cpu().numpy(), "face": got.face.cpu().numpy(), "bary": got.bary.cpu().numpy(), "hit": got.hit.cpu().numpy(),
               "status": int(got.status.item())}
        _same(out, law, route)
        occ = A.occluded(mesh, ot, dt_, lo, 2.0, cull="back", route=route)
        assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), law["hit"])
    assert 50 < law["hit"].sum() < 389
    empty = A.ray_mesh_intersect((vt, ft[:0]), ot, dt_)
    assert not empty.hit.any() and (empty.face == -1).all() and torch.isinf(empty.t).all()
    with pytest.raises(ValueError):
        A.ray_mesh_intersect(bvh, ot.cpu(), dt_)


# ------------------------------------------------------------------------------------------------ 3. fp64
def _well_posed(v, f, o, d):
    """fp64 nearest hit of every ray, and whether the ray is well posed (barycentric margin, no second face within 1e-4, t inside its bounds)"""
    T, M = R.all_hits(v, f, o, d, 0.0, np.inf, dt=np.float64)
    Tf = np.where(np.isnan(T), np.inf, T)
    face = Tf.argmin(1)
    r = np.arange(len(o))
    t = Tf[r, face]
    hit = np.isfinite(t)
    others = Tf.copy()
    others[r, face] = np.inf
    with np.errstate(invalid="ignore"):
        alone = ~(np.abs(others - t[:, None]) <= 1e-4 * np.abs(t[:, None])).any(1)
    margin = M[r, face] >= 1e-4
    inside = t * (1 - 1e-4) > 0.0                               # (t_max is infinite)
    return np.where(hit, face, -1), t, hit & alone & margin & inside, hit


@pytest.mark.parametrize("fixture", ["ico3", "soup3000"])
def test_against_the_fp64_restatement_on_well_posed_rays(fixture):
    """Measured with numpy alone, no device: the restatement in fp32 against itself in fp64 on these rays gives the same face on every
    well-posed ray and the same hit flag on all 2000; largest |t32 - t64| / t64 = 4.37e-7 (ico3: 1530 hits, all well posed) and 5.20e-6
    (soup3000: 1498 hits, 1497 well posed).  The bar is 4 x that deviation -- 1.75e-6 and 2.08e-5 -- formed in the test from the
    restatement's own two runs, never from the device's result.  Well posed must be >= 99 % of the rays whose fp64 trace hits anything
    (the three conditions are conditions on a nearest hit; a ray without one has none to judge)."""
    v, f = (R.icosphere(3) if fixture == "ico3" else R.soup(3000))
    o, d = _rays_around(2000, 21 if fixture == "ico3" else 22)
    face64, t64, good, hit64 = _well_posed(v, f, o, d)
    assert good.sum() >= 0.99 * hit64.sum() and hit64.sum() > 500, (int(good.sum()), int(hit64.sum()))
    law32 = R.trace(v, f, o, d, dt=F32)
    assert np.array_equal(law32["face"][good], face64[good]) and np.array_equal(law32["hit"], hit64)
    dev32 = float((np.abs(law32["t"][good].astype(np.float64) - t64[good]) / t64[good]).max())
    bar = 4.0 * dev32
    print(f"{fixture}: {int(good.sum())} well-posed of {int(hit64.sum())} hits; restatement fp32 vs fp64 {dev32:.3e}, bar {bar:.3e}")
    for route in ("bvh", "brute"):
        got = _raw_trace(route, v, f, o, d, 0.0, np.inf)
        assert got["status"] == law32["status"] == 0
        assert np.array_equal(got["face"][good], face64[good]) and np.array_equal(got["hit"], hit64), route
        err = float((np.abs(got["t"][good].astype(np.float64) - t64[good]) / t64[good]).max())
        print(f"  {route}: {err:.3e}")
        assert err <= bar, (route, err, bar)


# ------------------------------------------------------------------------------------------------ 4. watertightness
@pytest.mark.parametrize("route", ["bvh", "brute"])
def test_watertight_on_the_device(route):
    for name, v, f, o, d in _watertight_cases():
        got = _raw_trace(route, v, f, o, d, 0.0, np.inf)
        assert got["hit"].all(), (name, route, int((~got["hit"]).sum()))


# ------------------------------------------------------------------------------------------------ 6. integration
H = 2.0 / 63.0


def _sphere_net(which):
    key = ("net", which)
    if key not in _CACHE:
        from i2sdf_amd import I2SDFNetwork, marching_cubes, uniform_axes
        from i2sdf_amd.config import plumbing_conf, synthetic_conf
        from oracle import i2sdf_oracle as orc
        conf, ocfg = (synthetic_conf(), orc.synthetic_cfg()) if which == "synthetic" else (plumbing_conf(), orc.plumbing_cfg())
        net = I2SDFNetwork(conf)
        net.load_state_dict(orc.init_params(ocfg, seed=3))          # the geometric init: a sphere of radius ~0.6, positive outside
        net = net.cuda().eval()
        vol = net.sdf_volume(uniform_axes(64, (-1.0, 1.0)))
        mesh = marching_cubes(vol, 0.0, spacing=(H, H, H), origin=(-1.0, -1.0, -1.0))
        assert mesh.faces.shape[0] > 1000
        _CACHE[key] = (net, mesh)
    return _CACHE[key]


def _scene_rays(n, seed):
    """from the shell of radius 1.5: three rays in four towards a point within 0.4 of the centre (they meet the sphere of radius ~0.6
    at |d.n| >= 0.74), the fourth towards a point 0.75 .. 0.95 from it (most of those pass the sphere by)"""
    g = np.random.default_rng(seed)
    o = _unit(g.normal(size=(n, 3))) * 1.5
    r = np.where(np.arange(n) % 4 < 3, 0.4 * g.uniform(0, 1, n) ** (1 / 3), g.uniform(0.75, 0.95, n))
    d = _unit(_unit(g.normal(size=(n, 3))) * r[:, None] - o)
    return _cuda(o.astype(F32)), _cuda(d.astype(F32))


def _input(o, d):
    return {"uv": o, "rays": {"cam_loc": o, "dirs": d, "dnorm": torch.ones(o.shape[0], device="cuda")}}


@pytest.mark.parametrize("which", ["plumbing", "synthetic"])
def test_mesh_tracer_as_intersect_func(which):
    """The sphere tracer runs with step_scale 0.5: at its initialisation the 64-wide net is not 1-Lipschitz (|grad sdf| up to 1.74 along
    these rays, its level set a lumpy body of radius 0.34 .. 0.71), and a full first step from radius 1.5 (f = 1.89) lands behind the
    whole body, where f is positive again: the march then reports a MISS on rays whose sdf goes down to -0.18 in between (seen on five
    of these rays).  The mesh tracer has no such limit.
    Observed: max |t_mesh - t_sphere| over the rays both tracers hit with |d.n| >= 0.5 is printed by the test in units of h = 2 / 63, the
    bound (the chord sag h^2 kappa / 8 is about 2e-4): 0.046 h on the 64-wide net (294 rays), 0.059 h on the 256-wide net (303 rays)."""
    from i2sdf_amd.trace import HIT, MISS
    net, mesh = _sphere_net(which)
    n = 389
    o, d = _scene_rays(n, 31)
    sphere = net.sphere_tracer(t_min=0.0, t_max=4.0, step_scale=0.5, max_steps=128)
    before = {"default": net.get_incident_radiance(o, d), "sphere": net.get_incident_radiance(o, d, intersect_func=sphere),
              "surface": net.render_surface(_input(o, d), t_min=0.0, t_max=4.0, step_scale=0.5, max_steps=128)}
    tracer = net.mesh_tracer(mesh)
    rad = net.get_incident_radiance(o, d, intersect_func=tracer)
    out = net.render_surface(_input(o, d), intersect_func=tracer)
    assert rad.shape == (n, 3) and torch.equal(rad, out["rgb_values"])
    hit = out["hit"]
    assert 100 < int(hit.sum()) < n and torch.equal(out["status"], torch.where(hit, HIT, MISS).to(torch.int32))
    for k in ("rgb_values", "points", "normal_map", "feature_vectors"):
        assert bool((out[k][~hit] == 0).all()), k
    assert out["face"].dtype == torch.int32 and bool((out["face"][hit] >= 0).all()) and bool((out["face"][~hit] == -1).all())
    assert tuple(out["bary"].shape) == (n, 2)
    # the direct form and trace_surface carry the same hits; split_n_pixels changes nothing
    ts = tracer(o, d)
    assert torch.equal(ts["t"], out["t"]) and torch.equal(ts["face"], out["face"]) and "rgb_values" not in ts
    split = net.render_surface(_input(o, d), split_n_pixels=100, intersect_func=tracer)
    assert all(torch.equal(split[k], out[k]) for k in out)
    # rgb at the hits is rgb_forward at the returned t
    eng = net._engine_for(torch.device("cuda:0"))
    with torch.no_grad():
        fw = eng.sdf_forward_grad(rays=(o, d, out["t"].reshape(n, 1), 1), want_grad=True, save=False)
        rgb, _, _ = eng.rgb_forward(d, 1, fw["feat"], n, save=False, fw=fw)
    assert torch.equal(rgb[hit], out["rgb_values"][hit])
    # the hit lies on the mesh: the barycentric point of the face is the ray's point
    vf = mesh.verts[mesh.faces[out["face"][hit].long()].long()].double()
    u, w = out["bary"][hit][:, :1].double(), out["bary"][hit][:, 1:].double()
    on_face = u * vf[:, 0] + w * vf[:, 1] + (1 - u - w) * vf[:, 2]
    assert float((on_face - (o[hit].double() + out["t"][hit].double().unsqueeze(1) * d[hit].double())).abs().max()) < 1e-5
    # against the sphere tracer
    ss = sphere(o, d)
    s_hit = ss["status"] == HIT
    facing_s = s_hit & ((ss["normal_map"] * d).sum(1).abs() >= 0.5)
    fn = torch.nn.functional.normalize(torch.cross(vf[:, 1] - vf[:, 0], vf[:, 2] - vf[:, 0], dim=1), dim=1).float()
    facing_m = torch.zeros_like(hit)
    facing_m[hit] = (fn * d[hit]).sum(1).abs() >= 0.5
    assert bool(hit[facing_s].all()), "the sphere tracer hits head-on where the mesh tracer misses"
    assert bool(s_hit[facing_m].all()), ("the mesh tracer hits head-on where the sphere tracer ends with", ss["status"][facing_m & ~s_hit].tolist())
    both = facing_s & hit
    gap = float((out["t"][both] - ss["t"][both]).abs().max())
    print(f"{which}: {int(both.sum())} rays, max |t_mesh - t_sphere| = {gap:.3e} = {gap / H:.4f} h")
    assert int(both.sum()) > 100 and gap <= H
    # bounds and culling of the tracer: a window that ends before the sphere misses everything; the far side is a back face
    assert not bool(net.mesh_tracer(mesh, t_max=0.5)(o, d)["hit"].any())
    # (the 64-wide net's level set is a lumpy closed surface, not convex: a ray may leave it and enter it again)
    def along(res):                                           # face normal . d at the hits of `res`
        q = mesh.verts[mesh.faces[res["face"][res["hit"]].long()].long()]
        return (torch.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], dim=1) * d[res["hit"]]).sum(1)
    back = net.mesh_tracer(mesh, t_min=0.0, cull="back")(o, d)
    assert torch.equal(back["t"], out["t"]) and bool((along(out) < 0).all())        # from outside, the first face met is a front face
    far = net.mesh_tracer(mesh, t_min=out["t"] + 0.05)(o, d)
    far_culled = net.mesh_tracer(mesh, t_min=out["t"] + 0.05, cull="back")(o, d)
    assert bool((far["t"][far["hit"]] > out["t"][far["hit"]] + 0.05).all()) and bool((along(far_culled) < 0).all())
    leaving = torch.zeros_like(hit)
    leaving[far["hit"]] = along(far) > 0                      # the next face is where the ray leaves the body: a back face
    assert int(leaving.sum()) > 100 and bool((~far_culled["hit"][leaving] | (far_culled["t"][leaving] > far["t"][leaving])).all())
    # nothing of the earlier routes moved
    after = {"default": net.get_incident_radiance(o, d), "sphere": net.get_incident_radiance(o, d, intersect_func=sphere),
             "surface": net.render_surface(_input(o, d), t_min=0.0, t_max=4.0, step_scale=0.5, max_steps=128)}
    assert torch.equal(before["default"], after["default"]) and torch.equal(before["sphere"], after["sphere"])
    assert all(torch.equal(before["surface"][k], after["surface"][k]) for k in before["surface"])
    assert torch.equal(before["sphere"], before["surface"]["rgb_values"])
    assert torch.equal(net.render_surface(_input(o, d), intersect_func=sphere)["rgb_values"], before["sphere"])


def test_rendering_layer_with_a_mesh_tracer_and_refusals():
    from i2sdf_amd import RenderingLayer
    net, mesh = _sphere_net("plumbing")
    tracer = net.mesh_tracer(mesh)
    layer = RenderingLayer(4, 100)
    n = 64
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.rand(*s, generator=g).cuda()
    nrm = torch.nn.functional.normalize(r(n, 3) - 0.5, dim=1)
    pts = nrm * 1.2                                            # outside the sphere, looking around
    view, samples = torch.nn.functional.normalize(r(n, 3) - 0.5, dim=1), r(n, 4, 3)

    class ByHand:                                              # the same radiance, fetched without the hook
        def get_incident_radiance(self, p, d_, f):
            assert f is None
            return net.render_surface(_input(p.detach().float().contiguous(), d_.detach().float().contiguous()), intersect_func=tracer)["rgb_values"]

    res = []
    for model, hook in ((net, tracer), (ByHand(), None)):
        Kd, Ks, rough = (t.clone().requires_grad_(True) for t in (r(n, 3) * 0 + 0.5, r(n, 3) * 0 + 0.3, r(n, 1) * 0 + 0.4))
        cd, cs, mask = layer(model, pts, view, Kd, Ks, -nrm, rough, intersect_func=hook, samples=samples)
        (cd.sum() + 2 * cs.sum()).backward()
        res.append((cd.detach(), cs.detach(), mask, Kd.grad, Ks.grad, rough.grad))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert all(bool(torch.isfinite(t).all()) for t in res[0] if t.dtype.is_floating_point) and float(res[0][0].abs().sum()) > 0
    z = torch.zeros(4, 3, device="cuda")
    other, _ = _sphere_net("synthetic")
    for bad in (lambda *a: None, other.mesh_tracer(mesh), other.sphere_tracer()):
        with pytest.raises(NotImplementedError, match="intersect_func"):
            net.get_incident_radiance(z, z, intersect_func=bad)
        with pytest.raises(NotImplementedError, match="intersect_func"):
            net.render_surface(_input(z, z), intersect_func=bad)
    with pytest.raises(TypeError, match="mesh tracer"):
        net.trace_surface(_input(z, z), intersect_func=tracer, eps=1e-4)
