"""GPU: point-to-mesh queries (csrc/closest.hip, i2sdf_amd.mesh) held to the numpy restatement tests/closest_ref.py.
  1. the tree route, the brute route and the restatement agree bit for bit in dist, point, face, bary, feature -- and in sdist when
     the restatement is fed the device's own tables -- with canaries around every output; the tree is build_bvh's, unmodified;
  2. the pseudonormal tables against the restatement, and bitwise between two runs;
  3. the sign on the device: the sharp wedge against the exact convex test, the non-convex star against crossing parity;
  4. against the ray caster on the same tree;
  5. surface_scores.
The tables' tolerance.  The issue's bound is 1 fp32 ulp per component, because atan2 is correctly rounded on neither side.  A
component whose terms cancel (a vertex normal's tangential part on a symmetric mesh) is, on both sides, the fp64 rounding noise of
terms of magnitude up to pi: no ulp of ITS magnitude can hold there.  Seven corners or fewer per vertex, each angle * n_f good to
4 fp64 ulps of pi on either side, give 2 * 7 * 4 * pi * 2^-53 < 2^-45.  The test holds every component above 2^-20 to the issue's 1 fp32 ulp exactly, and the others
(cancellations: the entries are sums of terms of order 1) to 2^-45 absolute."""
import numpy as np
import pytest
import torch

import closest_ref as CR
import raycast_ref as R

pytestmark = pytest.mark.gpu

F32, D = np.float32, np.float64
CANARY = 64
_CACHE = {}
FIELDS = ("dist", "point", "face", "bary", "feature")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mesh(v, f):
    return _cuda(np.asarray(v, F32)), _cuda(np.asarray(f, np.int32).reshape(-1, 3))


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * CANARY,), fill, dtype=dtype, device="cuda")
    return buf, buf[CANARY:CANARY + n]


def _raw(route, v, f, q, max_dist=np.inf, normals=None, bvh=None):
    """the C ABI with guarded outputs -> dict of numpy arrays; canaries checked.  normals: device tensors (vnormal, enormal)"""
    from i2sdf_amd import lib as L
    from i2sdf_amd import mesh as M
    lib = L.load()
    n = len(q)
    vt, ft = _mesh(v, f)
    qt = _cuda(np.asarray(q, F32).reshape(n, 3))
    bufs = {"dist": _guarded(n, torch.float32, -7.5), "point": _guarded(3 * n, torch.float32, -7.5), "face": _guarded(n, torch.int32, -77),
            "bary": _guarded(2 * n, torch.float32, -7.5), "feature": _guarded(n, torch.uint8, 201), "status": _guarded(1, torch.int32, -77)}
    if normals is not None:
        bufs["sdist"] = _guarded(n, torch.float32, -7.5)
    p = {k: L.ptr(w) for k, (_, w) in bufs.items()}
    one = torch.zeros(4, dtype=torch.float32, device="cuda")
    tab = (None, None) if normals is None else tuple(L.ptr(t) if t.numel() else L.ptr(one) for t in normals)
    args = (L.ptr(qt), n, float(max_dist), *tab, p["dist"], p["point"], p["face"], p["bary"], p["feature"], p.get("sdist"), p["status"],
            L.stream_ptr())
    if route == "bvh":
        bvh = bvh or M.build_bvh((vt, ft))
        L.check(lib.i2sdf_closest_bvh(L.ptr(bvh.buffer), L.ptr(vt), len(v), L.ptr(ft), len(ft), *args), "i2sdf_closest_bvh")
    else:
        L.check(lib.i2sdf_closest_brute(L.ptr(vt), len(v), L.ptr(ft), len(ft), *args), "i2sdf_closest_brute")
    torch.cuda.synchronize()
    out = {}
    for k, (buf, w) in bufs.items():
        fill = buf[0].item()
        assert bool((buf[:CANARY] == fill).all()) and bool((buf[CANARY + w.numel():] == fill).all()), f"{route}: canary of {k} overwritten"
        out[k] = w.cpu().numpy()
    out["point"], out["bary"] = out["point"].reshape(n, 3), out["bary"].reshape(n, 2)
    out["status"] = int(out["status"][0])
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, what, fields=FIELDS):
    for k in fields:
        x, y = _bits(a[k]), _bits(np.asarray(b[k], a[k].dtype))
        assert np.array_equal(x, y), f"{what}: {k} differs in {int((x != y).reshape(len(x), -1).any(1).sum())} of {len(x)} rows"
    assert a["status"] == b["status"], (what, a["status"], b["status"])


def _fixtures():
    gv, gf = R.flat_grid()
    iv, ifc = R.icosphere(2)
    return {"ico2": (iv, ifc), "ico3": R.icosphere(3), "soup3000": R.soup(3000), "grid": (gv, gf), "wedge": CR.wedge(),
            "duplicated": CR.duplicated(iv, ifc), "bad_faces": CR.with_bad_faces(iv, ifc),
            "F0": (R.soup(4)[0], np.zeros((0, 3), np.int32)), "F1": (R.soup(4)[0], R.soup(4)[1][:1]), "F2": (R.soup(4)[0], R.soup(4)[1][:2])}


NAMES = ["ico2", "ico3", "soup3000", "grid", "wedge", "duplicated", "bad_faces", "F0", "F1", "F2"]


def _case(name, shift):
    """mesh, queries, and the restatement without max_dist (computed once)"""
    key = (name, shift)
    if key not in _CACHE:
        v, f = _fixtures()[name]
        v = (v.astype(D) + shift).astype(F32)
        q = CR.queries(v, f, 226, seed=31)                      # 226 + 160 special + 36 + 4 + 3 = 429 rows
        _CACHE[key] = (v, f, q, CR.closest(v, f, q))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. routes and law
@pytest.mark.parametrize("shift", [0.0, 1000.0])
@pytest.mark.parametrize("name", NAMES)
def test_tree_brute_and_restatement_agree_bit_for_bit(name, shift):
    from i2sdf_amd import mesh as M
    v, f, q, law = _case(name, shift)
    vt, ft = _mesh(v, f)
    bvh = M.build_bvh((vt, ft))                                # the unmodified build
    nm = M.pseudonormals((vt, ft))
    nm_np = (nm.vertex.cpu().numpy(), nm.edge.cpu().numpy())
    fb = f[law["face"][law["face"] >= 0]]
    full = dict(law)
    full["sdist"] = (CR.sign(v, f, q.astype(D), law["face"], law["feature"].astype(np.int64), law["c"], nm_np) * law["dist"]).astype(F32)
    hits = {}
    for max_dist in (np.inf, 0.05, 0.0):
        want = CR.limit(full, max_dist)
        for route in ("bvh", "brute"):
            got = _raw(route, v, f, q, max_dist, normals=(nm.vertex, nm.edge), bvh=bvh)
            _same(got, want, f"{name}+{shift:g} {route} max_dist={max_dist}", FIELDS + ("sdist",))
            plain = _raw(route, v, f, q, max_dist, bvh=bvh)
            _same(plain, want, f"{name}+{shift:g} {route} max_dist={max_dist} (no tables)")
        hits[max_dist] = int((want["face"] >= 0).sum())
    finite = int(np.isfinite(q).all(1).sum())
    if len(fb):
        assert hits[np.inf] == finite and 0 < hits[0.0] <= hits[0.05] < finite, hits      # every bound cuts something, none everything
        assert want["status"] & CR.BAD_POINT
    else:
        assert hits[np.inf] == 0
    if name == "bad_faces":
        assert law["status"] == CR.BAD_POINT | CR.BAD_FACE
    if name == "duplicated":
        assert (np.sort(f, 1)[law["face"][law["face"] >= 0]][:, None] == np.sort(f, 1)[None]).all(2).sum(1).min() == 2     # every hit has a twin


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 389, 2000])
def test_every_query_count(n):
    from i2sdf_amd import mesh as M
    if "counts" not in _CACHE:
        v, f = CR.with_bad_faces(*R.icosphere(2))
        q = np.concatenate([CR.queries(v, f, 1700, seed=41)] * 2)[:2000]
        _CACHE["counts"] = (v, f, q, CR.closest(v, f, q, 0.4, normals=CR.pseudonormals(v, f)))
    v, f, q, law = _CACHE["counts"]
    vt, ft = _mesh(v, f)
    want = {k: (x[:n] if isinstance(x, np.ndarray) else x) for k, x in law.items()}
    want["status"] = (CR.BAD_POINT if n and not np.isfinite(q[:n]).all() else 0) | CR.BAD_FACE        # n = 0 still reports the face bit
    for route in ("bvh", "brute"):
        _same(_raw(route, v, f, q[:n], 0.4), want, f"n={n} {route}")
    res = M.closest_point((vt, ft), _cuda(q[:n]), 0.4, route="auto")          # 326 faces: the tree
    assert res.sdist is None and res.dist.shape == (n,) and res.point.shape == (n, 3) and res.feature.dtype == torch.uint8
    assert np.array_equal(_bits(res.dist.cpu().numpy()), _bits(want["dist"])) and int(res.status.item()) == want["status"]


def test_front_end_routes_and_signed_distance():
    from i2sdf_amd import mesh as M
    v, f, q, law = _case("ico2", 0.0)
    vt, ft = _mesh(v, f)
    qt = _cuda(q)
    bvh = M.build_bvh((vt, ft))
    nm = M.pseudonormals(bvh)
    a = M.closest_point(bvh, qt, normals=nm)
    b = M.closest_point((vt, ft), qt, normals=nm, route="brute")
    c = M.closest_point(M.Mesh(vt, ft, vt), qt, route="bvh")
    for k in FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)) and torch.equal(getattr(a, k), getattr(c, k)), k
    assert torch.equal(a.sdist.view(torch.int32), b.sdist.view(torch.int32)) and c.sdist is None
    sd = M.signed_distance((vt, ft), qt)
    assert torch.equal(sd.view(torch.int32), a.sdist.view(torch.int32))
    assert np.array_equal(_bits(a.dist.cpu().numpy()), _bits(law["dist"]))
    inside = np.linalg.norm(q.astype(D), axis=1) < 0.97
    assert inside.sum() > 3 and bool((sd.cpu().numpy()[inside] < 0).all())
    cut = M.signed_distance(bvh, qt, nm, max_dist=0.05).cpu().numpy()
    assert np.isinf(cut).sum() > 100 and (np.abs(cut[np.isfinite(cut)]) <= F32(0.05)).all()


# ------------------------------------------------------------------------------------------------ 2. the tables
@pytest.mark.parametrize("name", ["ico2", "soup3000", "grid", "wedge", "bad_faces", "bumpy", "F0", "F1"])
def test_pseudonormal_tables(name):
    from i2sdf_amd import mesh as M
    v, f = CR.bumpy_sphere(2) if name == "bumpy" else _fixtures()[name]
    if name == "soup3000":
        v, f = v[:900], f[:300]
    vt, ft = _mesh(v, f)
    a, b = M.pseudonormals((vt, ft)), M.pseudonormals((vt, ft))
    torch.cuda.synchronize()
    assert torch.equal(a.vertex.view(torch.int32), b.vertex.view(torch.int32)) and torch.equal(a.edge.view(torch.int32), b.edge.view(torch.int32))
    assert a.vertex.shape == (len(v), 3) and a.edge.shape == (len(f), 3, 3)
    vn, en = CR.pseudonormals(v, f)
    worst = small = 0.0
    for got, want in ((a.vertex.cpu().numpy(), vn), (a.edge.cpu().numpy(), en)):
        ulp = np.spacing(np.abs(want)).astype(D)
        err = np.abs(got.astype(D) - want.astype(D))
        big = np.abs(want) > 2.0 ** -20
        if big.any():
            worst = max(worst, float((err / ulp)[big].max()))
        if (~big).any():
            small = max(small, float(err[~big].max()))
        assert (err <= np.where(big, ulp, 2.0 ** -45)).all(), (name, worst, small)
    print(f"{name}: largest table error {worst:.2f} fp32 ulp of the component; {small:.2e} absolute where it is below 2^-20")
    # the edge entries are not atan2's business: bitwise
    assert np.array_equal(_bits(a.edge.cpu().numpy()), _bits(en)), name


# ------------------------------------------------------------------------------------------------ 3. the sign
def test_sign_on_the_sharp_wedge_is_the_exact_convex_test():
    from i2sdf_amd import mesh as M
    from test_closest_ref import _wedge_queries
    v, f = CR.wedge()
    q = _wedge_queries()
    inside, well = CR.wedge_inside(q)
    vt, ft = _mesh(v, f)
    for route in ("bvh", "brute"):
        res = M.closest_point((vt, ft), _cuda(q), normals=M.pseudonormals((vt, ft)), route=route)
        sd = res.sdist.cpu().numpy()
        assert len(q) == 1600 and well.sum() > 1500
        assert int(((sd < 0) != inside)[well].sum()) == 0, route
        assert np.array_equal(np.abs(sd), res.dist.cpu().numpy())


def test_sign_on_a_non_convex_star_is_the_crossing_parity():
    from i2sdf_amd import mesh as M
    v, f = CR.bumpy_sphere(2)
    g = np.random.default_rng(7)
    q = g.uniform(-1.7, 1.7, (600, 3)).astype(F32)
    inside, well = CR.parity_inside(v, f, q, seed=8)            # on the CPU, fp64
    vt, ft = _mesh(v, f)
    sd = M.signed_distance(M.build_bvh((vt, ft)), _cuda(q)).cpu().numpy()
    assert well.sum() > 550 and 50 < inside.sum() < 500
    assert int(((sd < 0) != inside)[well].sum()) == 0


# ------------------------------------------------------------------------------------------------ 4. against the ray caster
def test_hit_points_of_the_ray_caster_lie_on_the_surface():
    from i2sdf_amd import mesh as M
    v, f = R.icosphere(2)
    vt, ft = _mesh(v, f)
    bvh = M.build_bvh((vt, ft))
    g = np.random.default_rng(51)
    o = g.normal(size=(600, 3))
    o = (3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(F32)
    d = (g.uniform(-0.5, 0.5, (600, 3)) - o).astype(F32)
    hits = M.ray_mesh_intersect(bvh, _cuda(o), _cuda(d))
    assert bool(hits.hit.all())
    t = hits.t.cpu().numpy()
    p = (t.astype(D)[:, None] * d.astype(D) + o.astype(D)).astype(F32)         # fma(t, d, o): the product is exact in fp64
    res = M.closest_point(bvh, _cuda(p))
    dist = res.dist.cpu().numpy().astype(D)
    unit = 2.0 ** -24 * (np.abs(o).max(1).astype(D) + np.abs(t).astype(D) * np.abs(d).max(1).astype(D))
    print(f"largest distance of a hit point to the surface: {(dist / unit).max():.2f} units of 2^-24 (|o| + |t| |d|)")
    assert (dist <= 16.0 * unit).all(), float((dist / unit).max())
    bary = hits.bary.cpu().numpy().astype(D)
    clear = np.minimum(bary.min(1), 1.0 - bary.sum(1)) > 1e-4
    assert clear.sum() > 500
    assert np.array_equal(res.face.cpu().numpy()[clear], hits.face.cpu().numpy()[clear])


# ------------------------------------------------------------------------------------------------ 5. surface_scores
def _draws(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda: {"u_face": torch.rand(n, device="cuda", generator=g), "u_bary": torch.rand(n, 2, device="cuda", generator=g)}
    return {"pred": mk(), "trgt": mk()}


def test_surface_scores():
    from i2sdf_amd import mesh as M
    v, f = R.icosphere(3)
    P = v[f].astype(D)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    h = np.abs((P[:, 0] * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)      # origin-to-plane distance of every face
    s = 1.0 - h.min()                                                      # the sagitta of the fixture
    cut = 0.02 * float(np.median(h))       # parallel faces lie 0.02 h apart: a threshold that cuts through both sets of distances
    vt, ft = _mesh(v, f)
    n, draws = 500, _draws(500, 3)
    same = M.surface_scores((vt, ft), (vt, ft), n, draws=draws)
    assert set(same) == {"Acc", "Comp", "Prec", "Recal", "F-score"} and all(x.is_cuda and x.dtype == torch.float64 for x in same.values())
    print(f"a mesh against itself: Acc {float(same['Acc']):.3e}, Comp {float(same['Comp']):.3e}")
    # Exactly 0 cannot be: sample_surface forms p0 + a e1 + b e2 in fp32, and the fp64 rule sees the rounding.  Per component: two
    # roundings at the coordinate's magnitude (1 ulp of the fixture's largest coordinate C together) and four at an edge component's
    # (edges of icosphere(3) are below C / 4: half an ulp of C together) -- 1.5 ulp, times sqrt(3) for the three axes: below 3 ulp.
    off = 3.0 * float(np.spacing(np.abs(v).max()))
    assert (np.abs(P[:, 1] - P[:, 0]).max(), np.abs(P[:, 2] - P[:, 0]).max()) < (np.abs(v).max() / 4,) * 2
    assert 0.0 <= float(same["Acc"]) <= off and 0.0 <= float(same["Comp"]) <= off, (float(same["Acc"]), float(same["Comp"]), off)
    assert float(same["F-score"]) == 1.0 and float(same["Prec"]) == 1.0 and float(same["Recal"]) == 1.0
    v2 = (v.astype(D) * 1.02).astype(F32)
    v2t = _cuda(v2)
    big = M.surface_scores(M.build_bvh((vt, ft)), (v2t, ft), n, threshold=cut, draws=draws)
    again = M.surface_scores((vt, ft), M.Mesh(v2t, ft, v2t), n, threshold=cut, draws=draws)
    for k in big:
        assert torch.equal(big[k].view(torch.int64), again[k].view(torch.int64)), k           # two runs, the same draws: the same bits
    assert 0.02 - s <= float(big["Acc"]) <= 0.02 + s and 0.02 - s <= float(big["Comp"]) <= 0.02 + s, (float(big["Acc"]), float(big["Comp"]), s)
    # the restatement on the device's own samples
    sp = M.sample_surface((vt, ft), n, draws["pred"])[0].cpu().numpy()
    st = M.sample_surface((v2t, ft), n, draws["trgt"])[0].cpu().numpy()
    d2 = CR.closest(v2, f, sp)["dist"].astype(D)              # pred samples -> trgt
    d1 = CR.closest(v, f, st)["dist"].astype(D)               # trgt samples -> pred
    prec, recal = (d2 < cut).mean(), (d1 < cut).mean()
    want = {"Acc": d2.mean(), "Comp": d1.mean(), "Prec": prec, "Recal": recal, "F-score": 2 * prec * recal / (prec + recal)}
    for k, w in want.items():
        assert abs(float(big[k]) - w) <= 1e-12 * max(abs(w), 1e-300), (k, float(big[k]), w)
    assert 0.0 < prec < 1.0 and 0.0 < recal < 1.0              # (the threshold cuts through both sets)
