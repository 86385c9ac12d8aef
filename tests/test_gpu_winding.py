"""GPU: generalized winding numbers (csrc/winding.hip, i2sdf_amd.mesh) held to the numpy restatement tests/winding_ref.py.
  1. the moments table downloaded from the device against the restatement's pass over the downloaded tree, bitwise between two runs;
  2. the brute route against the exact sum, and the tree route at beta = inf, 2, 3 against the restatement of the same rule on the same
     tree AND the same table (the acceptance test is exact fp64 on the same bits, so the accepted nodes are identical);
  3. queries on vertices, edges and faces; every query count; F = 0, 1, 2; canaries around every buffer;
  4. inside / signed_distance(sign="winding") on the cube without its top, and on a level set against the network's own sign.

The bar of the sums (derived, not chosen).  A face term is 2 atan2(det, den) with det and den the same bits on both sides (held on
the host by test_winding_host.py).  The device library's atan2 is built to the OpenCL C bound of 6 ulp, the restatement's to the C
library's 1 ulp: two terms differ by at most 7 ulp of their magnitude, 7 * 2^-52 |t_i| (an ulp is at most 2^-52 of the value; the
factor 2 is exact).  A far-field term is + - * / sqrt only: no difference.  Both sides then add the same n terms in the same order:
recursive summation of terms that differ by e_i differs by at most sum e_i + n 2^-53 sum |t_i| on either side, and the division by
4 pi adds one rounding of the quotient each.  So per query, from the restatement's own magnitudes:
    bar = (7 * 2^-52 * sum_exact |t_i| + 2 n 2^-53 sum |t_i|) / (4 pi) + 2^-52 |w|.
The brute route is held to the exact sum with n = the number of valid faces.  Where the brute route and the tree route at beta = inf
are compared with each other, the orders differ and each carries its own bar: their sum.

The bound of the table.  The device and the restatement perform the same IEEE operations in the same order (a parent is child 0 +
child 1), so the expected difference is zero; what is allowed is 4 ulp of the magnitude each entry accumulates -- sum |leaf term| below
the node for the sums, and for the derived entries the magnitudes of their operands:
    N0_j: 4u mag(N0_j);  p~_i: 4u (mag(S_i) / A + |p~_i|);  N1_ij: 4u (mag(M_ij) + |p~_i - o_i| mag(N0_j) + |p~_i| |N0_j|);
    r: 4u (r + max |p~|),   u = 2^-52.
The share of each bar that was used is printed."""
import numpy as np
import pytest
import torch

import closest_ref as CR
import raycast_ref as R
import winding_ref as W

pytestmark = pytest.mark.gpu

F32, D = np.float32, np.float64
CANARY = 64
U = 2.0 ** -52
ATAN2_REL = 7.0 * U
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mesh(v, f):
    return _cuda(np.asarray(v, F32)), _cuda(np.asarray(f, np.int32).reshape(-1, 3))


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * CANARY,), fill, dtype=dtype, device="cuda")
    return buf, buf[CANARY:CANARY + n]


def _check_canary(buf, w, what):
    fill = buf[0].item()
    assert bool((buf[:CANARY] == fill).all()) and bool((buf[CANARY + w.numel():] == fill).all()), f"canary of {what} overwritten"


def _dec(e):
    """the order-preserving image of an fp32 in the tree's header -> the fp32"""
    e = np.asarray(e, np.uint32)
    return np.where(e & np.uint32(0x80000000), e & np.uint32(0x7fffffff), ~e).astype(np.uint32).view(F32)


def _download(bvh):
    """the device's tree as the records winding_ref walks"""
    raw = bvh.buffer.cpu().numpy()
    F = bvh.faces.shape[0]
    nodes = raw[256:256 + 64 * F].view(np.int32).reshape(F, 16)[:max(F - 1, 0)]
    leaves = raw[256 + 64 * F:256 + 112 * F].view(np.int32).reshape(F, 12)
    bounds = raw[:32].view(np.uint32)
    with np.errstate(invalid="ignore"):
        o = (_dec(bounds[0:3]).astype(D) + _dec(bounds[4:7]).astype(D)) * 0.5
    return dict(child=nodes[:, 12:14].copy(), box=nodes[:, :12].copy().view(F32).reshape(-1, 2, 2, 3),
                leaf_v=leaves[:, :9].copy().view(F32).reshape(F, 3, 3), leaf_face=leaves[:, 9].copy(), o=o,
                flags=int(raw[32:36].view(np.int32)[0]))


def _moments_raw(bvh):
    """i2sdf_winding_moments into a guarded buffer -> (WindingMoments on the device, table (F - 1, 16) fp64 on the host)"""
    from i2sdf_amd import lib as L
    from i2sdf_amd import mesh as M
    lib = L.load()
    F = bvh.faces.shape[0]
    nbytes = int(lib.i2sdf_winding_moments_bytes(F))
    assert nbytes >= 128 * max(F - 1, 0) + 16 and nbytes % 16 == 0
    buf, w = _guarded(nbytes, torch.uint8, 0xA5)
    L.check(lib.i2sdf_winding_moments(L.ptr(bvh.buffer), F, L.ptr(w), L.stream_ptr()), "i2sdf_winding_moments")
    torch.cuda.synchronize()
    _check_canary(buf, w, "moments")
    mom = M.WindingMoments(w, F)
    return mom, mom.table.cpu().numpy().copy()


def _raw(route, v, f, q, beta=2.0, bvh=None, mom=None):
    """the C ABI with guarded outputs -> (w (n,) fp64, status); canaries checked"""
    from i2sdf_amd import lib as L
    lib = L.load()
    n = len(q)
    vt, ft = _mesh(v, f)
    qt = _cuda(np.asarray(q, F32).reshape(n, 3))
    wb, w = _guarded(n, torch.float64, -7.5)
    sb, s = _guarded(1, torch.int32, -77)
    if route == "bvh":
        L.check(lib.i2sdf_winding_bvh(L.ptr(bvh.buffer), L.ptr(mom.buffer), len(ft), L.ptr(qt), n, float(beta), L.ptr(w), L.ptr(s),
                                      L.stream_ptr()), "i2sdf_winding_bvh")
    else:
        L.check(lib.i2sdf_winding_brute(L.ptr(vt), len(v), L.ptr(ft), len(ft), L.ptr(qt), n, L.ptr(w), L.ptr(s), L.stream_ptr()),
                "i2sdf_winding_brute")
    torch.cuda.synchronize()
    _check_canary(wb, w, f"{route} w")
    _check_canary(sb, s, f"{route} status")
    return w.cpu().numpy().copy(), int(s.item())


def _bar(sum_exact, sum_all, n_terms, w):
    return (ATAN2_REL * sum_exact + 2.0 * n_terms * 2.0 ** -53 * sum_all) / W.FOUR_PI + U * np.abs(np.nan_to_num(w))


def _held(got, want, bar, what):
    """NaN rows agree; the others within their bar -> the largest share of the bar that was used"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok])
    assert (err <= bar[ok]).all(), (what, float(err.max()), float(bar[ok][err.argmax()]))
    return float((err / np.maximum(bar[ok], 1e-300)).max())


def _fixtures():
    iv, ifc = R.icosphere(2)
    sv, sf = R.soup(4)
    return {"ico2": (iv, ifc), "flipped": (iv, W.flipped(ifc)), "dup_shuffled": (iv, W.shuffled(W.duplicated(ifc), 3)), "cap": W.cap(3),
            "open_cube": W.open_cube(), "square": W.square(), "soup3000": R.soup(3000), "bad_faces": W.with_bad_faces(iv, ifc),
            "F0": (sv, np.zeros((0, 3), np.int32)), "F1": (sv, sf[:1]), "F2": (sv, sf[:2])}


NAMES = ["ico2", "flipped", "dup_shuffled", "cap", "open_cube", "square", "soup3000", "bad_faces", "F0", "F1", "F2"]


def _case(name, by):
    key = (name, by)
    if key not in _CACHE:
        v, f = _fixtures()[name]
        v = W.shift(v, by)
        q = W.queries(v, f, 150 if name == "soup3000" else 300, seed=71)
        _CACHE[key] = (v, f, q, W.exact(v, f, q))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("by", [0.0, 1000.0])
@pytest.mark.parametrize("name", NAMES)
def test_moments_table_against_the_restatement(name, by):
    from i2sdf_amd import mesh as M
    v, f, _, _ = _case(name, by)
    bvh = M.build_bvh(_mesh(v, f))
    before = bvh.buffer.clone()
    mom, got = _moments_raw(bvh)
    _, again = _moments_raw(bvh)
    assert torch.equal(bvh.buffer, before)                                     # the tree is only read
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), name      # two runs, the same bits
    tree = _download(bvh)
    want, raw, mag = W.moments(tree)
    assert got.shape == want.shape == (max(len(f) - 1, 0), 16)
    if not len(want):
        return
    with np.errstate(all="ignore"):
        area = raw[:, 0:1]
        p, s = want[:, 0:3], want[:, 0:3] - tree["o"][None]
        bound = np.zeros_like(want)
        bound[:, 0:3] = 4 * U * (mag[:, 1:4] / area + np.abs(p))
        bound[:, 3] = 4 * U * (want[:, 3] + np.abs(p).max(1))
        bound[:, 4:7] = 4 * U * mag[:, 4:7]
        bound[:, 7:] = 4 * U * (mag[:, 7:].reshape(-1, 3, 3) + np.abs(s)[:, :, None] * mag[:, None, 4:7]
                                + np.abs(p)[:, :, None] * np.abs(want[:, None, 4:7])).reshape(-1, 9)
    some = raw[:, 0] > 0
    assert np.array_equal(np.isinf(got[:, 3]), ~some) and np.array_equal(np.isinf(want[:, 3]), ~some), name      # no area: r = +inf
    err = np.abs(got[some] - want[some])
    assert (err <= bound[some]).all(), (name, float((err / np.maximum(bound[some], 1e-300)).max()))
    share = float((err / np.maximum(bound[some], 1e-300)).max()) if some.any() else 0.0
    print(f"{name}+{by:g}: {int(some.sum())} of {len(want)} records with area; largest share of the 4-ulp bound used: {share:.3f}; "
          f"bitwise equal: {np.array_equal(got[some].view(np.int64), want[some].view(np.int64))}")


# ------------------------------------------------------------------------------------------------ 2. routes and law
@pytest.mark.parametrize("by", [0.0, 1000.0])
@pytest.mark.parametrize("name", NAMES)
def test_brute_and_tree_routes_against_the_restatement(name, by):
    from i2sdf_amd import mesh as M
    v, f, q, (w_exact, sa, status) = _case(name, by)
    nv = int(R.valid_faces(v, f).sum()) if len(f) else 0
    got, st = _raw("brute", v, f, q)
    assert st == status, (name, st, status)
    shares = {"brute": _held(got, w_exact, _bar(sa, sa, nv, w_exact), f"{name}+{by:g} brute")}
    bvh = M.build_bvh(_mesh(v, f))
    mom, table = _moments_raw(bvh)
    tree = _download(bvh)
    for beta in (np.inf, 2.0, 3.0):
        h = W.hierarchical(tree, table, q, beta)
        got_t, st = _raw("bvh", v, f, q, beta, bvh, mom)
        assert st == status, (name, beta, st, status)
        shares[f"tree beta={beta:g}"] = _held(got_t, h["w"], _bar(h["sum_abs_exact"], h["sum_abs"], h["terms"], h["w"]), f"{name}+{by:g} beta={beta:g}")
        if beta == np.inf:
            assert (h["exact"][np.isfinite(q).all(1)] == nv).all()
            _held(got_t, got, _bar(sa, sa, nv, w_exact) + _bar(h["sum_abs_exact"], h["sum_abs"], h["terms"], h["w"]), f"{name}+{by:g} tree against brute")
        elif nv >= 300:
            assert h["terms"][np.isfinite(q).all(1)].mean() < 0.6 * nv, name     # the far field is taken at all
    print(f"{name}+{by:g}: largest share of the bar used: " + ", ".join(f"{k} {s:.3f}" for k, s in shares.items()))
    fin = np.isfinite(q).all(1)
    assert np.isnan(got[~fin]).all() and np.isfinite(got[fin]).all() and (~fin).sum() == 2
    assert abs(got[-1]) < 1e-6                                                  # the row at 1e6
    if name in ("ico2", "flipped", "dup_shuffled", "bad_faces"):               # closed: integers
        k = {"ico2": 1, "flipped": -1, "dup_shuffled": 2, "bad_faces": 1}[name]
        r = np.linalg.norm(q[fin].astype(D) - by, axis=1)
        assert np.abs(got[fin][r < 0.9] - k).max() < 1e-9 and np.abs(got[fin][r > 1.1]).max() < 1e-9


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 389, 2000])
def test_every_query_count(n):
    from i2sdf_amd import mesh as M
    if "counts" not in _CACHE:
        v, f = W.with_bad_faces(*R.icosphere(2))
        q = np.concatenate([W.queries(v, f, 997, seed=81)] * 2)
        bvh = M.build_bvh(_mesh(v, f))
        mom, table = _moments_raw(bvh)
        _CACHE["counts"] = (v, f, q, bvh, mom, W.exact(v, f, q), W.hierarchical(_download(bvh), table, q, 2.0))
    v, f, q, bvh, mom, (w_exact, sa, _), h = _CACHE["counts"]
    nv = int(R.valid_faces(v, f).sum())
    status = (W.BAD_POINT if n and not np.isfinite(q[:n]).all() else 0) | W.BAD_FACE            # n = 0 still reports the face bit
    got, st = _raw("brute", v, f, q[:n])
    assert st == status and got.shape == (n,)
    _held(got, w_exact[:n], _bar(sa, sa, nv, w_exact)[:n], f"n={n} brute")
    got, st = _raw("bvh", v, f, q[:n], 2.0, bvh, mom)
    assert st == status
    _held(got, h["w"][:n], _bar(h["sum_abs_exact"], h["sum_abs"], h["terms"], h["w"])[:n], f"n={n} tree")
    res = M.winding_number(bvh, _cuda(q[:n]), moments=mom)
    assert res.dtype == torch.float64 and res.shape == (n,)
    assert np.array_equal(res.cpu().numpy().view(np.int64), got.view(np.int64))


# ------------------------------------------------------------------------------------------------ 3. the surface, the front end
@pytest.mark.parametrize("name", ["ico2", "open_cube", "soup3000"])
def test_queries_on_the_surface(name):
    from i2sdf_amd import mesh as M
    v, f = _fixtures()[name]
    q = W.on_surface(v, f, 100)
    bvh = M.build_bvh(_mesh(v, f))
    mom, table = _moments_raw(bvh)
    a, _ = _raw("brute", v, f, q)
    b, _ = _raw("bvh", v, f, q, np.inf, bvh, mom)
    a2, _ = _raw("brute", v, f, q)
    b2, _ = _raw("bvh", v, f, q, np.inf, bvh, mom)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a.view(np.int64), a2.view(np.int64)) and np.array_equal(b.view(np.int64), b2.view(np.int64))
    # On the surface a term is atan2 of a det that is 0 up to rounding over a den that may be negative: the restatement's bar holds for
    # the same det and den, and both routes compute the same ones -- but the two ORDERS of summation are each held to their own bar.
    w_exact, sa, _ = W.exact(v, f, q)
    h = W.hierarchical(_download(bvh), table, q, np.inf)
    nv = len(f)
    bar = _bar(sa, sa, nv, w_exact) + _bar(h["sum_abs_exact"], h["sum_abs"], h["terms"], h["w"])
    share = float((np.abs(a - b) / bar).max())
    print(f"{name}: {len(q)} queries on vertices, edges and faces; brute against tree at beta = inf: largest share of the bar used {share:.3f}")
    assert (np.abs(a - b) <= bar).all(), share
    _held(a, w_exact, _bar(sa, sa, nv, w_exact), f"{name} surface brute")


def test_front_end_routes_and_errors():
    from i2sdf_amd import lib as L
    from i2sdf_amd import mesh as M
    import i2sdf_amd as A
    v, f, q, (w_exact, sa, _) = _case("ico2", 0.0)
    vt, ft = _mesh(v, f)
    qt = _cuda(q)
    bvh = A.build_bvh((vt, ft))
    mom = A.winding_moments(bvh)
    assert isinstance(mom, A.WindingMoments) and mom.table.shape == (len(f) - 1, 16) and mom.table.dtype == torch.float64
    a = A.winding_number(bvh, qt)                                              # the tree, its moments built here
    b = A.winding_number(bvh, qt, moments=mom)
    c = A.winding_number((vt, ft), qt, route="bvh")                            # a bare mesh gets its tree and table built
    d = A.winding_number(M.Mesh(vt, ft, vt), qt, route="brute")
    e = A.winding_number(bvh, qt, beta=float("inf"), moments=mom)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))
    assert M.WINDING_BRUTE_MAX_FACES == 1024
    assert torch.equal(A.winding_number((vt, ft), qt).view(torch.int64), d.view(torch.int64))       # 320 faces, bare: auto sums every face
    big_v, big_f = R.icosphere(3)
    big = _mesh(big_v, big_f)                                                   # 1280 faces, bare: auto takes the tree
    assert torch.equal(A.winding_number(big, qt).view(torch.int64), A.winding_number(big, qt, route="bvh").view(torch.int64))
    assert not torch.equal(A.winding_number(big, qt).view(torch.int64), A.winding_number(big, qt, route="brute").view(torch.int64))
    fin = np.isfinite(q).all(1)
    bar = 2 * _bar(sa, sa, len(f), w_exact)
    assert (np.abs(d.cpu().numpy() - e.cpu().numpy())[fin] <= bar[fin]).all()
    assert float((a - d).abs()[torch.from_numpy(fin).cuda()].max()) < 0.1      # beta = 2 against exact: the law's approximation
    small_v, small_f = W.open_cube()
    ins = A.inside(bvh, qt, moments=mom)
    r = np.linalg.norm(q.astype(D), axis=1)
    assert ins.dtype == torch.bool and bool(ins.cpu().numpy()[fin & (r < 0.9)].all()) and not ins.cpu().numpy()[~fin | (r > 1.1)].any()
    with pytest.raises(ValueError):
        A.winding_number(bvh, qt, beta=-1.0)
    with pytest.raises(ValueError):
        A.winding_number(bvh, qt, beta=float("nan"))
    with pytest.raises(ValueError):
        A.winding_number(bvh, qt, route="fast")
    with pytest.raises(ValueError):
        A.winding_number((vt, ft), qt, moments=mom)                            # moments belong to a tree
    with pytest.raises(ValueError):
        A.winding_number(A.build_bvh(_mesh(small_v, small_f)), qt, moments=mom)
    with pytest.raises(ValueError):
        A.signed_distance(bvh, qt, sign="parity")
    with pytest.raises(L.I2SDFError):
        A.winding_number((vt.cpu(), ft.cpu()), qt.cpu())
    lib = L.load()
    one = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.i2sdf_winding_moments_bytes(-1) == 0 and lib.i2sdf_winding_moments_bytes(L.BVH_MAX_FACES + 1) == 0
    assert lib.i2sdf_winding_moments(None, 4, L.ptr(one), None) != 0 and lib.i2sdf_winding_moments(L.ptr(bvh.buffer), 4, None, None) != 0
    assert lib.i2sdf_winding_bvh(L.ptr(bvh.buffer), L.ptr(mom.buffer), len(f), L.ptr(qt), 4, -1.0, L.ptr(one), L.ptr(one), None) != 0
    assert lib.i2sdf_winding_brute(L.ptr(vt), len(v), L.ptr(ft), len(f), L.ptr(qt), -1, L.ptr(one), L.ptr(one), None) != 0
    assert lib.i2sdf_winding_brute(L.ptr(vt), len(v), L.ptr(ft), len(f), L.ptr(qt), 4, L.ptr(one), None, None) != 0


# ------------------------------------------------------------------------------------------------ 4. inside, signed distance
def test_inside_and_signed_distance_on_the_cube_without_its_top():
    import i2sdf_amd as A
    v, f = W.open_cube()
    vt, ft = _mesh(v, f)
    g = np.random.default_rng(91)
    q = g.uniform(-0.3, 0.3, (400, 3)).astype(F32)                              # depth >= 0.2 below every wall, and below the missing top
    out = (g.uniform(0.8, 2.0, (200, 3)) * g.choice([-1.0, 1.0], (200, 3))).astype(F32)
    qt, ot = _cuda(q), _cuda(out)
    for mesh in ((vt, ft), A.build_bvh((vt, ft))):
        assert bool(A.inside(mesh, qt).all()) and not bool(A.inside(mesh, ot).any())
        sd = A.signed_distance(mesh, qt, sign="winding")
        assert sd.dtype == torch.float32 and bool((sd < 0).all())
        assert torch.equal(sd.abs(), A.closest_point(mesh, qt).dist)
        assert bool((A.signed_distance(mesh, ot, sign="winding") > 0).all())
        assert bool(torch.isinf(A.signed_distance(mesh, ot, sign="winding", max_dist=0.1)).all())
    # the default is what it was: the pseudonormal sign, the bits of closest_point with the tables -- and of the restatement fed them
    nm = A.pseudonormals((vt, ft))
    both = torch.cat([qt, ot])
    d0 = A.signed_distance((vt, ft), both)
    d1 = A.signed_distance((vt, ft), both, nm, float("inf"))
    d2 = A.closest_point((vt, ft), both, normals=nm).sdist
    assert torch.equal(d0.view(torch.int32), d2.view(torch.int32)) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    qq = both.cpu().numpy()
    law = CR.closest(v, f, qq)
    sign = CR.sign(v, f, qq.astype(D), law["face"], law["feature"].astype(np.int64), law["c"], (nm.vertex.cpu().numpy(), nm.edge.cpu().numpy()))
    assert np.array_equal((sign * law["dist"]).astype(F32).view(np.int32), d0.cpu().numpy().view(np.int32))


def test_level_set_of_the_network_agrees_with_its_sign():
    import i2sdf_amd as A
    torch.manual_seed(0)
    net = A.I2SDFNetwork(A.synthetic_conf()).cuda().eval()                      # 64 wide, geometric init: a sphere of radius about 0.6
    ax = A.uniform_axes(32, (-1.0, 1.0))
    mesh = net.extract_mesh(ax)
    cell = float(ax.spacing[0])
    assert mesh.faces.shape[0] > 500
    g = torch.Generator(device="cuda").manual_seed(7)
    q = (torch.rand(2000, 3, device="cuda", generator=g) * 1.8 - 0.9).contiguous()
    with torch.no_grad():
        sdf = net.sdf_grid(q).reshape(-1)
    far = sdf.abs() > 2 * cell
    neg = sdf < 0
    assert int((far & neg).sum()) > 100 and int((far & ~neg).sum()) > 100
    for beta in (2.0, 3.0, float("inf")):
        ins = A.inside(mesh, q, beta=beta)
        assert torch.equal(ins[far], neg[far]), (beta, int((ins[far] != neg[far]).sum()))
    sd = A.signed_distance(mesh, q, sign="winding")
    assert torch.equal((sd < 0)[far], neg[far])
