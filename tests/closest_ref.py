"""numpy restatement of the closest-point law of include/i2sdf.h ("Closest point"): the per-face rule (fp64, one IEEE operation per
line and value, replaying csrc/tri_closest.h), the law with its tie rule, max_dist, the faces that are never closest and the status
bits, the box bound of the tree route, the pseudonormal tables and the sign.  Also an independent formulation of the distance, and
the fixtures the tests share.  Vectorised over points; the faces are looped over (the fixtures are small)."""
import numpy as np

import raycast_ref as R

BAD_POINT, BAD_FACE = 1, 2
FACE, EDGE_AB, EDGE_BC, EDGE_CA, VERT_A, VERT_B, VERT_C = range(7)
MUTATIONS = ("largest_face_wins", "max_dist_exclusive", "face_normal_everywhere", "unclamped_plane", "degenerate_kept")
BOX_REL, BOX_ABS = 2.0 ** -20, 2.0 ** -32
D = np.float64


# ------------------------------------------------------------------------------------------------ fixtures
def subdivide(v, f, times):
    v = [np.asarray(x, D) for x in v]
    f = [tuple(t) for t in f]
    for _ in range(times):
        cache, g = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                v.append((v[a] + v[b]) / 2.0)
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v, D), np.array(f, np.int32)


WEDGE_Y = np.round(0.06 * 2 ** 24) / 2 ** 24        # 0.06 to 20 bits: every twice-subdivided coordinate is exact in fp32


def wedge_corners():
    return np.array([(0, 0, 0), (1, 0, 0), (0.5, WEDGE_Y, 1), (0.5, -WEDGE_Y, 1)], D)


def wedge_planes():
    """the four faces of the tetrahedron, oriented outward: (corner indices), and (normal, point) of their planes"""
    v = wedge_corners()
    cen = v.mean(0)
    tris, planes = [], []
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        n = np.cross(v[b] - v[a], v[c] - v[a])
        if n @ (v[a] - cen) < 0:
            b, c, n = c, b, -n
        tris.append((a, b, c))
        planes.append((n / np.linalg.norm(n), v[a]))
    return tris, planes


def wedge():
    """a sharp wedge: the tetrahedron (0,0,0), (1,0,0), (0.5, +-0.06, 1), outward, each face subdivided twice (64 faces)"""
    tris, _ = wedge_planes()
    v, f = subdivide(wedge_corners(), tris, 2)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(D), v)
    return v32, f


def wedge_inside(p):
    """the exact convex test (fp64) -> inside (bool), well_posed (no plane within 1e-9)"""
    _, planes = wedge_planes()
    s = np.stack([(np.asarray(p, D) - a) @ n for n, a in planes], 1)
    return (s < 0).all(1), (np.abs(s) > 1e-9).all(1)


def bumpy_sphere(s=2):
    """icosphere(s), radially perturbed: r = 1 + 0.6 sin 3 theta cos 2 phi -- closed, consistently oriented, star-shaped, not convex"""
    v, f = R.icosphere(s)
    v = v.astype(D)
    theta = np.arccos(np.clip(v[:, 2] / np.linalg.norm(v, axis=1), -1, 1))
    phi = np.arctan2(v[:, 1], v[:, 0])
    r = 1.0 + 0.6 * np.sin(3 * theta) * np.cos(2 * phi)
    return (v * r[:, None]).astype(np.float32), f


def duplicated(v, f, seed=5):
    """every face twice, shuffled: each closest face ties with its copy, and the smaller index must win"""
    g = np.random.default_rng(seed)
    ff = np.concatenate([f, f], 0)
    return v, ff[g.permutation(len(ff))].astype(np.int32)


def with_bad_faces(v, f, seed=6):
    """the mesh with never-closest faces mixed in: a bad index, a NaN vertex, zero-area faces (two equal vertices; three collinear)"""
    g = np.random.default_rng(seed)
    V = len(v)
    line = np.array([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]], np.float32)        # exactly collinear
    v2 = np.concatenate([v, [[np.nan, 0.0, 0.0]], line]).astype(np.float32)
    extra = np.array([[0, 1, V + 100], [0, -1, 2], [0, 1, V], [3, 3, 4], [5, 6, 5], [V + 1, V + 2, V + 3]], np.int32)
    ff = np.concatenate([f, extra], 0)
    return v2, ff[g.permutation(len(ff))].astype(np.int32)


# ------------------------------------------------------------------------------------------------ the rule
def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def tri_closest(p, A, B, C, mutate=None):
    """one face (A, B, C: (3,) or (n, 3) fp64) against the points p (n, 3) fp64 -> c (n, 3), d2, u, v (n), feature (n)"""
    with np.errstate(all="ignore"):
        p = np.asarray(p, D)
        n = len(p)
        A, B, C = (np.broadcast_to(np.asarray(X, D), (n, 3)) for X in (A, B, C))
        ab, ac, ap = B - A, C - A, p - A
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - B
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = p - C
        d5, d6 = dot(ab, cp), dot(ac, cp)
        p1, p2 = d1 * d4, d3 * d2
        vc = p1 - p2
        p1, p2 = d5 * d2, d1 * d6
        vb = p1 - p2
        p1, p2 = d3 * d6, d5 * d4
        va = p1 - p2
        e43, e56 = d4 - d3, d5 - d6
        one = np.ones(n)
        zero = np.zeros(n)
        s_ab = d1 / (d1 - d3)
        w_ca = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        den = 1.0 / ((va + vb) + vc)
        s_f, w_f = vb * den, vc * den
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        if mutate == "unclamped_plane":
            conds = [np.zeros(n, bool)] * 6
        feats = [VERT_A, VERT_B, EDGE_AB, VERT_C, EDGE_CA, EDGE_BC]
        cs = [A, B, A + s_ab[:, None] * ab, C, A + w_ca[:, None] * ac, B + w_bc[:, None] * (C - B)]
        us = [one, zero, 1.0 - s_ab, zero, 1.0 - w_ca, zero]
        vs = [zero, one, s_ab, zero, zero, 1.0 - w_bc]
        c = (A + s_f[:, None] * ab) + w_f[:, None] * ac
        u, v = (1.0 - s_f) - w_f, s_f
        feature = np.full(n, FACE)
        for cond, ft, cc, uu, vv in reversed(list(zip(conds, feats, cs, us, vs))):       # the first that applies decides
            c = np.where(cond[:, None], cc, c)
            u, v = np.where(cond, uu, u), np.where(cond, vv, v)
            feature = np.where(cond, ft, feature)
        r = p - c
        return c, dot(r, r), u, v, feature


def cross(ab, ac):
    return np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                     ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)


def countable_faces(verts, faces, mutate=None):
    """faces that may be closest: valid by the ray law, and ab x ac not exactly zero -> (countable, valid)"""
    valid = R.valid_faces(verts, faces)
    ok = valid.copy()
    if mutate != "degenerate_kept":
        P = verts[faces[valid]].astype(D)
        n = cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        ok[valid] &= ~(n == 0).all(1)
    return ok, valid


def closest(verts, faces, points, max_dist=np.inf, normals=None, mutate=None):
    """the brute-force law -> dict(dist, point, face, bary, feature, sdist, status, d2, c): the outputs as the device rounds them,
    and the unrounded d2 and c"""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3)
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(p32)
    p = p32.astype(D)
    ok_p = np.isfinite(p32).all(1)
    count, valid = countable_faces(verts, faces, mutate)
    status = (BAD_POINT if (~ok_p).any() else 0) | (BAD_FACE if (~valid).any() else 0)
    bound = D(np.float32(max_dist)) * D(np.float32(max_dist))
    best = np.full(n, bound)
    bf = np.full(n, -1, np.int32)
    bc, bu, bv, bft = np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    Vd = verts.astype(D)
    for f in np.nonzero(count)[0]:
        a, b, c = faces[f]
        cc, d2, u, v, ft = tri_closest(np.where(ok_p[:, None], p, 0.0), Vd[a], Vd[b], Vd[c], mutate)
        inside = (d2 < bound) if mutate == "max_dist_exclusive" else (d2 <= bound)
        if mutate == "largest_face_wins":
            take = inside & ((bf < 0) | (d2 <= best))
        else:
            take = inside & ((bf < 0) | (d2 < best))           # (faces come in ascending order: an equal d2 keeps the smaller index)
        take &= ok_p
        best = np.where(take, d2, best)
        bf = np.where(take, f, bf).astype(np.int32)
        bc = np.where(take[:, None], cc, bc)
        bu, bv, bft = np.where(take, u, bu), np.where(take, v, bv), np.where(take, ft, bft)
    hit = bf >= 0
    with np.errstate(all="ignore"):
        dist = np.where(hit, np.sqrt(best).astype(np.float32), np.float32(np.inf)).astype(np.float32)
    out = dict(dist=dist, point=np.where(hit[:, None], bc, 0.0).astype(np.float32), face=bf,
               bary=np.where(hit[:, None], np.stack([bu, bv], 1), 0.0).astype(np.float32), feature=np.where(hit, bft, 0).astype(np.uint8),
               sdist=None, status=status, d2=best, c=bc)
    if normals is not None:
        out["sdist"] = (sign(verts, faces, p, bf, bft, bc, normals, mutate) * dist).astype(np.float32)
    return out


def sign(verts, faces, p, face, feature, c, normals, mutate=None):
    """+1 / -1 per point (+1 on a miss: +inf stays +inf)"""
    vn, en = np.asarray(normals[0], np.float32).astype(D), np.asarray(normals[1], np.float32).astype(D)
    n = len(p)
    s = np.ones(n)
    hit = np.nonzero(face >= 0)[0]
    if len(hit) == 0:
        return s
    f, ft = face[hit], feature[hit]
    idx = faces[f]
    P = verts[idx].astype(D)
    N = cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    if mutate != "face_normal_everywhere":
        e = (ft >= EDGE_AB) & (ft <= EDGE_CA)
        N[e] = en[f[e], ft[e] - EDGE_AB]
        k = ft >= VERT_A
        N[k] = vn[idx[k, ft[k] - VERT_A]]
    with np.errstate(all="ignore"):
        s[hit] = np.where(dot(p[hit] - c[hit], N) >= 0, 1.0, -1.0)
    return s


# ------------------------------------------------------------------------------------------------ the tables
def pseudonormals(verts, faces, as_f64=False):
    """vnormal (V, 3), enormal (F, 3, 3): fp64 sums in ascending face index, rounded to fp32 once"""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(verts), len(faces)
    count, _ = countable_faces(verts, faces)
    vn = np.zeros((V, 3))
    esum = {}
    for f in np.nonzero(count)[0]:
        idx = faces[f]
        P = verts[idx].astype(D)
        x = cross(P[1] - P[0], P[2] - P[0])
        nf = x / np.sqrt(dot(x, x))
        for k in range(3):
            e1, e2 = P[(k + 1) % 3] - P[k], P[(k + 2) % 3] - P[k]
            y = cross(e1, e2)
            ang = np.arctan2(np.sqrt(dot(y, y)), dot(e1, e2))
            vn[idx[k]] = vn[idx[k]] + ang * nf
            key = (min(idx[k], idx[(k + 1) % 3]), max(idx[k], idx[(k + 1) % 3]))
            esum[key] = esum.get(key, np.zeros(3)) + 1.0 * nf
    en = np.zeros((F, 3, 3))
    for f in np.nonzero(count)[0]:
        idx = faces[f]
        for k in range(3):
            en[f, k] = esum[(min(idx[k], idx[(k + 1) % 3]), max(idx[k], idx[(k + 1) % 3]))]
    if as_f64:
        return vn, en
    return vn.astype(np.float32), en.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the box bound of the tree route
def box_dist2(p, lo, hi):
    p, lo, hi = np.asarray(p, D), np.asarray(lo, np.float32).astype(D), np.asarray(hi, np.float32).astype(D)
    e = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def box_skip_above(bound, M):
    r = np.sqrt(bound) * (1.0 + BOX_REL) + BOX_ABS * M
    return r * r


# ------------------------------------------------------------------------------------------------ an independent formulation
def independent_d2(verts, faces, points):
    """(n, F) squared distances, not by regions: the minimum over the plane projection (when it lies inside the triangle), the three
    clamped segments and the three vertices.  nan for faces that may not be closest."""
    p = np.asarray(points, np.float32).astype(D)
    count, _ = countable_faces(verts, faces)
    out = np.full((len(p), len(faces)), np.nan)
    for f in np.nonzero(count)[0]:
        A, B, C = verts[faces[f]].astype(D)
        best = np.full(len(p), np.inf)
        for X in (A, B, C):
            best = np.minimum(best, ((p - X) ** 2).sum(1))
        for X, Y in ((A, B), (B, C), (C, A)):
            e = Y - X
            t = np.clip(((p - X) @ e) / (e @ e), 0.0, 1.0)
            best = np.minimum(best, ((p - (X + t[:, None] * e)) ** 2).sum(1))
        nrm = np.cross(B - A, C - A)
        nn = nrm @ nrm
        h = ((p - A) @ nrm) / nn
        q = p - h[:, None] * nrm
        inside = np.ones(len(p), bool)
        for X, Y in ((A, B), (B, C), (C, A)):
            inside &= np.cross(Y - X, q - X) @ nrm >= 0
        best = np.where(inside, np.minimum(best, h * h * nn), best)
        out[:, f] = best
    return out


# ------------------------------------------------------------------------------------------------ queries and signs for the tests
def queries(verts, faces, n_random=300, seed=0, special=True):
    """fp32 queries: random in twice the bounding box; and (special) exactly on vertices, on fp32-rounded edge midpoints and face
    centroids, on the planes of the root box, at 1e6 from the mesh, and NaN / inf rows"""
    g = np.random.default_rng(seed)
    ok = R.valid_faces(verts, faces)
    P = verts[faces[ok]].astype(D) if ok.any() else np.zeros((1, 3, 3))
    lo, hi = P.min((0, 1)), P.max((0, 1))
    cen, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.05)
    out = [cen + g.uniform(-2, 2, (n_random, 3)) * half]
    if special:
        k = g.permutation(len(P))[:40]
        out += [P[k, 0], (P[k, 0] + P[k, 1]) / 2, (P[k, 1] + P[k, 2]) / 2, P[k].mean(1)]
        onbox = cen + g.uniform(-1.5, 1.5, (36, 3)) * half
        for i in range(36):
            onbox[i, i % 3] = (lo, hi)[(i // 3) % 2][i % 3]
        out += [onbox, cen + 1e6 * np.array([[1, 0, 0], [0, -1, 0], [0.6, 0.0, 0.8], [-1, -1, -1]])]
        out += [np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])]
    with np.errstate(all="ignore"):
        return np.concatenate(out, 0).astype(np.float32)


def parity_inside(verts, faces, p, seed=0):
    """inside by crossing parity of one random ray per point (raycast_ref.all_hits, fp64) -> inside, well_posed (every crossing's
    smallest barycentric weight above 1e-6)"""
    g = np.random.default_rng(seed)
    d = g.normal(size=(len(p), 3))
    T, Mg = R.all_hits(verts, faces, np.asarray(p, D), d, 0.0, np.inf)
    hits = ~np.isnan(T)
    well = np.where(hits, Mg, 1.0).min(1) > 1e-6
    return hits.sum(1) % 2 == 1, well


def limit(res, max_dist):
    """the law's result under `max_dist` from its result without one: the smallest d2 of all counts iff it is <= max_dist^2
    (tests/test_closest_ref.py holds this against a direct run)"""
    bound = D(np.float32(max_dist)) * D(np.float32(max_dist))
    keep = (res["face"] >= 0) & (res["d2"] <= bound)
    out = dict(res)
    out["dist"] = np.where(keep, res["dist"], np.float32(np.inf)).astype(np.float32)
    out["face"] = np.where(keep, res["face"], -1).astype(np.int32)
    for k in ("point", "bary"):
        out[k] = np.where(keep[:, None], res[k], 0).astype(np.float32)
    out["feature"] = np.where(keep, res["feature"], 0).astype(np.uint8)
    if res.get("sdist") is not None:
        out["sdist"] = np.where(keep, res["sdist"], np.float32(np.inf)).astype(np.float32)
    return out
