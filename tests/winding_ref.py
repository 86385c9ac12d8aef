"""numpy restatement of the winding-number law of include/i2sdf.h ("Winding number"): the Van Oosterom-Strackee term operation by
operation as csrc/tri_solid_angle.h writes it, the exact sum in ascending face order, the composable moments with their bottom-up
pass, and the hierarchical rule (orders 0 and 1 of Barill et al. 2018) on the tree of tests/raycast_ref.py -- or on any tree given as
records, such as one downloaded from the device.  Also the fixtures the tests share.  Vectorised over queries; faces and nodes are
looped over (the fixtures are small).  Every line is one rounded fp64 operation per value."""
import sys

import numpy as np

import raycast_ref as R

BAD_POINT, BAD_FACE = 1, 2
MUTATIONS = ("dropped_factor_2", "den_sign", "no_recentre", "order1_sign")
F32, D = np.float32, np.float64
FOUR_PI = D(4.0) * D(np.pi)


# ------------------------------------------------------------------------------------------------ fixtures
def flipped(faces):
    return np.ascontiguousarray(faces[:, [0, 2, 1]])


def duplicated(faces):
    return np.concatenate([faces, faces], 0)


def open_cube():
    """the cube [-0.5, 0.5]^3 without its top face (z = +0.5), normals outward: ten faces"""
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], F32)
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]      # bottom, y-, y+, x-, x+
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    return v, np.array(f, np.int32)


def square(a=0.5):
    """the square [-a, a]^2 in z = 0 made of two faces, normal -z: from above it is seen as the inside of a closed mesh sees its faces"""
    v = np.array([[-a, -a, 0], [a, -a, 0], [a, a, 0], [-a, a, 0]], F32)
    return v, np.array([[0, 2, 1], [0, 3, 2]], np.int32)


def cap(s=3, z_min=0.3):
    """the faces of icosphere(s) whose centroid lies above z_min: an open sheet"""
    v, f = R.icosphere(s)
    keep = v[f].astype(D).mean(1)[:, 2] > z_min
    return v, np.ascontiguousarray(f[keep])


def with_bad_faces(v, f):
    """faces with an index outside [0, V) and faces with a non-finite vertex mixed in: none of them contributes"""
    v2 = np.concatenate([v, np.array([[np.nan, 0, 0], [0, np.inf, 0]], F32)], 0)
    V = len(v)
    bad = np.array([[0, 1, V + 2], [-1, 2, 3], [V, 4, 5], [V + 1, 6, 7], [0, 1, 2 ** 31 - 1]], np.int32)
    out = np.concatenate([f[:7], bad[:2], f[7:40], bad[2:4], f[40:], bad[4:]], 0)
    return v2, np.ascontiguousarray(out)


def shuffled(f, seed=0):
    return np.ascontiguousarray(f[np.random.default_rng(seed).permutation(len(f))])


def shift(v, by):
    return (v.astype(D) + by).astype(F32)


# ------------------------------------------------------------------------------------------------ the per-face term
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def solid_angle_terms(q, A, B, C, mutate=None):
    """det, den of 2 atan2(det, den); q (n, 3), A, B, C (3,) or (n, 3), all widened to fp64"""
    q, A, B, C = (np.asarray(x, D) for x in (q, A, B, C))
    with np.errstate(all="ignore"):
        a, b, c = A - q, B - q, C - q
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        x0 = b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]
        x1 = b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]
        x2 = b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]
        det = (a[..., 0] * x0 + a[..., 1] * x1) + a[..., 2] * x2
        ab, bc, ca = _dot(a, b), _dot(b, c), _dot(c, a)
        if mutate == "den_sign":
            den = (((la * lb) * lc + ab * lc) - bc * la) + ca * lb
        else:
            den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb
    return det, den


def solid_angle(q, A, B, C, mutate=None):
    det, den = solid_angle_terms(q, A, B, C, mutate)
    t = np.arctan2(det, den)
    return t if mutate == "dropped_factor_2" else D(2.0) * t


def exact(verts, faces, q, mutate=None):
    """the brute-force law: (w, sum |Omega_f|, status); the sum runs in ascending face order"""
    q32 = np.asarray(q, F32).reshape(-1, 3)
    qd = q32.astype(D)
    ok = np.isfinite(q32).all(1)
    fv = R.valid_faces(verts, faces) if len(faces) else np.zeros(0, bool)
    s, sa = np.zeros(len(qd)), np.zeros(len(qd))
    P = verts.astype(D)
    safe = np.where(ok[:, None], qd, 0.0)
    for f in np.nonzero(fv)[0]:
        t = solid_angle(safe, P[faces[f, 0]], P[faces[f, 1]], P[faces[f, 2]], mutate)
        s = s + t
        sa = sa + np.abs(t)
    w = np.where(ok, s / FOUR_PI, np.nan)
    return w, sa, (BAD_POINT if (~ok).any() else 0) | (BAD_FACE if (~fv).any() else 0)


# ------------------------------------------------------------------------------------------------ the tree as records
def tree_of(verts, faces):
    """the tree raycast_ref builds, as the records the device holds: child (F - 1, 2) int32, box (F - 1, 2, 2, 3) fp32 [node][slot]
    [lo, hi][axis], leaf_v (F, 3, 3) fp32, leaf_face (F,) int32 (-1: no face), o (3,) fp64 the centre of the root box"""
    F = len(faces)
    fv = R.valid_faces(verts, faces) if F else np.zeros(0, bool)
    skeys = np.sort(R.morton_keys(verts, faces)) if F else np.zeros(0, np.int64)
    child = R.karras(skeys)
    box, _ = R.boxes(verts, faces, skeys, child)
    order = (skeys & 0xffffffff).astype(np.int64)
    leaf_face = np.where(fv[order], order, -1).astype(np.int32) if F else np.zeros(0, np.int32)
    leaf_v = np.full((F, 3, 3), np.nan, F32)
    for j in range(F):
        if leaf_face[j] >= 0:
            leaf_v[j] = verts[faces[leaf_face[j]]]
    if fv.any():
        P = verts[faces[fv]]
        o = (P.min((0, 1)).astype(D) + P.max((0, 1)).astype(D)) * D(0.5)
    else:
        o = np.full(3, np.nan)
    return dict(child=child, box=box, leaf_v=leaf_v, leaf_face=leaf_face, o=o)


# ------------------------------------------------------------------------------------------------ the moments
def face_moments(T, o):
    """the sixteen raw sums of one face T (3, 3) about o: area, area * centroid (3), area vector (3), (centroid - o) (x) area vector (9)"""
    A, B, C = T.astype(D)
    e, g = B - A, C - A
    n = np.array([(e[1] * g[2] - e[2] * g[1]) * 0.5, (e[2] * g[0] - e[0] * g[2]) * 0.5, (e[0] * g[1] - e[1] * g[0]) * 0.5])
    area = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    c = ((A + B) + C) / D(3.0)
    m = np.zeros(16)
    m[0] = area
    m[1:4] = area * c
    m[4:7] = n
    with np.errstate(invalid="ignore"):
        m[7:] = ((c - o)[:, None] * n[None, :]).ravel()
    return m


def finish(m, o, lo, hi, mutate=None):
    """raw sums -> the record: centroid (3), radius, N0 (3), N1 (9)"""
    t = np.zeros(16)
    with np.errstate(all="ignore"):
        p = m[1:4] / m[0]
        t[0:3] = p
        t[4:7] = m[4:7]
        below, above = p - lo.astype(D), hi.astype(D) - p
        e = np.where(below > above, below, above)
        s = p - o
        M = m[7:].reshape(3, 3)
        t[7:] = (M if mutate == "no_recentre" else M - s[:, None] * m[4:7][None, :]).ravel()
        t[3] = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) if m[0] > 0.0 else np.inf
    return t


def moments(tree, mutate=None):
    """(table (F - 1, 16) fp64, raw (F - 1, 16) fp64, mag (F - 1, 16): the sums of |leaf term| below every node, for error bounds)"""
    child, box, o = tree["child"], tree["box"], tree["o"]
    nn = len(child)
    raw, mag, table = np.zeros((nn, 16)), np.zeros((nn, 16)), np.zeros((nn, 16))

    def below(c):
        if c < 0:
            j = ~c
            m = face_moments(tree["leaf_v"][j], o) if tree["leaf_face"][j] >= 0 else np.zeros(16)
            return m, np.abs(m)
        (m0, a0), (m1, a1) = below(child[c, 0]), below(child[c, 1])
        raw[c], mag[c] = m0 + m1, a0 + a1
        return raw[c], mag[c]
    if nn:
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
        below(0)
    for i in range(nn):
        lo = R._mn(box[i, 0, 0], box[i, 1, 0])
        hi = R._mx(box[i, 0, 1], box[i, 1, 1])
        table[i] = finish(raw[i], o, lo, hi, mutate)
    return table, raw, mag


# ------------------------------------------------------------------------------------------------ the hierarchical rule
def far_field(q, t, beta2, mutate=None, order=1):
    """one record t (16,) against queries q (n, 3) -> accept (n,) bool, omega (n,)"""
    with np.errstate(all="ignore"):
        r = t[None, 0:3] - q
        d2 = _dot(r, r)
        accept = d2 > beta2 * (t[3] * t[3])
        d = np.sqrt(d2)
        d3 = d2 * d
        d5 = d3 * d2
        order0 = ((r[:, 0] * t[4] + r[:, 1] * t[5]) + r[:, 2] * t[6]) / d3
        trace = (t[7] + t[11]) + t[15]
        quad = np.zeros(len(q))
        for i in range(3):
            for j in range(3):
                quad = quad + (r[:, i] * r[:, j]) * t[7 + 3 * j + i]
        order1 = trace / d3 - (D(3.0) * quad) / d5
        if mutate == "order1_sign":
            order1 = -order1
        omega = order0 + order1 if order >= 1 else order0
    return accept, omega


def hierarchical(tree, table, q, beta, mutate=None, order=1):
    """the tree route -> dict(w, sum_abs = sum |t_i| over the terms a query added, sum_abs_exact = the same over its face terms, exact =
    how many of them were faces, terms = all)"""
    q32 = np.asarray(q, F32).reshape(-1, 3)
    qd = q32.astype(D)
    n = len(qd)
    ok = np.isfinite(q32).all(1)
    child, leaf_v, leaf_face = tree["child"], tree["leaf_v"], tree["leaf_face"]
    F = len(leaf_face)
    s, sa, sae = np.zeros(n), np.zeros(n), np.zeros(n)
    n_exact, n_terms = np.zeros(n, np.int64), np.zeros(n, np.int64)
    beta2 = D(beta) * D(beta)

    def visit(c, idx):
        nonlocal s, sa
        if len(idx) == 0:
            return
        if c < 0:
            j = ~c
            if leaf_face[j] >= 0:
                T = leaf_v[j].astype(D)
                t = solid_angle(qd[idx], T[0], T[1], T[2], mutate)
                s[idx] = s[idx] + t
                sa[idx] = sa[idx] + np.abs(t)
                sae[idx] = sae[idx] + np.abs(t)
                n_exact[idx] += 1
                n_terms[idx] += 1
            return
        accept, omega = far_field(qd[idx], table[c], beta2, mutate, order)
        far = idx[accept]
        s[far] = s[far] + omega[accept]
        sa[far] = sa[far] + np.abs(omega[accept])
        n_terms[far] += 1
        near = idx[~accept]
        visit(child[c, 0], near)
        visit(child[c, 1], near)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    if F == 1:
        visit(~0, np.nonzero(ok)[0])
    elif F > 1:
        visit(0, np.nonzero(ok)[0])
    return dict(w=np.where(ok, s / FOUR_PI, np.nan), sum_abs=sa, sum_abs_exact=sae, exact=n_exact, terms=n_terms)


# ------------------------------------------------------------------------------------------------ queries
def queries(verts, faces, n, seed=0):
    """n points (fp32) in the mesh's box grown by a quarter, then a NaN row, an inf row and a row at 1e6"""
    g = np.random.default_rng(seed)
    fv = R.valid_faces(verts, faces) if len(faces) else np.zeros(0, bool)
    if fv.any():
        P = verts[faces[fv]].astype(D)
        lo, hi = P.min((0, 1)), P.max((0, 1))
    else:
        lo, hi = -np.ones(3), np.ones(3)
    ext = np.maximum(hi - lo, 0.5)
    q = g.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (n, 3)).astype(F32)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e6, 1e6, -1e6]], F32)
    special[2] += ((lo + hi) / 2).astype(F32)
    return np.concatenate([q, special])


def surface_distance_at_least(verts, faces, q, dist):
    """(n,) bool: is q at least `dist` from every valid face (closest_ref's law, fp64)"""
    import closest_ref as CR
    return CR.closest(verts, faces, np.asarray(q, F32))["dist"].astype(D) >= dist


def on_surface(verts, faces, per=40, seed=0):
    """vertices, edge midpoints and face centroids of the first faces, rounded to fp32"""
    P = verts[faces[:per]].astype(D)
    return np.concatenate([P[:, 0], (P[:, 0] + P[:, 1]) / 2, (P[:, 1] + P[:, 2]) / 2, P.mean(1)]).astype(F32)
