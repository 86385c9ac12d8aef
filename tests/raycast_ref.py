"""numpy restatement of the ray-casting law of include/i2sdf.h ("Ray casting"): the watertight per-face rule (generic in dtype: fp32
replays csrc/tri_isect.h operation by operation, fp64 is the accuracy reference), the brute-force law with its tie rule, culling,
bounds and status bits, the Morton keys and Karras' topology with the bottom-up boxes.  Also the fixtures the tests share.
Vectorised over rays; the faces are looped over (the fixtures are small)."""
import numpy as np

BAD_RAY, BAD_FACE = 1, 2
MUTATIONS = ("largest_face_wins", "t_min_inclusive", "no_fp64", "det_zero_ok")


# ------------------------------------------------------------------------------------------------ fixtures
def icosphere(s):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1),
         (-p, 0, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(s):
        cache, g = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


def soup(n, seed=0):
    g = np.random.default_rng(seed)
    c = g.uniform(-1, 1, (n, 1, 3))
    v = (c + g.normal(0, 0.08, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def flat_grid(cells=16, z=0.5):
    k = np.arange(cells + 1)
    x = (-1.0 + 2.0 * k / cells).astype(np.float32)          # multiples of 1/8: exact
    v = np.stack([np.repeat(x, cells + 1), np.tile(x, cells + 1), np.full((cells + 1) ** 2, z, np.float32)], 1).astype(np.float32)
    idx = lambda i, j: i * (cells + 1) + j
    f = []
    for i in range(cells):
        for j in range(cells):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(f, dtype=np.int32)


def edges_of(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    return np.unique(np.sort(e, 1), axis=0)


def watertight_targets(verts, faces, interior_only=False):
    """every vertex and four points on every edge (fp64); interior_only drops what lies on an edge used by one face only"""
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    vmask = np.ones(len(verts), bool)
    if interior_only:
        rim = ue[cnt == 1]
        vmask[rim.ravel()] = False
        ue = ue[cnt == 2]
    v = verts.astype(np.float64)
    pts = [v[vmask]]
    for w in (0.2, 0.4, 0.6, 0.8):
        pts.append((1 - w) * v[ue[:, 0]] + w * v[ue[:, 1]])
    return np.concatenate(pts, 0)


# ------------------------------------------------------------------------------------------------ the rule
def ray_shear(o, d, dt):
    """per ray: kx, ky, kz, Sx, Sy, Sz, the permuted origin, ok"""
    o, d = np.asarray(o, dt), np.asarray(d, dt)
    n = len(o)
    a = np.abs(d)
    kz = np.zeros(n, np.int64)
    m = a[:, 0].copy()
    for k in (1, 2):
        g = a[:, k] > m
        kz[g], m[g] = k, a[g, k]
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    r = np.arange(n)
    dkz = d[r, kz]
    sw = dkz < 0
    kx, ky = np.where(sw, ky, kx), np.where(sw, kx, ky)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = d[r, kx] / dkz, d[r, ky] / dkz, dt(1) / dkz
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (m > 0) & np.isfinite(Sz)
    return dict(kx=kx, ky=ky, kz=kz, Sx=Sx.astype(dt), Sy=Sy.astype(dt), Sz=Sz.astype(dt), ox=o[r, kx], oy=o[r, ky], oz=o[r, kz], ok=ok, r=r)


def tri_hit(R, A, B, C, t_min, t_max, cull, dt, mutate=None):
    """one face (A, B, C: (3,) arrays; or (n, 3): a face per ray) against all rays -> accept (bool), t, u, v, det.
    Every line is one rounded operation per value."""
    with np.errstate(all="ignore"):
        P = {}
        for name, X in (("A", A), ("B", B), ("C", C)):
            X = np.asarray(X, dt)
            comp = (lambda k, X=X: X[k]) if X.ndim == 1 else (lambda k, X=X: X[R["r"], k])
            kzv = comp(R["kz"]) - R["oz"]
            sx = R["Sx"] * kzv
            sy = R["Sy"] * kzv
            P[name] = (kzv, (comp(R["kx"]) - R["ox"]) - sx, (comp(R["ky"]) - R["oy"]) - sy)
        (Akz, Ax, Ay), (Bkz, Bx, By), (Ckz, Cx, Cy) = P["A"], P["B"], P["C"]
        p1, p2 = Cx * By, Cy * Bx
        U = p1 - p2
        p1, p2 = Ax * Cy, Ay * Cx
        V = p1 - p2
        p1, p2 = Bx * Ay, By * Ax
        W = p1 - p2
        if mutate != "no_fp64" and dt is not np.float64:
            z = (U == 0) | (V == 0) | (W == 0)
            if z.any():
                D = np.float64
                U = np.where(z, (Cx.astype(D) * By.astype(D) - Cy.astype(D) * Bx.astype(D)).astype(dt), U)
                V = np.where(z, (Ax.astype(D) * Cy.astype(D) - Ay.astype(D) * Cx.astype(D)).astype(dt), V)
                W = np.where(z, (Bx.astype(D) * Ay.astype(D) - By.astype(D) * Ax.astype(D)).astype(dt), W)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        ok = ~mixed
        if mutate != "det_zero_ok":
            ok &= det != 0
        if cull == "back":
            ok &= ~(det < 0)
        Az, Bz, Cz = R["Sz"] * Akz, R["Sz"] * Bkz, R["Sz"] * Ckz
        q1, q2, q3 = U * Az, V * Bz, W * Cz
        T = (q1 + q2) + q3
        t = T / det
        lower = (t_min <= t) if mutate == "t_min_inclusive" else (t_min < t)
        ok &= lower & (t <= t_max)
        return ok, t, U / det, V / det, det


def valid_faces(verts, faces):
    V = len(verts)
    inr = ((faces >= 0) & (faces < V)).all(1)
    ok = inr.copy()
    ok[inr] &= np.isfinite(verts[faces[inr]]).all((1, 2))
    return ok


def trace(verts, faces, o, d, t_min=0.0, t_max=np.inf, cull="none", dt=np.float32, mutate=None):
    """the brute-force law -> dict(t, face, bary, hit, status)"""
    o, d = np.asarray(o, dt), np.asarray(d, dt)
    n = len(o)
    t_min = np.broadcast_to(np.asarray(t_min, dt), (n,)).astype(dt)
    t_max = np.broadcast_to(np.asarray(t_max, dt), (n,)).astype(dt)
    R = ray_shear(o, d, dt)
    ok_ray = R["ok"] & ~np.isnan(t_min) & ~np.isnan(t_max)
    fv = valid_faces(verts, faces)
    status = (BAD_RAY if (~ok_ray).any() else 0) | (BAD_FACE if (~fv).any() else 0)
    best_t, best_f = t_max.copy(), np.full(n, -1, np.int32)
    bu, bv = np.zeros(n, dt), np.zeros(n, dt)
    V = verts.astype(dt)
    for f in np.nonzero(fv)[0]:
        a, b, c = faces[f]
        ok, t, u, v, _ = tri_hit(R, V[a], V[b], V[c], t_min, best_t, cull, dt, mutate)
        ok &= ok_ray
        if mutate == "largest_face_wins":
            take = ok                                          # (faces come in ascending order: the last one with t <= best stays)
        else:
            take = ok & ((t < best_t) | (best_f < 0))          # (t <= best_t already; an equal t keeps the earlier, smaller face)
        best_t = np.where(take, t, best_t)
        best_f = np.where(take, f, best_f).astype(np.int32)
        bu, bv = np.where(take, u, bu), np.where(take, v, bv)
    return dict(t=best_t, face=best_f, bary=np.stack([bu, bv], 1), hit=best_f >= 0, status=status)


def all_hits(verts, faces, o, d, t_min, t_max, cull="none", dt=np.float64):
    """(n, F) t of every face that counts (nan elsewhere), and (n, F) the smallest normalised barycentric weight"""
    n, F = len(o), len(faces)
    R = ray_shear(np.asarray(o, dt), np.asarray(d, dt), dt)
    T, Mg = np.full((n, F), np.nan), np.full((n, F), np.nan)
    V = verts.astype(dt)
    fv = valid_faces(verts, faces)
    tmn = np.broadcast_to(np.asarray(t_min, dt), (n,))
    tmx = np.broadcast_to(np.asarray(t_max, dt), (n,))
    for f in np.nonzero(fv)[0]:
        a, b, c = faces[f]
        ok, t, u, v, _ = tri_hit(R, V[a], V[b], V[c], tmn, tmx, cull, dt)
        ok &= R["ok"]
        T[ok, f] = t[ok]
        Mg[ok, f] = np.minimum(np.minimum(u, v), 1 - u - v)[ok]
    return T, Mg


# ------------------------------------------------------------------------------------------------ keys, topology, boxes
def _spread10(x):
    x = x.astype(np.uint64) & 0x3ff
    x = (x | (x << 16)) & 0x030000ff
    x = (x | (x << 8)) & 0x0300f00f
    x = (x | (x << 4)) & 0x030c30c3
    x = (x | (x << 2)) & 0x09249249
    return x


def morton_keys(verts, faces):
    F = len(faces)
    fv = valid_faces(verts, faces)
    code = np.full(F, 1 << 30, np.uint64)
    if fv.any():
        P = verts[faces[fv]].astype(np.float64)                # (f, 3 vertices, 3 axes)
        lo, hi = P.min((0, 1)), P.max((0, 1))
        c = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0
        ext = hi - lo
        with np.errstate(all="ignore"):
            s = np.floor(((c - lo) / np.where(ext > 0, ext, 1.0)) * 1024.0)
        s = np.where(ext > 0, s, 0.0)
        q = np.clip(s, 0, 1023).astype(np.uint64)
        code[fv] = (_spread10(q[:, 0]) << np.uint64(2)) | (_spread10(q[:, 1]) << np.uint64(1)) | _spread10(q[:, 2])
    return ((code << np.uint64(32)) | np.arange(F, dtype=np.uint64)).astype(np.int64)


def _delta(k, i, j):
    if j < 0 or j >= len(k):
        return -1
    x = int(k[i]) ^ int(k[j])
    return 64 - x.bit_length()


def karras(skeys):
    """children (F - 1, 2) int32 of the internal nodes: >= 0 an internal node, < 0 the leaf ~child"""
    F = len(skeys)
    child = np.zeros((max(F - 1, 0), 2), np.int32)
    for i in range(F - 1):
        d = -1 if _delta(skeys, i, i + 1) - _delta(skeys, i, i - 1) < 0 else 1
        dmin = _delta(skeys, i, i - d)
        lmax = 2
        while _delta(skeys, i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if _delta(skeys, i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dn = _delta(skeys, i, j)
        s, t = 0, l
        while True:
            t = (t + 1) // 2
            if _delta(skeys, i, i + (s + t) * d) > dn:
                s += t
            if t <= 1:
                break
        g = i + s * d + min(d, 0)
        child[i, 0] = ~g if min(i, j) == g else g
        child[i, 1] = ~(g + 1) if max(i, j) == g + 1 else g + 1
    return child


def _mn(a, b):
    return np.where(b < a, b, a)


def _mx(a, b):
    return np.where(b > a, b, a)


def boxes(verts, faces, skeys, child):
    """(F - 1, 2, 2, 3) fp32: node, slot, lo / hi, axis -- and the leaf visit count of a walk from the root"""
    F = len(skeys)
    fv = valid_faces(verts, faces)
    order = (skeys & 0xffffffff).astype(np.int64)
    out = np.zeros((max(F - 1, 0), 2, 2, 3), np.float32)
    seen = np.zeros(F, np.int64)
    inf = np.float32(np.inf)

    def box(c):
        if c < 0:
            j = ~c
            seen[j] += 1
            f = order[j]
            if not fv[f]:
                return np.full(3, inf), np.full(3, -inf)
            A, B, C = verts[faces[f]]
            return _mn(_mn(A, B), C), _mx(_mx(A, B), C)
        (l0, h0), (l1, h1) = box(child[c, 0]), box(child[c, 1])
        out[c, 0, 0], out[c, 0, 1], out[c, 1, 0], out[c, 1, 1] = l0, h0, l1, h1
        return _mn(l0, l1), _mx(h0, h1)
    if F >= 2:
        import sys
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
        box(0)
    elif F == 1:
        seen[0] = 1
    return out, seen
