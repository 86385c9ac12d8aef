"""numpy restatement of the mesh-simplification law of include/i2sdf.h ("Mesh simplification"): the grid of voxel_down_sample, the face
quadric about the cell centre, the per-corner accumulation in the header's order (corners grouped by a stable sort, position j of a run
in lane j mod 64, lanes combined by the xor butterfly), the adjugate solve with its clamp, the face rules, and `clean` / `topology`.
Also the fixtures the tests share.  Every line is one rounded fp64 operation per value (numpy contracts nothing)."""
import numpy as np

import pointops_ref as P
import raycast_ref as R

F32, D = np.float32, np.float64
VOXEL_BITS = 21
MUTATIONS = ("once_per_cell", "merge_opposite", "largest_face_kept", "no_clamp", "round_for_floor")
TOPO_KEYS = ("edges", "boundary_edges", "manifold_edges", "nonmanifold_edges", "misoriented_edges", "repeated_index_faces",
             "referenced_vertices", "faces", "euler")


# ------------------------------------------------------------------------------------------------ fixtures
def cube(n=32):
    """the surface of [-1, 1]^3 with n x n quads a side, vertices shared along edges and corners, normals outward: 6 n^2 + 2 vertices"""
    k = np.arange(n + 1)
    x = (-1.0 + 2.0 * k / n)
    index, verts, faces = {}, [], []

    def vid(p):
        key = tuple(int(round((c + 1.0) * n / 2.0)) for c in p)
        if key not in index:
            index[key] = len(verts)
            verts.append(p)
        return index[key]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (-1.0, 1.0):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[w] = side, x[i + di], x[j + dj]
                        q.append(vid(tuple(p)))
                    if side < 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.array(verts, F32), np.array(faces, np.int32)


def cube_without_top(n=8):
    v, f = cube(n)
    keep = ~(v[f][:, :, 2] == 1.0).all(1)
    return v, np.ascontiguousarray(f[keep])


def folded_sheet(n=6):
    """a flat grid and the same faces again with the opposite orientation: opposite duplicates, both kept"""
    v, f = R.flat_grid(n)
    return v, np.concatenate([f, f[:, [0, 2, 1]]], 0)


def with_unreferenced(v, f, seed=3):
    g = np.random.default_rng(seed)
    extra = g.uniform(-1.2, 1.2, (37, 3)).astype(F32)
    return np.concatenate([extra[:20], v, extra[20:]], 0), (f + 20).astype(np.int32)


def duplicated_shuffled(f, seed=3):
    g = np.random.default_rng(seed)
    rot = np.stack([f[:, [1, 2, 0]], f[:, [2, 0, 1]]])[g.integers(0, 2, len(f)), np.arange(len(f))]      # the same cyclic sequence, rotated
    both = np.concatenate([f, rot], 0)
    return np.ascontiguousarray(both[g.permutation(len(both))]).astype(np.int32)


def shift(v, by):
    return (np.asarray(v, F32).astype(D) + by).astype(F32)


def vertex_normals(v):
    """some normals to carry along: the normalised positions about the centroid (zeros stay zeros)"""
    c = v.astype(D) - v.astype(D).mean(0) if len(v) else v.astype(D)
    n = np.linalg.norm(c, axis=1, keepdims=True)
    return np.where(n > 0, c / np.where(n > 0, n, 1.0), 0.0).astype(F32)


# ------------------------------------------------------------------------------------------------ the grid
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cells_of(verts, h, mutate=None):
    """-> (cell (V,) int64 in ascending key order, keys (M,) int64, lo (3,)); refuses what the status word refuses"""
    p = np.asarray(verts, F32).reshape(-1, 3).astype(D)
    if not np.isfinite(p).all():
        raise ValueError("non-finite coordinate")
    h = D(h)
    lo = p.min(0) - D(0.5) * h
    t = (p - lo) / h
    idx = (np.floor(t + 0.5) if mutate == "round_for_floor" else np.floor(t))
    if (idx >= float(1 << VOXEL_BITS)).any():
        raise ValueError("voxel index does not fit 21 bits")
    idx = idx.astype(np.int64)
    key = (idx[:, 0] << (2 * VOXEL_BITS)) | (idx[:, 1] << VOXEL_BITS) | idx[:, 2]
    keys, cell = np.unique(key, return_inverse=True)
    return cell.reshape(-1).astype(np.int64), keys, lo


def centres(keys, lo, h):
    mask = (1 << VOXEL_BITS) - 1
    idx = np.stack([(keys >> (2 * VOXEL_BITS)) & mask, (keys >> VOXEL_BITS) & mask, keys & mask], 1).astype(D)
    return lo[None] + (idx + D(0.5)) * D(h)


def _run_sums(cell, M, values):
    """sequential left-to-right fp64 sums of `values` (n, k) per cell, rows taken in ascending row index -> (sums (M, k), counts (M,))"""
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    start = np.searchsorted(sc, np.arange(M), "left")
    counts = np.searchsorted(sc, np.arange(M), "right") - start
    sums = np.zeros((M, values.shape[1]), D)
    sv = values[order]
    for r in range(int(counts.max()) if M else 0):
        has = counts > r
        sums[has] = sums[has] + sv[start[has] + r]
    return sums, counts


# ------------------------------------------------------------------------------------------------ quadrics
def face_quadric(a, b, c, cc):
    """(n, 9): n n^T as xx, xy, xz, yy, yz, zz and d n, about cc (n, 3) -- csrc/quadric.h's quadric_face"""
    e, g = b - a, c - a
    n0 = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
    n1 = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
    n2 = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
    r = a - cc
    d = -((n0 * r[:, 0] + n1 * r[:, 1]) + n2 * r[:, 2])
    return np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, d * n0, d * n1, d * n2], 1)


def cell_quadrics(verts, faces, cell, cc, mutate=None):
    """the header's sum: corners in a stable sort by cell, position j of a run in lane j mod 64 (ascending j within a lane, from +0),
    then the xor butterfly over the 64 lanes -> (M, 9)"""
    M = len(cc)
    V = len(verts)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(1)
    corner = np.arange(3 * len(f))
    cf, ck = corner // 3, corner % 3
    good = ok[cf]
    corner, cf, ck = corner[good], cf[good], ck[good]
    ccell = cell[f[cf, ck]]
    if mutate == "once_per_cell":                        # a face adds once per distinct cell, not once per corner
        first = np.ones(len(corner), bool)
        tri = cell[f[cf]]
        first &= ~((ck >= 1) & (tri[np.arange(len(cf)), ck] == tri[:, 0]))
        first &= ~((ck == 2) & (tri[:, 2] == tri[:, 1]))
        corner, cf, ck, ccell = corner[first], cf[first], ck[first], ccell[first]
    order = np.argsort(ccell, kind="stable")
    cf, ccell = cf[order], ccell[order]
    p = np.asarray(verts, F32).astype(D)
    q = face_quadric(p[f[cf, 0]], p[f[cf, 1]], p[f[cf, 2]], cc[ccell])
    start = np.searchsorted(ccell, np.arange(M), "left")
    j = np.arange(len(ccell)) - start[ccell]
    lane, rnd = j % 64, j // 64
    part = np.zeros((M, 64, 9), D)
    for r in range(int(rnd.max()) + 1 if len(rnd) else 0):
        s = rnd == r
        part[ccell[s], lane[s]] = part[ccell[s], lane[s]] + q[s]
    l = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        part = part + part[:, l ^ s]
    return part[:, 0]


def solve(q, reg, m, half, mutate=None):
    """csrc/quadric.h's quadric_solve, vectorised -> (x (M, 3), fallback (M,) bool)"""
    with np.errstate(all="ignore"):
        tr = (q[:, 0] + q[:, 3]) + q[:, 5]
        bad = ~(tr > 0.0) | ~(tr < np.inf)
        lam = D(reg) * tr
        m00, m01, m02, m11, m12, m22 = q[:, 0] + lam, q[:, 1], q[:, 2], q[:, 3] + lam, q[:, 4], q[:, 5] + lam
        r0, r1, r2 = lam * m[:, 0] - q[:, 6], lam * m[:, 1] - q[:, 7], lam * m[:, 2] - q[:, 8]
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
        left = ~(np.abs(x) <= D(half)).all(1)
        if mutate == "no_clamp":
            left = ~np.isfinite(x).all(1)
        fb = bad | left
    return np.where(fb[:, None], m, x), fb


# ------------------------------------------------------------------------------------------------ faces
def _canonical(t):
    """the lexicographically smallest rotation of every triple"""
    rots = np.stack([t, t[:, [1, 2, 0]], t[:, [2, 0, 1]]], 0)
    best = rots[0].copy()
    for r in rots[1:]:
        less = (r[:, 0] < best[:, 0]) | ((r[:, 0] == best[:, 0]) & ((r[:, 1] < best[:, 1]) | ((r[:, 1] == best[:, 1]) & (r[:, 2] < best[:, 2]))))
        best[less] = r[less]
    return best


def keep_faces(mapped, alive, duplicated=True, mutate=None):
    """of the `alive` faces, the first (smallest index) of every cyclic sequence -> keep (F,) bool"""
    keep = alive.copy()
    if not duplicated or not alive.any():
        return keep
    key = _canonical(mapped)
    if mutate == "merge_opposite":                       # duplicates merged whatever their orientation
        key = np.sort(mapped, 1)
    idx = np.nonzero(alive)[0]
    order = idx[np.lexsort((idx, key[idx, 2], key[idx, 1], key[idx, 0]))]
    k = key[order]
    head = np.concatenate([[True], (k[1:] != k[:-1]).any(1)])
    keep[:] = False
    if mutate == "largest_face_kept":
        tail = np.concatenate([head[1:], [True]])
        keep[order[tail]] = True
    else:
        keep[order[head]] = True
    return keep


def compact(table_v, table_n, mapped, keep):
    """kept faces in input order over the referenced rows of the table in ascending row order -> (verts, faces, normals, used, new_index)"""
    used = np.zeros(len(table_v), bool)
    used[mapped[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    faces = new[mapped[keep]].astype(np.int32).reshape(-1, 3)
    return table_v[used], faces, None if table_n is None else table_n[used], used, new


# ------------------------------------------------------------------------------------------------ the law
def simplify(verts, faces, h, contraction="quadric", reg=1e-3, normals=None, mutate=None, detail=False):
    """-> dict(verts, faces, normals, vertex_map, face_map, fallback) as the device returns them (detail: the cell table too)"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    if not (np.isfinite(h) and h > 0) or not (np.isfinite(reg) and reg > 0):
        raise ValueError("h and reg must be finite and positive")
    if ((f < 0) | (f >= V)).any():
        raise ValueError("face index outside [0, V)")
    if V == 0:
        return dict(verts=v, faces=f.astype(np.int32), normals=normals, vertex_map=np.zeros(0, np.int32), face_map=np.zeros(0, np.int32),
                    fallback=np.zeros(0, bool))
    cell, keys, lo = cells_of(v, h, mutate)
    M = len(keys)
    cc = centres(keys, lo, h)
    sums, counts = _run_sums(cell, M, v.astype(D))
    mean = sums / counts[:, None].astype(D)
    if contraction == "average":
        rep, fb, q = mean.astype(F32), np.zeros(M, bool), None
    else:
        q = cell_quadrics(v, f, cell, cc, mutate)
        x, fb = solve(q, reg, mean - cc, D(0.5) * D(h), mutate)
        rep = (cc + x).astype(F32)
    cn = None
    if normals is not None:
        s, _ = _run_sums(cell, M, np.asarray(normals, F32).astype(D))
        with np.errstate(all="ignore"):
            ln = np.sqrt(_dot(s, s))
            okn = (ln > 0) & (ln < np.inf)
            cn = np.where(okn[:, None], s / np.where(okn, ln, 1.0)[:, None], 0.0).astype(F32)
    mapped = cell[f] if len(f) else np.zeros((0, 3), np.int64)
    alive = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0])
    keep = keep_faces(mapped, alive, True, mutate)
    ov, of, on, used, new = compact(rep, cn, mapped, keep)
    out = dict(verts=ov, faces=of, normals=on, vertex_map=np.where(used[cell], new[cell], -1).astype(np.int32),
               face_map=np.nonzero(keep)[0].astype(np.int32), fallback=fb[used])
    if detail:
        out.update(cell=cell, centres=cc, quadrics=q, mean=mean, cell_fallback=fb, cell_verts=rep)
    return out


def position_key(v):
    b = np.ascontiguousarray(v, F32).view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    return b


def clean(verts, faces, normals=None, merge_vertices=True, degenerate=True, zero_area=True, duplicated=True):
    """-> dict(verts, faces, normals, vertex_map, face_map)"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    if ((f < 0) | (f >= V)).any():
        raise ValueError("face index outside [0, V)")
    vmap = np.arange(V)
    if merge_vertices and V:
        b = position_key(v)
        order = np.lexsort((np.arange(V), b[:, 2], b[:, 1], b[:, 0]))
        sb = b[order]
        head = np.concatenate([[True], (sb[1:] != sb[:-1]).any(1)])
        first = np.maximum.accumulate(np.where(head, np.arange(V), 0))
        vmap[order] = order[first]
    mapped = vmap[f] if len(f) else np.zeros((0, 3), np.int64)
    alive = np.ones(len(f), bool)
    if degenerate:
        alive &= (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0])
    if zero_area and len(f):
        p = v.astype(D)
        a, b_, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        e, g = b_ - a, c - a
        n = np.stack([e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1], e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2], e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]], 1)
        alive &= ~(n == 0.0).all(1)
    keep = keep_faces(mapped, alive, duplicated)
    ov, of, on, used, new = compact(v, None if normals is None else np.asarray(normals, F32), mapped, keep)
    return dict(verts=ov, faces=of, normals=on, vertex_map=np.where(used[vmap], new[vmap], -1).astype(np.int32),
                face_map=np.nonzero(keep)[0].astype(np.int32))


def topology(verts, faces):
    """-> the dict of MeshTopology.as_dict() (+ watertight, oriented)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    if ((f < 0) | (f >= V)).any():
        raise ValueError("face index outside [0, V)")
    rep = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    g = f[~rep]
    a = np.concatenate([g[:, 0], g[:, 1], g[:, 2]])
    b = np.concatenate([g[:, 1], g[:, 2], g[:, 0]])
    und = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
    direction = (a > b).astype(np.int64)
    out = dict.fromkeys(TOPO_KEYS, 0)
    out["repeated_index_faces"], out["faces"] = int(rep.sum()), int(len(g))
    out["referenced_vertices"] = int(len(np.unique(g)))
    if len(und):
        uniq, inv, cnt = np.unique(und, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        dsum = np.bincount(inv, weights=direction, minlength=len(uniq))
        out["edges"] = int(len(uniq))
        out["boundary_edges"] = int((cnt == 1).sum())
        out["manifold_edges"] = int((cnt == 2).sum())
        out["nonmanifold_edges"] = int((cnt >= 3).sum())
        out["misoriented_edges"] = int(((cnt == 2) & (dsum != 1)).sum())
    out["euler"] = out["referenced_vertices"] - out["edges"] + out["faces"]
    out["watertight"] = out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0
    out["oriented"] = out["misoriented_edges"] == 0
    return out


def plain_cell_mean(verts, h):
    """an independent fp64 cell mean (np.add.at, no pinned order) -> (means (M, 3) fp64 in ascending key order, cell (V,))"""
    cell, keys, _ = cells_of(verts, h)
    s = np.zeros((len(keys), 3), D)
    np.add.at(s, cell, np.asarray(verts, F32).astype(D))
    return s / np.bincount(cell, minlength=len(keys))[:, None], cell


def cube_surface_distance(p):
    """distance of points to the surface of [-1, 1]^3"""
    p = np.abs(np.asarray(p, D))
    outside = np.linalg.norm(np.maximum(p - 1.0, 0.0), axis=1)
    inside = 1.0 - p.max(1)
    return np.where((p <= 1.0).all(1), inside, outside)
