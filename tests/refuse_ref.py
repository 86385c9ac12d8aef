"""Numpy restatement of the visibility culling (csrc/raster.hip, csrc/tsdf.hip): mesh depth by fp64 ray-triangle edge functions with
a top-left rule, and rules 1-5 of the TSDF fusion / extraction, vectorised per unit.  The arithmetic follows the order written at the
head of the two kernel files (numpy rounds every fp32 / fp64 operation on its own, as the kernels do with contraction off), so that
coverage, touched units and weights can be compared as integers.  Also the small scene builders the CPU and GPU tests share.
Neither open3d nor pyrender is available: the tests that use this file check it against closed-form geometry first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcubes_ref as M  # noqa: E402

F32, F64 = np.float32, np.float64
SMALL_MAX = 64                                  # I2SDF_RASTER_SMALL_MAX: pixel boxes above it go to the workgroup-per-triangle kernel


def k4_of(K):
    K = np.asarray(K, F64)
    return tuple(F32(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def transform(m, x):
    """((m0 x + m1 y) + m2 z) + m3 per row of the 3 x 4 matrix m, in the dtype of the inputs."""
    return np.stack([((m[k, 0] * x[:, 0] + m[k, 1] * x[:, 1]) + m[k, 2] * x[:, 2]) + m[k, 3] for k in range(3)], 1)


# ----------------------------------------------------------------------------------------------------------- mesh depth
def _cross(p, q):
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def tri_setup(vc, faces, k4, H, W, znear, cull):
    """Per triangle of one camera: valid, the three edge normals (F, 3, 3) and det in fp64 (oriented so that det > 0), and the fp32
    pixel box (x0, x1, y0, y1) of the kernel."""
    fx, fy, cx, cy = k4
    znear = F32(znear)
    p = vc[faces]                                                        # (F, 3, 3) fp32
    inn = p[:, :, 2] >= znear
    a, b, c = (p[:, i].astype(F64) for i in range(3))
    n = np.stack([_cross(b, c), _cross(c, a), _cross(a, b)], 1)
    det = (a[:, 0] * n[:, 0, 0] + a[:, 1] * n[:, 0, 1]) + a[:, 2] * n[:, 0, 2]
    valid = inn.any(1) & ((det < 0) | (det > 0))
    if cull:
        valid &= ~(det > 0)
    flip = det < 0
    n[flip] = -n[flip]
    det = np.where(flip, -det, det)
    lo = np.full((p.shape[0], 2), np.inf, F32)
    hi = np.full((p.shape[0], 2), -np.inf, F32)

    def add(x, y, z, m):
        with np.errstate(all="ignore"):
            px, py = (x * fx) / z + cx, (y * fy) / z + cy
        for k, q in ((0, px), (1, py)):
            lo[m, k] = np.fmin(lo[m, k], q[m])
            hi[m, k] = np.fmax(hi[m, k], q[m])

    for e in range(3):
        f = (e + 1) % 3
        add(p[:, e, 0], p[:, e, 1], p[:, e, 2], inn[:, e])
        m = inn[:, e] != inn[:, f]
        with np.errstate(all="ignore"):
            s = (znear - p[:, e, 2]) / (p[:, f, 2] - p[:, e, 2])
            add(p[:, e, 0] + s * (p[:, f, 0] - p[:, e, 0]), p[:, e, 1] + s * (p[:, f, 1] - p[:, e, 1]), np.full(p.shape[0], znear, F32), m)
    with np.errstate(all="ignore"):
        x0 = np.fmax(np.floor(lo[:, 0]) - F32(1), F32(0))
        x1 = np.fmin(np.ceil(hi[:, 0]) + F32(1), F32(W - 1))
        y0 = np.fmax(np.floor(lo[:, 1]) - F32(1), F32(0))
        y1 = np.fmin(np.ceil(hi[:, 1]) + F32(1), F32(H - 1))
    valid &= (x1 >= x0) & (y1 >= y0)
    box = np.stack([x0, x1, y0, y1], 1)
    box = np.where(valid[:, None], box, 0).astype(np.int64)
    return valid, n, det, box


def mesh_depth(verts, faces, w2c, K, H, W, znear=0.05, zfar=100.0, cull="back", margin=2, edge_eps=1e-6):
    """-> dict(depth (n_cam, H, W) fp32, near_edge (n_cam, H, W) bool: a sample within edge_eps pixels of an edge of a triangle that
    (nearly) covers it, n_large / n_small (n_cam,): triangles per path by the kernel's box rule, hits (n_cam, H, W) int: how many
    triangles cover each sample).  The samples tried for a triangle are those of its box widened by `margin` more pixels, so a box
    that is too tight shows as a difference."""
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int64)
    w2c = np.asarray(w2c, F32)
    k4 = k4_of(K)
    fx, fy, cx, cy = (F64(v) for v in k4)
    n_cam = w2c.shape[0]
    depth = np.zeros((n_cam, H, W), F32)
    near_edge = np.zeros((n_cam, H, W), bool)
    hits = np.zeros((n_cam, H, W), np.int64)
    n_large, n_small = np.zeros(n_cam, np.int64), np.zeros(n_cam, np.int64)
    for c in range(n_cam):
        if verts.shape[0] == 0 or faces.shape[0] == 0:
            continue
        vc = transform(w2c[c], verts)
        valid, n, det, box = tri_setup(vc, faces, k4, H, W, znear, cull == "back")
        area = (box[:, 1] - box[:, 0] + 1) * (box[:, 3] - box[:, 2] + 1)
        n_large[c] = int((valid & (area > SMALL_MAX)).sum())
        n_small[c] = int((valid & (area <= SMALL_MAX)).sum())
        t = np.nonzero(valid)[0]
        if t.size == 0:
            continue
        x0, x1 = np.maximum(box[t, 0] - margin, 0), np.minimum(box[t, 1] + margin, W - 1)
        y0, y1 = np.maximum(box[t, 2] - margin, 0), np.minimum(box[t, 3] + margin, H - 1)
        bw, cnt = x1 - x0 + 1, (x1 - x0 + 1) * (y1 - y0 + 1)
        zbuf = np.full(H * W, np.inf, F32)
        ne, hc = near_edge[c].reshape(-1), hits[c].reshape(-1)
        for s in range(0, t.size, 4096):                                 # (chunks of triangles keep the pair arrays small)
            sl = slice(s, s + 4096)
            tri = np.repeat(np.arange(t[sl].size), cnt[sl])
            q = np.arange(tri.size) - np.repeat(np.cumsum(cnt[sl]) - cnt[sl], cnt[sl])
            u, v = x0[sl][tri] + q % bw[sl][tri], y0[sl][tri] + q // bw[sl][tri]
            nn, dd = n[t[sl]][tri], det[t[sl]][tri]
            dx, dy = (u.astype(F64) - cx) / fx, (v.astype(F64) - cy) / fy
            e = (nn[:, :, 0] * dx[:, None] + nn[:, :, 1] * dy[:, None]) + nn[:, :, 2]
            cov = (e > 0) | ((e == 0) & ((nn[:, :, 0] > 0) | ((nn[:, :, 0] == 0) & (nn[:, :, 1] > 0))))
            ssum = (e[:, 0] + e[:, 1]) + e[:, 2]
            with np.errstate(all="ignore"):
                z = (dd / ssum).astype(F32)
                ok = cov.all(1) & (ssum > 0) & (z >= F32(znear)) & (z <= F32(zfar))
                # distance of the sample to each edge line in pixels, signed (positive inside)
                dist = e / np.sqrt((nn[:, :, 0] / fx) ** 2 + (nn[:, :, 1] / fy) ** 2)
            near = (np.abs(dist).min(1) < edge_eps) & (dist > -edge_eps).all(1)
            pix = v * W + u
            np.minimum.at(zbuf, pix[ok], z[ok])
            np.add.at(hc, pix[ok], 1)
            ne[pix[near]] = True
        depth[c] = np.where(np.isfinite(zbuf), zbuf, F32(0)).reshape(H, W)
    return dict(depth=depth, near_edge=near_edge, hits=hits, n_large=n_large, n_small=n_small)


# ---------------------------------------------------------------------------------------------------------- TSDF fusion
def _measurement(d, dtrunc):
    with np.errstate(invalid="ignore"):
        return np.where((d > 0) & (d < F32(dtrunc)), d, F32(0)).astype(F32)


def touched_units(depth, c2w, k4, ul, trunc, dtrunc, stride):
    """(n, 3) int64 unit indices camera touches (rule 3), unique, lexicographic."""
    fx, fy, cx, cy = k4
    H, W = depth.shape
    v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    d = _measurement(depth[v, u], dtrunc)
    m = d > 0
    u, v, d = u[m], v[m], d[m]
    if d.size == 0:
        return np.zeros((0, 3), np.int64)
    xc, yc = ((u.astype(F32) - cx) * d) / fx, ((v.astype(F32) - cy) * d) / fy
    p = transform(c2w, np.stack([xc, yc, d], 1))
    lo = np.floor((p - F32(trunc)) / F32(ul)).astype(np.int64)
    hi = np.floor((p + F32(trunc)) / F32(ul)).astype(np.int64)
    out = []
    r = (hi - lo).max(0)
    for ox in range(r[0] + 1):
        for oy in range(r[1] + 1):
            for oz in range(r[2] + 1):
                q = lo + np.array([ox, oy, oz])
                out.append(q[(q <= hi).all(1)])
    return np.unique(np.concatenate(out), axis=0)


LIN = np.arange(4096)
IJK = np.stack([LIN >> 8, (LIN >> 4) & 15, LIN & 15], 1)


def voxel_centres(units, vl, ul):
    """(n_units, 4096, 3) fp32 centres, voxel (i, j, k) at i << 8 | j << 4 | k."""
    return units.astype(F32)[:, None, :] * F32(ul) + (IJK.astype(F32)[None] + F32(0.5)) * F32(vl)


def tsdf_integrate(depths, c2w, w2c, K, voxel_length=0.01, sdf_trunc=None, depth_trunc=5.0, stride=4):
    """Rules 1-4 -> dict(units (n, 3) lexicographic, weight (n, 4096) int, tsdf32: every operation in fp32 as the kernel does them,
    tsdf64: the same fp32 coordinates, pixel and sdf, but t and the running average in fp64, tmax: the largest |t| that entered a voxel,
    borderline (n, 4096) bool: in fp64 the voxel's projection lies within 1e-4 px of a pixel boundary, or its sdf within 1e-5 sdf_trunc
    of -sdf_trunc, for some camera that touched its unit; per_camera: the touched unit sets)."""
    depths, c2w, w2c = np.asarray(depths, F32), np.asarray(c2w, F32), np.asarray(w2c, F32)
    k4 = k4_of(K)
    fx, fy, cx, cy = k4
    vl = F32(voxel_length)
    trunc = F32(3.0 * voxel_length if sdf_trunc is None else sdf_trunc)
    ul = F32(F32(16.0) * vl)
    n_cam, H, W = depths.shape
    per_cam = [touched_units(depths[c], c2w[c], k4, ul, trunc, depth_trunc, stride) for c in range(n_cam)]
    units = np.unique(np.concatenate(per_cam + [np.zeros((0, 3), np.int64)]), axis=0)
    n = units.shape[0]
    key = lambda a: (a[:, 0] * (1 << 42)) + (a[:, 1] * (1 << 21)) + a[:, 2] if a.size else np.zeros(0, np.int64)
    ukeys = key(units - units.min(0)) if n else np.zeros(0, np.int64)
    tsdf32, tsdf64 = np.zeros((n, 4096), F32), np.zeros((n, 4096), F64)
    weight = np.zeros((n, 4096), np.int64)
    tmax = np.zeros((n, 4096), F64)
    borderline = np.zeros((n, 4096), bool)
    for c in range(n_cam):
        if per_cam[c].shape[0] == 0:
            continue
        rows = np.searchsorted(ukeys, key(per_cam[c] - units.min(0)))
        x = voxel_centres(units[rows], vl, ul).reshape(-1, 3)
        q = transform(w2c[c], x)
        with np.errstate(all="ignore"):
            fu = (((q[:, 0] * fx) / q[:, 2]) + cx) + F32(0.5)
            fv = (((q[:, 1] * fy) / q[:, 2]) + cy) + F32(0.5)
            inside = (q[:, 2] > 0) & (fu > -1) & (fu < F32(W)) & (fv > -1) & (fv < F32(H))
        idx = np.nonzero(inside)[0]
        u, v = fu[idx].astype(np.int64), fv[idx].astype(np.int64)        # (astype truncates towards zero, like the C cast)
        d = _measurement(depths[c][v, u], depth_trunc)
        ax, ay = (u.astype(F32) - cx) / fx, (v.astype(F32) - cy) / fy
        m = np.sqrt((ax * ax + ay * ay) + F32(1))
        sdf = (d - q[idx, 2]) * m
        upd = (d > 0) & (sdf > -trunc)
        # borderline voxels, judged in fp64 from the same fp32 centres
        x64 = x[idx].astype(F64)
        q64 = transform(w2c[c].astype(F64), x64)
        fu64 = q64[:, 0] * F64(fx) / q64[:, 2] + F64(cx) + 0.5
        fv64 = q64[:, 1] * F64(fy) / q64[:, 2] + F64(cy) + 0.5
        m64 = np.sqrt(((u - F64(cx)) / F64(fx)) ** 2 + ((v - F64(cy)) / F64(fy)) ** 2 + 1.0)
        sdf64 = (d.astype(F64) - q64[:, 2]) * m64
        bl = (np.abs(fu64 - np.round(fu64)) < 1e-4) | (np.abs(fv64 - np.round(fv64)) < 1e-4) | \
             ((d > 0) & (np.abs(sdf64 + F64(trunc)) < 1e-5 * F64(trunc)))
        r, l = rows[idx // 4096], idx % 4096
        borderline[r[bl], l[bl]] = True
        r, l, sdf = r[upd], l[upd], sdf[upd]
        t32 = np.minimum(F32(1), sdf / trunc)
        t64 = np.minimum(1.0, sdf.astype(F64) / F64(trunc))
        w32, w64 = weight[r, l].astype(F32), weight[r, l].astype(F64)
        tsdf32[r, l] = (tsdf32[r, l] * w32 + t32) / (w32 + F32(1))
        tsdf64[r, l] = (tsdf64[r, l] * w64 + t64) / (w64 + 1.0)
        tmax[r, l] = np.maximum(tmax[r, l], np.abs(t64))
        weight[r, l] += 1
    return dict(units=units, weight=weight, tsdf32=tsdf32, tsdf64=tsdf64, tmax=tmax, borderline=borderline, per_camera=per_cam,
                voxel_length=float(vl), unit_length=float(ul), sdf_trunc=float(trunc))


def dense_volume(units, tsdf, weight):
    """(origin unit (3,), tsdf (nx, ny, nz) fp32, valid bool) over the bounding box of the units."""
    org = units.min(0)
    dims = (units.max(0) - org + 1) * 16
    vol, valid = np.zeros(dims, F32), np.zeros(dims, bool)
    for s, U in enumerate(units):
        o = (U - org) * 16
        vol[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16] = np.asarray(tsdf[s], F32).reshape(16, 16, 16)
        valid[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16] = (np.asarray(weight[s]) > 0).reshape(16, 16, 16)
    return org, vol, valid


def tsdf_extract(units, tsdf, weight, voxel_length):
    """Rule 5 -> (verts (V, 3) fp32, faces (F, 3) int64) -- vertices in dense lattice order (the library's order is unit, voxel, axis),
    so compare them as sets."""
    units = np.asarray(units, np.int64)
    if units.shape[0] == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int64)
    vl = F32(voxel_length)
    ul = F32(F32(16.0) * vl)
    org, vol, valid = dense_volume(units, tsdf, weight)
    nx, ny, nz = vol.shape
    above = ~(vol < 0)
    cv = np.ones((nx - 1, ny - 1, nz - 1), bool)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = M.CORNER_OFF[c]
        sl = (slice(dx, nx - 1 + dx), slice(dy, ny - 1 + dy), slice(dz, nz - 1 + dz))
        cv &= valid[sl]
        case |= above[sl].astype(np.int64) << c
    cvp = np.zeros((nx + 1, ny + 1, nz + 1), bool)                        # cvp[p + 1] = the cell whose low corner is p counts
    cvp[1:nx, 1:ny, 1:nz] = cv
    cross = np.zeros(vol.shape + (3,), bool)
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        used = np.zeros(vol.shape, bool)
        for ob in (0, 1):
            for od in (0, 1):
                sl = [slice(1, None)] * 3
                sl[b] = slice(1 - ob, cvp.shape[b] - ob)
                sl[d] = slice(1 - od, cvp.shape[d] - od)
                used |= cvp[tuple(sl)]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        cr = np.zeros(vol.shape, bool)
        cr[tuple(lo)] = above[tuple(lo)] != above[tuple(hi)]
        cross[..., a] = cr & used
    flat = cross.reshape(-1)
    vid = np.full(flat.shape[0], -1, np.int64)
    ids = np.nonzero(flat)[0]
    vid[ids] = np.arange(ids.shape[0])
    p, axis = ids // 3, ids % 3
    idx = np.stack(np.unravel_index(p, vol.shape), -1)
    e = np.eye(3, dtype=np.int64)[axis]
    f0 = vol.reshape(-1)[p]
    f1 = vol.reshape(-1)[np.ravel_multi_index((idx + e).T, vol.shape)]
    with np.errstate(all="ignore"):
        t = (F32(0) - f0) / (f1 - f0)
    centre = (org + idx // 16).astype(F32) * ul + ((idx % 16).astype(F32) + F32(0.5)) * vl
    verts = np.where(e == 1, centre + (t * vl)[:, None], centre).astype(F32)
    case = np.where(cv, case, 0).reshape(-1)
    ci = np.nonzero(M.NUM_TRI[case] > 0)[0]
    nt = M.NUM_TRI[case[ci]]
    cell = np.repeat(ci, nt)
    slot = np.arange(cell.shape[0]) - np.repeat(np.cumsum(nt) - nt, nt)
    edges = M.TRI_TABLE[case[cell], slot].astype(np.int64)
    cidx = np.stack(np.unravel_index(cell, (nx - 1, ny - 1, nz - 1)), -1)
    owner = cidx[:, None, :] + M.CORNER_OFF[M.EDGE_LO[edges]]
    pl = np.ravel_multi_index(owner.reshape(-1, 3).T, vol.shape).reshape(edges.shape)
    faces = vid[pl * 3 + M.EDGE_AXIS[edges]]
    assert (faces >= 0).all()
    return verts, faces


# -------------------------------------------------------------------------------------------------------- scene builders
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """Camera-to-world 4 x 4 (x right, y down, z forward) of a camera at `eye` looking at `target`."""
    eye, target, up = (np.asarray(a, F64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def box_mesh(lo, hi, inward=False):
    """A closed box as 12 triangles; right-hand normals outwards, or inwards (a room seen from inside)."""
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    c = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)])
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]   # -x +x -y +y -z +z
    f = np.array([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))], np.int64)
    nrm = np.cross(c[f[:, 1]] - c[f[:, 0]], c[f[:, 2]] - c[f[:, 0]])
    out = (nrm * (c[f].mean(1) - 0.5 * (lo + hi))).sum(1) > 0
    f = np.where((out != inward)[:, None], f, f[:, ::-1])               # right-hand normal away from the centre, or towards it
    return c.astype(F32), np.ascontiguousarray(f).astype(np.int32)


def merge(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, F32))
        fs.append(np.asarray(f, np.int64) + off)
        off += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.int32)


def uv_sphere(radius, n_lat, n_lon, centre=(0.0, 0.0, 0.0)):
    """A closed latitude / longitude sphere, right-hand normals outwards; vertices ON the sphere."""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    f = []
    idx = lambda i, j: 1 + i * n_lon + j % n_lon
    last = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        f.append((0, idx(0, j), idx(0, j + 1)))
        f.append((last, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)))
        for i in range(n_lat - 2):
            f.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return v.astype(F32), np.array(f, np.int32)


def box_sdf_volume(lo, hi, n, pad=0.1):
    """(vol (n, n, n) fp32, spacing (3,), origin (3,)): the signed distance to the box [lo, hi], NEGATED (positive inside), on a grid
    that is `pad` larger on every side -- its zero-level mesh has right-hand normals towards the inside: a room's inner surface."""
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    org = lo - pad
    sp = (hi - lo + 2 * pad) / (n - 1)
    g = [org[k] + sp[k] * np.arange(n) for k in range(3)]
    X = np.stack(np.meshgrid(*g, indexing="ij"), -1)
    q = np.abs(X - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    sdf = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
    return (-sdf).astype(F32), sp, org


# ------------------------------------------------------------------------------------------ the scene of the GPU tests
# A 1.0 x 0.8 x 0.6 room with a partition slab at x in [0.70, 0.76]: the cameras stand in x < 0.70, the chamber behind the slab is
# seen by none.  "pred" is what a network would give: the visible part of the room, a solid chamber with a small void box hidden in
# it, and an outer shell 0.15 outside the room; "trgt" is the true room with its slab and the empty chamber.
ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.8, 0.6])
SLAB_LO, SLAB_HI = np.array([0.70, 0.0, 0.0]), np.array([0.76, 0.8, 0.6])
VIS_LO, VIS_HI = ROOM_LO, np.array([0.70, 0.8, 0.6])                    # the part of the room the cameras stand in (convex)
SHELL_LO, SHELL_HI = ROOM_LO - 0.15, ROOM_HI + 0.15
HIDDEN_LO, HIDDEN_HI = np.array([0.82, 0.3, 0.2]), np.array([0.92, 0.5, 0.4])
VOXEL = 0.02


def _box_sdf(X, lo, hi):
    q = np.abs(X - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)


def _lattice(lo, hi, n):
    sp = (hi - lo) / (n - 1)
    X = np.stack(np.meshgrid(*[lo[k] + sp[k] * np.arange(n) for k in range(3)], indexing="ij"), -1)
    return X, sp, lo


def scene_volumes():
    """{name: (vol fp32, spacing, origin)}: volumes that are positive in free space, so that their zero-level meshes
    (marching_cubes: right-hand normals towards increasing values) face the free space."""
    X, sp, org = _lattice(ROOM_LO - 0.1, ROOM_HI + 0.1, 48)
    trgt = np.minimum(-_box_sdf(X, ROOM_LO, ROOM_HI), _box_sdf(X, SLAB_LO, SLAB_HI))
    Xp, spp, orgp = _lattice(SHELL_LO - 0.1, SHELL_HI + 0.1, 64)
    pred = np.maximum(np.maximum(-_box_sdf(Xp, VIS_LO, VIS_HI), -_box_sdf(Xp, HIDDEN_LO, HIDDEN_HI)), _box_sdf(Xp, SHELL_LO, SHELL_HI))
    return {"trgt": (trgt.astype(F32), sp, org), "pred": (pred.astype(F32), spp, orgp)}


def scene_triangles():
    """The same two scenes as a few large triangles each."""
    trgt = merge(box_mesh(ROOM_LO, ROOM_HI, inward=True), box_mesh(SLAB_LO, SLAB_HI))
    pred = merge(box_mesh(VIS_LO, VIS_HI, inward=True), box_mesh(HIDDEN_LO, HIDDEN_HI, inward=True), box_mesh(SHELL_LO, SHELL_HI))
    return {"trgt": trgt, "pred": pred}


def scene_cameras(H, W):
    """(poses (6, 4, 4), K 3 x 3): six cameras in the visible part of the room, one looking at each of its faces from positions that are
    no round numbers (no voxel lattice line projects onto a pixel boundary by construction); the horizontal field of view is 62 degrees."""
    eye = np.array([0.3471, 0.4093, 0.2957])
    P = [look_at(eye + [0.11, 0.013, 0.007], eye + [-1, 0.05, 0.02]), look_at(eye - [0.13, 0.021, 0.011], eye + [1, -0.04, 0.03]),
         look_at(eye + [0.02, 0.09, -0.01], eye + [0.03, -1, 0.04]), look_at(eye + [-0.03, -0.12, 0.02], eye + [0.02, 1, -0.05]),
         look_at(eye + [0.01, 0.02, 0.08], eye + [0.04, 0.03, -1], up=(0.0, 1.0, 0.0)),
         look_at(eye + [-0.02, 0.01, -0.07], eye + [-0.03, 0.02, 1], up=(0.0, 1.0, 0.0))]
    f = 0.83 * W
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]])
    return np.stack(P), K


def overlapping_cameras(H, W):
    """(poses (6, 4, 4), K 3 x 3) for the fusion tests: two groups of three cameras, each group looking at one corner of the visible
    part of the room from three different places across it, so that the truncation bands of the walls around that corner are crossed
    by up to three (where the groups' views meet, more) cameras with a different fractional t each -- the running average
    tsdf <- (tsdf w + t) / (w + 1) is exercised with w = 1, 2, ..., which cameras that each face a wall of their own never do.
    Same intrinsics and the same kind of positions (no round numbers) as scene_cameras."""
    P = [look_at((0.5531, 0.6173, 0.4419), (0.0512, 0.1033, 0.0871)), look_at((0.6127, 0.4391, 0.3517), (0.0093, 0.2117, 0.1479)),
         look_at((0.4873, 0.6611, 0.2893), (0.1091, 0.0477, 0.2113)),
         look_at((0.1217, 0.1531, 0.1193), (0.6491, 0.7013, 0.5077)), look_at((0.0971, 0.3079, 0.2011), (0.6913, 0.6029, 0.4483)),
         look_at((0.2039, 0.1171, 0.2537), (0.6053, 0.7487, 0.4091))]
    return np.stack(P), scene_cameras(H, W)[1]


def distance_to_box_surface(p, lo, hi):
    return np.abs(_box_sdf(np.asarray(p, F64), lo, hi))


def visible_lattice(c2w, w2c, K, H, W, far_clip=5.0, n=9, inset=0.03):
    """(points (6 n^2, 3), seen): a fixed lattice on the six faces of the visible part of the room, and which of its points some camera
    sees within far_clip, inside the image by more than 2 px and at an incidence below 70 degrees.  That part of the room is convex and
    the cameras stand inside it, so nothing occludes a surface point from a camera."""
    g = [np.linspace(VIS_LO[k] + inset, VIS_HI[k] - inset, n) for k in range(3)]
    pts, nrm = [], []
    for ax in range(3):
        for side, x in ((0, VIS_LO[ax]), (1, VIS_HI[ax])):
            o = [a for a in range(3) if a != ax]
            A, B = np.meshgrid(g[o[0]], g[o[1]], indexing="ij")
            p = np.zeros(A.shape + (3,))
            p[..., ax], p[..., o[0]], p[..., o[1]] = x, A, B
            pts.append(p.reshape(-1, 3))
            nn = np.zeros(3)
            nn[ax] = 1.0 if side == 0 else -1.0                         # towards the inside
            nrm.append(np.tile(nn, (A.size, 1)))
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    seen = np.zeros(pts.shape[0], bool)
    fx, fy, cx, cy = (float(x) for x in k4_of(K))
    for k in range(w2c.shape[0]):
        q = transform(w2c[k].astype(F64), pts)
        with np.errstate(all="ignore"):
            u, v = q[:, 0] / q[:, 2] * fx + cx, q[:, 1] / q[:, 2] * fy + cy
        to_eye = c2w[k][:, 3].astype(F64) - pts
        cosi = (to_eye * nrm).sum(1) / np.linalg.norm(to_eye, axis=1)
        seen |= (q[:, 2] > 0.05) & (q[:, 2] < far_clip) & (u > 2) & (u < W - 3) & (v > 2) & (v < H - 3) & (cosi > np.cos(np.radians(70)))
    return pts, seen
