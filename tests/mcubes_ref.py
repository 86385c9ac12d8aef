"""Numpy restatement of the library's marching cubes (csrc/mcubes.hip): the same case tables (csrc/gen_mc_tables.py), the same
vertex / face order and the same fp32 arithmetic, vectorised.  Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "i2sdf_amd", "csrc"))
import gen_mc_tables as G  # noqa: E402

TRI_TABLE, NUM_TRI, MAX_TRI = G.tables()
EDGE_AXIS = np.array([G.edge_axis(e) for e in range(12)])
EDGE_LO = np.array([G.EDGES[e][0] for e in range(12)])
CORNER_OFF = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])


def gradient(vol, spacing):
    """np.gradient(vol, *spacing) in fp32: central differences over 2*spacing inside, one-sided at the border."""
    g = np.empty(vol.shape + (3,), np.float32)
    for a in range(3):
        s = np.float32(spacing[a])
        v = np.moveaxis(vol, a, 0)
        d = np.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) / (np.float32(2) * s)
        d[0] = (v[1] - v[0]) / s
        d[-1] = (v[-1] - v[-2]) / s
        g[..., a] = np.moveaxis(d, 0, a)
    return g


def marching_cubes(vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """-> verts (V,3) fp32, faces (F,3) int32, normals (V,3) fp32 in the library's order."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    lev = np.float32(level)
    sp, org = np.asarray(spacing, np.float32), np.asarray(origin, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        above = vol > lev
        # crossing edges owned by each lattice point (its +x, +y, +z edge)
        cross = np.zeros(vol.shape + (3,), bool)
        cross[:-1, :, :, 0] = above[:-1] != above[1:]
        cross[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
        cross[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
        flat = cross.reshape(-1)
        vid = np.full(flat.shape[0], -1, np.int64)
        ids = np.nonzero(flat)[0]                                   # lattice-point linear index, then axis x < y < z
        vid[ids] = np.arange(ids.shape[0])
        p, axis = ids // 3, ids % 3
        idx = np.stack(np.unravel_index(p, vol.shape), -1)
        e = np.eye(3, dtype=np.int64)[axis]
        v0 = vol.reshape(-1)[p]
        v1 = vol.reshape(-1)[np.ravel_multi_index((idx + e).T, vol.shape)]
        t = (lev - v0) / (v1 - v0)
        verts = org + (idx.astype(np.float32) + t[:, None] * e.astype(np.float32)) * sp
        g = gradient(vol, sp).reshape(-1, 3)
        g0, g1 = g[p], g[np.ravel_multi_index((idx + e).T, vol.shape)]
        n = (np.float32(1) - t)[:, None] * g0 + t[:, None] * g1
        nrm = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        normals = -(n / nrm[:, None])
        # cells, in cell linear order, then table slot
        case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
        for c in range(8):
            dx, dy, dz = CORNER_OFF[c]
            case |= above[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    case = case.reshape(-1)
    ci = np.nonzero(NUM_TRI[case] > 0)[0]
    nt = NUM_TRI[case[ci]]
    cell = np.repeat(ci, nt)
    slot = np.arange(cell.shape[0]) - np.repeat(np.cumsum(nt) - nt, nt)
    edges = TRI_TABLE[case[cell], slot].astype(np.int64)                    # (F,3)
    cidx = np.stack(np.unravel_index(cell, (nx - 1, ny - 1, nz - 1)), -1)   # (F,3) cell lattice point
    owner = cidx[:, None, :] + CORNER_OFF[EDGE_LO[edges]]                    # (F,3,3)
    pl = np.ravel_multi_index(owner.reshape(-1, 3).T, vol.shape).reshape(edges.shape)
    faces = vid[pl * 3 + EDGE_AXIS[edges]]
    assert (faces >= 0).all()
    return verts.astype(np.float32), faces.astype(np.int32), normals.astype(np.float32)


def edge_keys(vol_shape, verts, spacing, origin):
    """Lattice edge (point linear index * 3 + axis) of each vertex, from its position (scikit-image puts one vertex per crossing
    edge on smooth volumes): the one coordinate that is off the lattice names the axis."""
    q = (np.asarray(verts, np.float64) - np.asarray(origin, np.float64)) / np.asarray(spacing, np.float64)
    off = np.abs(q - np.round(q))
    axis = np.argmax(off, axis=1)                 # (a vertex on a lattice point, t = 0 or 1, is given to its +axis edge below)
    base = np.round(q).astype(np.int64)
    rows = np.arange(q.shape[0])
    base[rows, axis] = np.floor(q[rows, axis] + 1e-4).astype(np.int64)
    base = np.minimum(base, np.array(vol_shape) - 1)
    return np.ravel_multi_index(base.T, vol_shape) * 3 + axis


def mesh_stats(verts, faces):
    """(area, signed volume, Euler characteristic, closed: every undirected edge in exactly two faces, directed edges unique)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cr = np.cross(b - a, c - a)
    area = 0.5 * np.linalg.norm(cr, axis=1).sum()
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = max(int(f.max()) + 1, len(v)) if len(f) else len(v)
    dkey = de[:, 0] * n + de[:, 1]
    ukey = np.minimum(de[:, 0], de[:, 1]) * n + np.maximum(de[:, 0], de[:, 1])
    _, ucount = np.unique(ukey, return_counts=True)
    closed = bool((ucount == 2).all())
    directed_unique = np.unique(dkey).shape[0] == dkey.shape[0]
    used = np.unique(f).shape[0]
    euler = used - ucount.shape[0] + f.shape[0]
    return area, vol, euler, closed, directed_unique
