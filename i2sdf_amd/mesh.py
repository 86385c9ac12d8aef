"""Marching cubes on the device (csrc/mcubes.hip): the zero-level mesh of an SDF volume, in place of the host round trip
`volume.cpu().numpy()` -> `skimage.measure.marching_cubes` of model/eval/recon.py:53-60,91-95 and utils/plots.py:197-206.

Conventions are scikit-image's (Lewiner, gradient_direction='descent'): one vertex per lattice edge that crosses the level,
at linear interpolation; `verts` in index units x spacing (+ origin); int32 faces whose right-hand normal points towards
increasing values; `normals` pointing towards DEcreasing values (inward for an SDF).  Two differences:
  * ambiguous cells follow one fixed rule (csrc/gen_mc_tables.py) instead of Lewiner's, so on non-smooth volumes the
    triangulation of those cells differs (the mesh is still closed and consistently oriented);
  * a volume without any crossing gives empty tensors where scikit-image raises (and the reference returns None).
`values` is not returned (no reference call site reads it).

Mesh operations on the device (csrc/meshops.hip), the trimesh calls between the reference's two marching-cubes passes:
  * face_components    labels of `mesh.split(only_watertight=False)` (utils/plots.py:282): the smallest face index of each face's
                       component.  Faces are connected through a shared edge; unlike trimesh's face_adjacency an edge shared by
                       three or more faces connects them too (on a marching-cubes mesh the two rules agree);
  * largest_component  `components[areas.argmax()]` (utils/plots.py:283-284) as a compacted sub-mesh;
  * sample_surface     `trimesh.sample.sample_surface(mesh, count)` (utils/plots.py:286, model/eval/recon.py:62) with explicit
                       uniform draws, so that a run can be repeated and checked.
All of them are bitwise reproducible from run to run (integer atomics only, fp64 sums in a fixed order).

Scoring on the device (csrc/pointops.hip), the step the reference takes right after the export (utils/mesh_util.py:evaluate,
called by model/eval/recon.py:111-129, where open3d and a scikit-learn KDTree run on the host):
  * voxel_down_sample  open3d's `voxel_down_sample` rule (mesh_util.py:32-34) with pinned arithmetic: voxel indices in fp64, every
                       mean an fp64 sum in original index order; voxels in ascending (ix, iy, iz) order, not a hash map's;
  * nearest_neighbors  `KDTree(ref).query(query)` (mesh_util.py:12-22): exact fp32 distances and indices through a uniform grid
                       with a shell search and a brute-force second pass for the queries the grid cannot answer cheaply;
  * evaluate           Acc / Comp / Prec / Recal / F-score (mesh_util.py:25-52) of two vertex sets.  It scores whatever vertex
                       sets it is given; the reference's visibility culling (mesh_util.refuse) is not part of this library.
These are bitwise reproducible as well.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import torch

from . import lib as L


class Mesh(NamedTuple):
    verts: torch.Tensor      # (V, 3) fp32
    faces: torch.Tensor      # (F, 3) int32
    normals: torch.Tensor    # (V, 3) fp32


def _f3(x, what):
    vals = [float(v) for v in (x if hasattr(x, "__len__") else (x, x, x))]
    if len(vals) != 3:
        raise ValueError(f"{what}: expected 3 values, got {len(vals)}")
    import ctypes as C
    return (C.c_float * 3)(*vals)


@torch.no_grad()
def marching_cubes(volume: torch.Tensor, level: float = 0.0, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                   origin: Sequence[float] = (0.0, 0.0, 0.0)) -> Mesh:
    """Mesh of the `level` set of a device volume (nx, ny, nz), z fastest (I2SDFNetwork.sdf_volume's default order).
    Returns device tensors; one host synchronisation reads the vertex and face counts to size them."""
    if not torch.is_tensor(volume) or volume.dim() != 3 or not volume.is_cuda:
        raise ValueError("marching_cubes: volume must be a 3-d tensor on a GPU")
    vol = volume.to(torch.float32).contiguous()
    nx, ny, nz = vol.shape
    if min(nx, ny, nz) < 2:
        raise ValueError(f"marching_cubes: every axis needs at least 2 points, volume is {tuple(vol.shape)}")
    lib = L.load()
    dev = vol.device
    sp, org = _f3(spacing, "spacing"), _f3(origin, "origin")
    with torch.cuda.device(dev):
        nbytes = int(lib.i2sdf_marching_cubes_workspace_bytes(nx, ny, nz))
        if nbytes <= 0:
            raise ValueError(f"marching_cubes: volume shape {tuple(vol.shape)} not supported")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        st = L.stream_ptr()
        L.check(lib.i2sdf_marching_cubes_count(L.ptr(vol), nx, ny, nz, float(level), L.ptr(ws), L.ptr(counts), st),
                "i2sdf_marching_cubes_count")
        n_v, n_f = counts.tolist()
        if max(n_v, n_f) > 2 ** 31 - 1:
            raise L.I2SDFError(f"marching_cubes: {n_v} vertices / {n_f} faces do not fit int32 indices")
        verts = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        normals = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
        L.check(lib.i2sdf_marching_cubes_emit(L.ptr(vol), nx, ny, nz, float(level), sp, org, L.ptr(ws), L.ptr(verts), L.ptr(normals),
                                              L.ptr(faces), n_v, n_f, st), "i2sdf_marching_cubes_emit")
    return Mesh(verts, faces, normals)


def _mesh_args(mesh, what):
    verts, faces = mesh[0], mesh[1]
    normals = mesh[2] if len(mesh) > 2 else None
    for t, dt, name in ((verts, torch.float32, "verts"), (faces, torch.int32, "faces"), (normals, torch.float32, "normals")):
        if t is None and name == "normals":
            continue
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be a (n, 3) {dt} tensor on a GPU")
    if normals is not None and normals.shape[0] != verts.shape[0]:
        raise ValueError(f"{what}: {normals.shape[0]} normals for {verts.shape[0]} vertices")
    return verts.contiguous(), faces.contiguous(), None if normals is None else normals.contiguous()


def _components(faces, n_verts, status):
    """labels (F,) int32 of contiguous device faces; enqueues only (a bad face index sets `status`)."""
    lib = L.load()
    F, dev = faces.shape[0], faces.device
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return labels
    st = L.stream_ptr()
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    L.check(lib.i2sdf_mesh_edge_keys(L.ptr(faces), F, n_verts, L.ptr(keys), L.ptr(status), st), "i2sdf_mesh_edge_keys")
    skeys, perm = torch.sort(keys)                 # (the order inside a run of equal keys does not change the labels)
    del keys
    L.check(lib.i2sdf_mesh_face_components(L.ptr(skeys), L.ptr(perm), F, L.ptr(labels), st), "i2sdf_mesh_face_components")
    return labels


def _area_cdf(verts, faces, status, order=None):
    """fp32 face areas and their fp64 running sum (in `order`, a permutation of the faces, when given); enqueues only."""
    lib = L.load()
    F, dev = faces.shape[0], faces.device
    area = torch.empty(F, dtype=torch.float32, device=dev)
    cdf = torch.empty(F, dtype=torch.float64, device=dev)
    if F == 0:
        return area, cdf
    st = L.stream_ptr()
    L.check(lib.i2sdf_mesh_face_areas(L.ptr(verts), verts.shape[0], L.ptr(faces), F, L.ptr(area), L.ptr(status), st),
            "i2sdf_mesh_face_areas")
    ws = torch.empty(int(lib.i2sdf_mesh_scan_workspace_bytes(F)), dtype=torch.uint8, device=dev)
    L.check(lib.i2sdf_mesh_cumsum_f64(L.ptr(area), F, L.ptr(order), F, L.ptr(cdf), L.ptr(ws), st), "i2sdf_mesh_cumsum_f64")
    return area, cdf


def _new_status(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _bad_faces(what):
    return L.I2SDFError(f"{what} failed (-1): a face holds a vertex index outside [0, n_verts)")


@torch.no_grad()
def face_components(mesh_or_faces, n_verts: int = None) -> torch.Tensor:
    """labels (F,) int32: labels[f] is the smallest face index of the component of face f, where two faces are connected when
    they share an edge (an unordered pair of vertex indices) and components are the transitive closure.  This is trimesh's
    face_adjacency rule behind `Trimesh.split(only_watertight=False)`, except that an edge shared by three or more faces also
    connects them (trimesh ignores such edges); a shared single vertex does not connect.
    `mesh_or_faces`: a Mesh / (verts, faces, ...) tuple, or the (F, 3) int32 device faces with `n_verts` (None: indices are
    only required to be non-negative).  One host synchronisation reads the validation word."""
    if torch.is_tensor(mesh_or_faces):
        faces = mesh_or_faces
        n_verts = 2 ** 31 - 1 if n_verts is None else int(n_verts)
    else:
        faces = mesh_or_faces[1]
        n_verts = int(mesh_or_faces[0].shape[0]) if n_verts is None else int(n_verts)
    if not torch.is_tensor(faces) or not faces.is_cuda or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("face_components: faces must be a (F, 3) int32 tensor on a GPU")
    if not 0 <= n_verts <= 2 ** 31 - 1 or faces.shape[0] > 2 ** 31 - 1:
        raise ValueError("face_components: vertex and face counts must fit int32")
    faces = faces.contiguous()
    with torch.cuda.device(faces.device):
        status = _new_status(faces.device)
        labels = _components(faces, n_verts, status)
        L.check(L.load().i2sdf_mesh_status(L.ptr(status), L.stream_ptr()), "face_components: face indices")
    return labels


@torch.no_grad()
def compact(mesh, face_mask: torch.Tensor, _status=None) -> Mesh:
    """The sub-mesh of the faces where `face_mask` (F,) bool is set: kept faces in their original order, the vertices they
    still reference in their original order, faces re-indexed, normals carried along.  One host synchronisation reads the two
    counts that size the result."""
    verts, faces, normals = _mesh_args(mesh, "compact")
    F, V, dev = faces.shape[0], verts.shape[0], faces.device
    if not torch.is_tensor(face_mask) or face_mask.device != dev or face_mask.dtype != torch.bool or face_mask.shape != (F,):
        raise ValueError("compact: face_mask must be a (F,) bool tensor on the mesh's device")
    lib = L.load()
    with torch.cuda.device(dev):
        status = _new_status(dev) if _status is None else _status
        st = L.stream_ptr()
        fkeep = torch.empty(F, dtype=torch.int32, device=dev)
        vflag = torch.empty(V, dtype=torch.int32, device=dev)
        L.check(lib.i2sdf_mesh_compact_mark(L.ptr(faces), L.ptr(face_mask.contiguous().view(torch.uint8)), F, V, L.ptr(fkeep), L.ptr(vflag),
                                            L.ptr(status), st), "i2sdf_mesh_compact_mark")
        fscan = torch.cumsum(fkeep, 0, dtype=torch.int32)
        vscan = torch.cumsum(vflag, 0, dtype=torch.int32)
        last = lambda t: t[-1:] if t.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        n_f, n_v, bad = torch.cat([last(fscan), last(vscan), status]).tolist()
        if bad:
            raise _bad_faces("compact")
        out_v = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        out_n = None if normals is None else torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
        L.check(lib.i2sdf_mesh_compact_gather(L.ptr(verts), L.ptr(normals), V, L.ptr(faces), F, L.ptr(fkeep), L.ptr(fscan), L.ptr(vflag),
                                              L.ptr(vscan), L.ptr(out_v), L.ptr(out_n), L.ptr(out_f), n_v, n_f, st),
                "i2sdf_mesh_compact_gather")
    return Mesh(out_v, out_f, out_n)


@torch.no_grad()
def largest_component(mesh) -> Mesh:
    """The component (face_components) with the largest surface area as a compacted Mesh -- `components[areas.argmax()]` of
    utils/plots.py:282-284.  Face areas are fp32, component areas their fp64 sums in a fixed order (faces sorted by label,
    stable); ties go to the smaller label.  An empty mesh is returned as it is.  Everything stays on the device; the one host
    synchronisation is compact()'s."""
    verts, faces, normals = _mesh_args(mesh, "largest_component")
    F, dev = faces.shape[0], faces.device
    if F == 0:
        return Mesh(verts, faces, normals)
    lib = L.load()
    with torch.cuda.device(dev):
        status = _new_status(dev)
        labels = _components(faces, verts.shape[0], status)
        slab, order = torch.sort(labels, stable=True)
        _, cdf = _area_cdf(verts, faces, status, order)
        best = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(lib.i2sdf_mesh_largest_label(L.ptr(slab), L.ptr(cdf), F, L.ptr(best), L.stream_ptr()), "i2sdf_mesh_largest_label")
        mask = labels == best[1]
        return compact(Mesh(verts, faces, normals), mask, _status=status)


@torch.no_grad()
def sample_surface(mesh, count: int, draws=None, generator=None, _check=True):
    """`trimesh.sample.sample_surface(mesh, count)` on the device -> (points (count, 3) fp32, face_index (count,) int32).
    Faces are drawn with probability proportional to their area through the fp64 running sum of the fp32 face areas
    (pick = u_face * total; the first face whose running sum reaches it, np.searchsorted side='left'), points uniformly inside
    them from two more uniforms (reflected when they leave the triangle).  A face of zero area is never drawn, except face 0
    by a draw of exactly 0 (as in trimesh) and when every area is zero.
    draws: {"u_face": (count,), "u_bary": (count, 2)} fp32 in [0, 1) on the mesh's device; missing entries come from torch.rand
    with `generator`.  One host synchronisation reads the validation word."""
    verts, faces, _ = _mesh_args(mesh[:2], "sample_surface")
    count, F, dev = int(count), faces.shape[0], faces.device
    if count < 0:
        raise ValueError("sample_surface: count must not be negative")
    draws = draws or {}
    got = {}
    for name, shape in (("u_face", (count,)), ("u_bary", (count, 2))):
        u = draws.get(name)
        if u is None:
            u = torch.rand(*shape, device=dev, generator=generator)
        if not torch.is_tensor(u) or u.device != dev or u.dtype != torch.float32 or tuple(u.shape) != shape:
            raise ValueError(f"sample_surface: draws['{name}'] must be a {shape} fp32 tensor on the mesh's device")
        got[name] = u.contiguous()
    points = torch.empty(count, 3, dtype=torch.float32, device=dev)
    face_index = torch.empty(count, dtype=torch.int32, device=dev)
    if count == 0:
        return points, face_index
    if F == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    lib = L.load()
    with torch.cuda.device(dev):
        status = _new_status(dev)
        _, cdf = _area_cdf(verts, faces, status)
        st = L.stream_ptr()
        L.check(lib.i2sdf_mesh_sample_surface(L.ptr(verts), verts.shape[0], L.ptr(faces), F, L.ptr(cdf), L.ptr(got["u_face"]),
                                              L.ptr(got["u_bary"]), count, L.ptr(points), L.ptr(face_index), L.ptr(status), st),
                "i2sdf_mesh_sample_surface")
        if _check:                                 # (extract_mesh_high_res samples meshes the library made itself)
            L.check(lib.i2sdf_mesh_status(L.ptr(status), st), "sample_surface: face indices")
    return points, face_index


# ------------------------------------------------------------------------------------------------ scoring (csrc/pointops.hip)
def _points_arg(x, what, name):
    """(n, 3) fp32 device points of a Mesh / (verts, faces, ...) tuple or of a bare tensor."""
    if not torch.is_tensor(x):
        if not isinstance(x, (tuple, list)) or len(x) == 0:
            raise ValueError(f"{what}: {name} must be a (n, 3) fp32 tensor on a GPU or a Mesh")
        x = x[0]
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what}: {name} must be a (n, 3) fp32 tensor on a GPU")
    if x.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{what}: {name} must hold at most 2^31 - 1 points")
    return x.contiguous()


def _points_status(dev):
    return torch.zeros(2, dtype=torch.int32, device=dev)       # (flags, fallback count): include/i2sdf.h


def _raise_points_status(flags, what):
    if flags & 1:
        raise L.I2SDFError(f"{what} failed (-1): a coordinate is not finite")
    if flags & 2:
        raise L.I2SDFError(f"{what} failed (-1): a voxel index does not fit 21 bits per axis (voxel_size too small for the extent)")


@torch.no_grad()
def voxel_down_sample(points: torch.Tensor, voxel_size: float, _stats=None):
    """open3d's `PointCloud.voxel_down_sample(voxel_size)` (utils/mesh_util.py:evaluate) on the device ->
    (points_out (M, 3) fp32, counts (M,) int32): the mean of the points of every occupied voxel, where
    lo = min(points) - voxel_size / 2 per axis and a point's voxel is floor((p - lo) / voxel_size), computed in fp64 from the fp32
    coordinates.  Each mean is the fp64 sum of the voxel's points in original index order, divided by their number, rounded to
    fp32.  Voxels come in ascending (ix, iy, iz) order (open3d's order is that of its hash map).  Bitwise reproducible from run
    to run.  A non-finite coordinate, or a voxel index beyond 21 bits per axis, raises I2SDFError.  One host synchronisation
    reads M (and the validation word)."""
    pts = _points_arg(points, "voxel_down_sample", "points")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0) or voxel_size == float("inf"):
        raise ValueError("voxel_down_sample: voxel_size must be positive and finite")
    N, dev = pts.shape[0], pts.device
    if N == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    lib = L.load()
    ev = _marker(_stats)
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        status = _points_status(dev)
        bounds = torch.empty(8, dtype=torch.int32, device=dev)
        keys = torch.empty(N, dtype=torch.int64, device=dev)
        heads = torch.empty(N, dtype=torch.int32, device=dev)
        ev("start")
        L.check(lib.i2sdf_points_bounds(L.ptr(pts), N, L.ptr(bounds), L.ptr(status), st), "i2sdf_points_bounds")
        L.check(lib.i2sdf_points_voxel_keys(L.ptr(pts), N, L.ptr(bounds), voxel_size, L.ptr(keys), L.ptr(status), st),
                "i2sdf_points_voxel_keys")
        skeys, perm = torch.sort(keys, stable=True)            # stable: a voxel's points stay in original index order
        del keys
        ev("voxel_keys_sort")
        L.check(lib.i2sdf_points_voxel_heads(L.ptr(skeys), N, L.ptr(heads), st), "i2sdf_points_voxel_heads")
        scan = torch.cumsum(heads, 0, dtype=torch.int32)
        M, flags = torch.cat([scan[-1:], status[:1]]).tolist()
        _raise_points_status(flags, "voxel_down_sample")
        out = torch.empty(M, 3, dtype=torch.float32, device=dev)
        counts = torch.empty(M, dtype=torch.int32, device=dev)
        L.check(lib.i2sdf_points_voxel_mean(L.ptr(pts), N, L.ptr(skeys), L.ptr(perm), L.ptr(scan), L.ptr(out), L.ptr(counts), M, st),
                "i2sdf_points_voxel_mean")
        ev("voxel_mean")
    return out, counts


def _marker(stats):
    """ev(label): appends (label, event recorded now) to `stats`, the per-stage record scripts/mesh_eval_timing.py reads."""
    if stats is None:
        return lambda label: None

    def ev(label):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        stats.append((label, e))
    return ev


def _ring_budget(R):
    """Shells a query may search before it goes to the brute-force pass: as long as a shell block's cells ((2r + 1)^3) stay
    below the R / 32 a wave-per-query pass over R points costs per lane, and never more than 8."""
    r = 1
    while r < 8 and (2 * (r + 1) + 1) ** 3 <= R // 32:
        r += 1
    return r


@torch.no_grad()
def nearest_neighbors(query: torch.Tensor, ref: torch.Tensor, _stats=None):
    """Exact Euclidean nearest neighbour of every query among `ref` -> (dist (Q,) fp32, index (Q,) int32), what
    `sklearn.neighbors.KDTree(ref).query(query)` returns (utils/mesh_util.py:nn_correspondance).  Distances are computed in fp32
    from fp32 differences; equal distances go to the smallest reference index.  Exact wherever the query lies: `ref` is hashed
    into a uniform grid (whose cell count is capped whatever the bounding box), every query searches shells of cells around its
    own until the best distance is inside the searched shell, and the queries that exhaust a small shell budget (far from the
    cloud, or in its large empty parts) are answered by a brute-force pass over `ref`, one wave per query.
    Q = 0 gives empty tensors; R = 0 raises ValueError, a non-finite coordinate I2SDFError.  One host synchronisation reads the
    validation word."""
    q = _points_arg(query, "nearest_neighbors", "query")
    r = _points_arg(ref, "nearest_neighbors", "ref")
    if q.device != r.device:
        raise ValueError("nearest_neighbors: query and ref must be on the same device")
    Q, R, dev = q.shape[0], r.shape[0], q.device
    if R == 0:
        raise ValueError("nearest_neighbors: ref is empty")
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    index = torch.empty(Q, dtype=torch.int32, device=dev)
    lib = L.load()
    ev = _marker(_stats)
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        status = _points_status(dev)
        ws = torch.empty(int(lib.i2sdf_points_grid_workspace_bytes(R)), dtype=torch.uint8, device=dev)
        keys = torch.empty(R, dtype=torch.int64, device=dev)
        sref = torch.empty(R, 4, dtype=torch.float32, device=dev)
        fb = torch.empty(max(Q, 1), dtype=torch.int32, device=dev)
        ev("start")
        L.check(lib.i2sdf_points_grid_keys(L.ptr(r), R, L.ptr(ws), L.ptr(keys), L.ptr(status), st), "i2sdf_points_grid_keys")
        skeys, perm = torch.sort(keys, stable=True)            # stable: a cell's points stay in ascending index order
        del keys
        L.check(lib.i2sdf_points_grid_build(L.ptr(r), R, L.ptr(skeys), L.ptr(perm), L.ptr(ws), L.ptr(sref), st), "i2sdf_points_grid_build")
        ev("grid_build")
        if Q > 0:
            L.check(lib.i2sdf_points_nn_query(L.ptr(q), Q, L.ptr(sref), R, L.ptr(ws), _ring_budget(R), L.ptr(dist), L.ptr(index), L.ptr(fb),
                                              L.ptr(status), st), "i2sdf_points_nn_query")
            ev("nn_query")
            L.check(lib.i2sdf_points_nn_fallback(L.ptr(q), Q, L.ptr(r), R, L.ptr(fb), L.ptr(status), L.ptr(dist), L.ptr(index), st),
                    "i2sdf_points_nn_fallback")
            ev("nn_fallback")
        flags, n_fb = status.tolist()
        if _stats is not None:
            _stats.append(("fallback_count", n_fb))
        _raise_points_status(flags, "nearest_neighbors")
    return dist, index


@torch.no_grad()
def evaluate(pred, trgt, threshold: float = 0.05, down_sample: float = 0.02, _stats=None) -> dict:
    """`utils/mesh_util.py:evaluate` (model/eval/recon.py:111-129) on the device: both vertex sets are voxel down-sampled
    (a falsy `down_sample` skips that), nearest neighbours are found in both directions, and
        'Acc' = mean(dist2), 'Comp' = mean(dist1), 'Prec' = mean(dist2 < threshold), 'Recal' = mean(dist1 < threshold),
        'F-score' = 2 Prec Recal / (Prec + Recal)   (NaN when both are 0, as numpy gives it)
    come back as Python floats, where dist1 is the distance of each trgt point to its nearest pred point and dist2 that of each
    pred point to its nearest trgt point.  The means are fp64 sums in a fixed order, the counts integers; one download of the
    five numbers ends the call.
    `pred`, `trgt`: a Mesh / (verts, faces, ...) tuple or a bare (n, 3) fp32 device tensor; only vertices are used, as in the
    reference.  The function scores whatever vertex sets it is given: the reference first culls what no camera sees
    (mesh_util.refuse, a pyrender depth render re-fused into an open3d TSDF), which is not part of this library, so without that
    culling the numbers are not comparable with the paper's.  An empty set (after down-sampling) raises ValueError."""
    p = _points_arg(pred, "evaluate", "pred")
    t = _points_arg(trgt, "evaluate", "trgt")
    if p.device != t.device:
        raise ValueError("evaluate: pred and trgt must be on the same device")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("evaluate: threshold is NaN")
    if down_sample:
        p, _ = voxel_down_sample(p, down_sample, _stats=_stats)
        t, _ = voxel_down_sample(t, down_sample, _stats=_stats)
    if p.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError(f"evaluate: an empty point set ({p.shape[0]} pred, {t.shape[0]} trgt points)")
    dist1, _ = nearest_neighbors(t, p, _stats=_stats)
    dist2, _ = nearest_neighbors(p, t, _stats=_stats)
    lib = L.load()
    dev = p.device
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        sums = torch.empty(2, 2, dtype=torch.float64, device=dev)                  # rows: dist2 (pred), dist1 (trgt); (sum, count)
        for row, d in enumerate((dist2, dist1)):
            ws = torch.empty(int(lib.i2sdf_points_reduce_workspace_bytes(d.shape[0])), dtype=torch.uint8, device=dev)
            L.check(lib.i2sdf_points_threshold_reduce(L.ptr(d), d.shape[0], threshold, L.ptr(ws), L.ptr(sums[row]), st),
                    "i2sdf_points_threshold_reduce")
        # [[Acc, Prec], [Comp, Recal]]; the divisor is a tensor: a Python scalar would be turned into a multiplication by 1 / n
        m = sums / torch.tensor([[float(dist2.shape[0])], [float(dist1.shape[0])]], dtype=torch.float64, device=dev)
        f = 2.0 * m[0, 1] * m[1, 1] / (m[0, 1] + m[1, 1])
        acc, prec, comp, recal, fscore = torch.cat([m.reshape(-1), f.reshape(1)]).tolist()
    return {"Acc": acc, "Comp": comp, "Prec": prec, "Recal": recal, "F-score": fscore}
