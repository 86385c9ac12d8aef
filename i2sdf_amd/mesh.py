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
                       sets it is given; `score` first culls what no camera sees, as the reference does.
These are bitwise reproducible as well.

Visibility culling on the device (csrc/raster.hip, csrc/tsdf.hip), the step between the export and the scores
(model/eval/recon.py:111-125 -> utils/mesh_util.py:refuse, pyrender on EGL and open3d on the host in the reference):
  * mesh_depth         the depth render of every camera: fp64 edge functions, top-left rule, a 32-bit atomicMin per sample;
  * tsdf_integrate     open3d's ScalableTSDFVolume.integrate into 16^3-voxel units allocated where cameras touch them;
  * tsdf_extract       its extract_triangle_mesh by this module's marching cubes, across unit borders;
  * tsdf_fuse          the two together (the reference's depth2mesh); refuse = mesh_depth + tsdf_fuse; score = refuse, refuse, evaluate.
Bitwise reproducible too.  Neither open3d nor pyrender is available where this library is developed: the fusion rule and the depth
convention are restated from their sources and checked against a numpy restatement and closed-form geometry, not against them.  Not
imitated: OpenGL's 24-bit depth buffer (pyrender reads depth back through it: a relative error of about 6e-8 z / znear), open3d's
incremental fp32 accumulation of voxel coordinates, its table for ambiguous cells, its hash map's vertex order.  The scores are the
reference's up to those effects.

Ray casting on the device (csrc/bvh.hip, csrc/tri_isect.h), the ray caster on the extracted mesh the reference's `intersect_func` hook is
meant for, and shadow rays:
  * build_bvh           a linear BVH over the faces (Morton keys, one torch.sort, Karras' topology, boxes fitted bottom-up);
  * ray_mesh_intersect  the first face every ray meets, by the watertight rule of include/i2sdf.h ("Ray casting"): the smallest t, among
                        equal t the smallest face index, the same bits through the tree and through the brute-force route;
  * occluded            its any-hit form.
Bitwise reproducible; tests/raycast_ref.py restates the law in numpy.

Point-to-mesh queries on the device (csrc/closest.hip, csrc/tri_closest.h), what trimesh's `proximity` and open3d's
compute_closest_points / compute_signed_distance answer on the host, through the same tree:
  * closest_point       the closest point of the surface, its distance, face, weights and feature, by the fp64 rule of include/i2sdf.h
                        ("Closest point"): the smallest squared distance, among equal ones the smallest face index;
  * pseudonormals       the angle-weighted vertex and edge normals of the sign test (Baerentzen and Aanaes);
  * signed_distance     the distance with that sign: the quantity the implicit network approximates;
  * surface_scores      the five numbers of evaluate from surface samples to the other mesh's SURFACE, not to a vertex set.
Bitwise reproducible; tests/closest_ref.py restates the law in numpy.

Inside / outside for meshes that are open, cut or seen from one side (csrc/winding.hip, csrc/tri_solid_angle.h), through the same tree:
  * winding_number      the generalized winding number (include/i2sdf.h, "Winding number"): exact solid angles near, the far field of
                        Barill et al. 2018 (orders 0 and 1) for nodes farther than beta radii;
  * winding_moments     the far-field table of a tree, fitted bottom-up in a fixed order;
  * inside              |winding_number| > 0.5; signed_distance(sign="winding") takes its sign from it.
Each route bitwise reproducible; tests/winding_ref.py restates the law in numpy.

Between the producers and the consumers (csrc/simplify.hip, csrc/quadric.h; include/i2sdf.h, "Mesh simplification"):
  * simplify_vertex_clustering  vertex clustering on voxel_down_sample's grid with quadric placement (Lindstrom 2000; DeCoro and
                        Tatarchuk 2007): one wave per cell sums the corner quadrics in a fixed order and solves for the representative;
  * clean               bit-equal vertices merged, faces with a repeated index, of exactly zero area, or duplicated dropped;
  * topology            boundary / manifold / non-manifold / misoriented edges, the Euler number: is the mesh closed and oriented?
Bitwise reproducible; tests/simplify_ref.py restates the law in numpy.
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
    (mesh_util.refuse, a pyrender depth render re-fused into an open3d TSDF); `score` does that first (refuse, refuse, evaluate) and
    says how far its culling is the reference's.  An empty set (after down-sampling) raises ValueError."""
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


# ------------------------------------------------------------------- visibility culling (csrc/raster.hip, csrc/tsdf.hip)
class TsdfVolume(NamedTuple):
    """A block-sparse TSDF volume: 16^3-voxel units, allocated where a camera touched them, in ascending (ix, iy, iz) order."""
    tsdf: torch.Tensor       # (n_units, 4096) fp32; voxel (i, j, k) of a unit at i << 8 | j << 4 | k
    weight: torch.Tensor     # (n_units, 4096) fp32: the number of cameras that updated the voxel
    units: torch.Tensor      # (n_units, 3) int32 unit indices: a unit spans [index, index + 1) * 16 * voxel_length
    slot: torch.Tensor       # (dims) int32: the unit's row in tsdf / weight, -1 where there is none; cell [0, 0, 0] is unit `origin`
    origin: tuple            # lowest unit index per axis
    voxel_length: float
    sdf_trunc: float


def _f32(x):
    import ctypes as C
    return C.c_float(float(x)).value


def _intrinsics(K, what):
    """(fx, fy, cx, cy) of a 3x3 or 4x4 intrinsic matrix, read as utils/mesh_util.py:refuse reads them."""
    try:
        k = torch.as_tensor(K).detach().to("cpu", torch.float64)
    except Exception:
        raise ValueError(f"{what}: K must be a 3x3 or 4x4 matrix")
    if k.dim() != 2 or tuple(k.shape) not in ((3, 3), (4, 4)):
        raise ValueError(f"{what}: K must be a 3x3 or 4x4 matrix, got shape {tuple(k.shape)}")
    fx, fy, cx, cy = (_f32(k[0, 0]), _f32(k[1, 1]), _f32(k[0, 2]), _f32(k[1, 2]))
    if not (0.0 < fx < float("inf") and 0.0 < fy < float("inf") and abs(cx) < float("inf") and abs(cy) < float("inf")):
        raise ValueError(f"{what}: K needs finite fx, fy > 0 and finite cx, cy (got {fx}, {fy}, {cx}, {cy})")
    return fx, fy, cx, cy


def camera_matrices(poses):
    """(c2w, w2c): the (n_cam, 3, 4) fp32 CPU matrices the kernels read, from (n_cam, 4, 4) camera-to-world poses (any device, any
    floating dtype; x right, y down, z forward, last row 0 0 0 1).  The inverse is the fp64 adjugate formula, rounded to fp32 once.
    A pose that is not finite, not affine or not invertible raises ValueError."""
    if not torch.is_tensor(poses):
        try:
            poses = torch.as_tensor(poses)
        except Exception:
            raise ValueError("poses must be a (n_cam, 4, 4) tensor")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or not poses.dtype.is_floating_point:
        raise ValueError(f"poses must be a (n_cam, 4, 4) floating-point tensor, got {tuple(poses.shape)} {poses.dtype}")
    p = poses.detach().to("cpu", torch.float64)
    if p.shape[0] > 65535:
        raise ValueError("poses: at most 65535 cameras")
    if not bool(torch.isfinite(p).all()):
        raise ValueError("poses: a pose is not finite")
    if p.shape[0] and not bool((p[:, 3] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).all()):
        raise ValueError("poses: the last row of every pose must be (0, 0, 0, 1)")
    A, t = p[:, :3, :3], p[:, :3, 3]
    a, b, c = A[:, 0], A[:, 1], A[:, 2]                       # rows
    adj = torch.stack([torch.cross(b, c, dim=1), torch.cross(c, a, dim=1), torch.cross(a, b, dim=1)], dim=2)   # columns of the adjugate
    det = (a * torch.cross(b, c, dim=1)).sum(1)
    scale = A.abs().amax(dim=(1, 2)) ** 3 if p.shape[0] else det
    if p.shape[0] and not bool((det.abs() > 1e-12 * scale).all()):
        raise ValueError("poses: a pose is not invertible")
    inv = adj / det[:, None, None]
    tinv = -(inv @ t[:, :, None])
    w2c = torch.cat([inv, tinv], dim=2).to(torch.float32).contiguous()
    c2w = p[:, :3, :].to(torch.float32).contiguous()
    return c2w, w2c


def _image_size(H, W, what):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
        raise ValueError(f"{what}: H and W must be positive with H * W < 2^31 (got {H}, {W})")
    return H, W


def _k4(fx, fy, cx, cy):
    import ctypes as C
    return (C.c_float * 4)(fx, fy, cx, cy)


@torch.no_grad()
def mesh_depth(mesh, poses, K, H: int, W: int, znear: float = 0.05, zfar: float = 100.0, cull: str = "back", _stats=None) -> torch.Tensor:
    """Depth maps (n_cam, H, W) fp32 of a device mesh from pinhole cameras -- the pyrender depth render of utils/mesh_util.py:refuse.
    `poses` (n_cam, 4, 4) camera-to-world in the reference's convention (rend_util.load_K_Rt_from_P: x right, y down, z forward);
    `K` 3x3 or 4x4, read as refuse reads it (fx = K[0, 0], fy = K[1, 1], cx = K[0, 2], cy = K[1, 2]).
    depth[c, v, u] is the camera-space z of the nearest triangle crossed by the ray through ((u - cx) / fx, (v - cy) / fy, 1) -- the
    pixel pyrender's IntrinsicsCamera draws at column u, row v and the pixel open3d's integration reads back -- and 0 where there is
    none.  Samples (not triangles) with z outside [znear, zfar] give nothing (pyrender's default clip planes), so a triangle that
    crosses the camera plane still covers the pixels of its part in front.  cull="back" drops triangles whose winding is clockwise as
    the camera sees them (pyrender's default; the reference left SKIP_CULL_FACES commented out), cull="none" keeps both sides.  The
    marching-cubes meshes of this library have right-hand normals towards increasing SDF, so they face cameras in free space.
    Coverage is exact (fp64 edge functions, top-left rule) and the image is bitwise reproducible.  All depth maps stay resident on the
    device (n_cam H W 4 bytes); the projected vertices are held for a chunk of cameras at a time.
    Not imitated: OpenGL's 24-bit depth buffer, through which pyrender reads depth back (a relative error of about 6e-8 z / znear).
    The convention is restated from pyrender's sources, not checked against a build of it.  An empty mesh or camera list gives zeros /
    an empty tensor.  One host synchronisation reads the validation word."""
    verts, faces, _ = _mesh_args(mesh[:2], "mesh_depth")
    if cull not in ("back", "none"):
        raise ValueError(f"mesh_depth: cull must be 'back' or 'none', got {cull!r}")
    H, W = _image_size(H, W, "mesh_depth")
    k4 = _intrinsics(K, "mesh_depth")
    znear, zfar = float(znear), float(zfar)
    if not (0.0 < znear <= zfar < float("inf")):
        raise ValueError(f"mesh_depth: need 0 < znear <= zfar < inf (got {znear}, {zfar})")
    c2w, w2c = camera_matrices(poses)
    n_cam, V, F, dev = w2c.shape[0], verts.shape[0], faces.shape[0], verts.device
    if n_cam * H * W > (2 ** 31 - 1) * 256:
        raise ValueError("mesh_depth: too many pixels")
    depth = torch.empty(n_cam, H, W, dtype=torch.float32, device=dev)
    if n_cam == 0:
        return depth
    lib = L.load()
    ev = _marker(_stats)
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        ws = None
        if V and F:
            nbytes = int(lib.i2sdf_raster_workspace_bytes(V, F, n_cam))
            if nbytes <= 0:
                raise ValueError("mesh_depth: mesh size not supported")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counters = torch.empty(n_cam, 2, dtype=torch.int32, device=dev)
        status = _new_status(dev)
        w2c_d = w2c.to(dev)
        ev("start")
        L.check(lib.i2sdf_raster_depth(L.ptr(verts), V, L.ptr(faces), F, L.ptr(w2c_d), n_cam, _k4(*k4), H, W, znear, zfar,
                                       1 if cull == "back" else 0, L.ptr(ws), L.ptr(depth), L.ptr(counters), L.ptr(status), st),
                "i2sdf_raster_depth")
        ev("depth")
        if int(status.item()):
            raise _bad_faces("mesh_depth")
        if _stats is not None:
            _stats.append(("raster_counters", counters))
    return depth


def _tsdf_args(depths, poses, K, voxel_length, sdf_trunc, depth_trunc, stride, what):
    if not torch.is_tensor(depths) or not depths.is_cuda or depths.dtype != torch.float32 or depths.dim() != 3:
        raise ValueError(f"{what}: depths must be a (n_cam, H, W) fp32 tensor on a GPU")
    c2w, w2c = camera_matrices(poses)
    if c2w.shape[0] != depths.shape[0]:
        raise ValueError(f"{what}: {depths.shape[0]} depth maps for {c2w.shape[0]} poses")
    k4 = _intrinsics(K, what)
    voxel_length = float(voxel_length)
    sdf_trunc = 3.0 * voxel_length if sdf_trunc is None else float(sdf_trunc)
    depth_trunc, stride = float(depth_trunc), int(stride)
    inf = float("inf")
    if not (0.0 < _f32(voxel_length) < inf and 0.0 < _f32(sdf_trunc) < inf and depth_trunc > 0.0):
        raise ValueError(f"{what}: voxel_length, sdf_trunc and depth_trunc must be positive (and the first two finite)")
    if stride < 1:
        raise ValueError(f"{what}: depth_sampling_stride must be at least 1")
    if depths.shape[0] and (depths.shape[1] < 1 or depths.shape[2] < 1 or depths.shape[1] * depths.shape[2] > 2 ** 31 - 1):
        raise ValueError(f"{what}: depth maps of shape {tuple(depths.shape[1:])} are not supported")
    return depths.contiguous(), c2w, w2c, k4, voxel_length, sdf_trunc, min(depth_trunc, 3.0e38), stride


def _empty_volume(dev, voxel_length, sdf_trunc):
    z = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    return TsdfVolume(z(0, 4096), z(0, 4096), z(0, 3, dt=torch.int32), z(0, 0, 0, dt=torch.int32), (0, 0, 0), voxel_length, sdf_trunc)


@torch.no_grad()
def tsdf_integrate(depths: torch.Tensor, poses, K, voxel_length: float = 0.01, sdf_trunc: float = None, depth_trunc: float = 5.0,
                   depth_sampling_stride: int = 4, _stats=None) -> TsdfVolume:
    """Fuse device depth maps (n_cam, H, W) into a block-sparse TSDF volume: open3d's ScalableTSDFVolume.integrate for every camera
    in list order, with the rule written at the head of csrc/tsdf.hip (restated from open3d's sources, not checked against a build of
    it; open3d also accumulates voxel coordinates incrementally in fp32, which is not imitated).  `sdf_trunc` defaults to
    3 * voxel_length.  Memory grows with the units the cameras touch (32 KiB each), plus a table of 4-byte unit slots over their
    bounding box, which may hold at most 2^24 units: a larger extent raises I2SDFError.  Depth maps are read in place (all cameras
    resident).  Three host synchronisations: the bounding box of the touched units, their number, and the validation word."""
    depths, c2w, w2c, k4, vl, trunc, dtrunc, stride = _tsdf_args(depths, poses, K, voxel_length, sdf_trunc, depth_trunc,
                                                                 depth_sampling_stride, "tsdf_integrate")
    n_cam, H, W = depths.shape
    dev = depths.device
    if n_cam == 0:
        return _empty_volume(dev, vl, trunc)
    import ctypes as C
    lib = L.load()
    ev = _marker(_stats)
    ul = _f32(16.0 * _f32(vl))
    K4 = _k4(*k4)
    i32 = torch.int32
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        c2w_d, w2c_d = c2w.to(dev), w2c.to(dev)
        big = 2 ** 31 - 1
        bounds = torch.tensor([big, big, big, -big - 1, -big - 1, -big - 1, 0, 0], dtype=i32, device=dev)
        ev("start")
        L.check(lib.i2sdf_tsdf_bounds(L.ptr(depths), n_cam, H, W, L.ptr(c2w_d), K4, vl, ul, trunc, dtrunc, stride, L.ptr(bounds), st),
                "i2sdf_tsdf_bounds")
        b = bounds.tolist()
        if b[6]:
            raise L.I2SDFError("tsdf_integrate failed (-1): a back-projected point lies beyond 2^20 units of 16 voxels from the origin")
        if b[0] > b[3]:
            return _empty_volume(dev, vl, trunc)                  # no measurement in any depth map
        origin, dims = tuple(b[0:3]), tuple(b[3 + k] - b[k] + 1 for k in range(3))
        grid6 = (C.c_int32 * 6)(*origin, *dims)
        cells = int(lib.i2sdf_tsdf_table_cells(grid6))
        if cells <= 0:
            raise L.I2SDFError(f"tsdf_integrate failed (-1): the touched units span {dims[0]} x {dims[1]} x {dims[2]} units of 16 voxels; "
                               f"the unit table holds at most 2^24 cells (voxel_length too small for the extent)")
        stamp = torch.zeros(cells, dtype=i32, device=dev)
        flag = torch.zeros(1, dtype=i32, device=dev)
        L.check(lib.i2sdf_tsdf_mark(L.ptr(depths), n_cam, 0, H, W, L.ptr(c2w_d), K4, vl, ul, trunc, dtrunc, stride, grid6, None, 0,
                                    L.ptr(stamp), None, None, L.ptr(flag), st), "i2sdf_tsdf_mark")
        touched = stamp != 0
        incl = torch.cumsum(touched, 0, dtype=i32)
        slot = torch.where(touched, incl - 1, torch.full_like(incl, -1))
        unit_cell = torch.nonzero(touched).reshape(-1).to(i32)   # (synchronises: the number of units sizes the volume)
        n_units = unit_cell.shape[0]
        stamp.zero_()
        tsdf = torch.zeros(n_units, 4096, dtype=torch.float32, device=dev)
        weight = torch.zeros(n_units, 4096, dtype=torch.float32, device=dev)
        lst = torch.empty(n_units, dtype=i32, device=dev)
        counts = torch.zeros(n_cam, dtype=i32, device=dev)
        for c in range(n_cam):
            L.check(lib.i2sdf_tsdf_mark(L.ptr(depths), n_cam, c, H, W, L.ptr(c2w_d), K4, vl, ul, trunc, dtrunc, stride, grid6, L.ptr(slot),
                                        n_units, L.ptr(stamp), L.ptr(lst), L.ptr(counts[c:c + 1]), L.ptr(flag), st), "i2sdf_tsdf_mark")
            L.check(lib.i2sdf_tsdf_integrate(L.ptr(depths), n_cam, c, H, W, L.ptr(w2c_d), K4, vl, ul, trunc, dtrunc, grid6, L.ptr(unit_cell),
                                             n_units, L.ptr(lst), L.ptr(counts[c:c + 1]), L.ptr(tsdf), L.ptr(weight), st),
                    "i2sdf_tsdf_integrate")
        ev("mark_integrate")
        if int(flag.item()):
            raise L.I2SDFError("tsdf_integrate failed (-1): a touched unit lies outside the unit table")
        uc = unit_cell.to(torch.int64)
        units = torch.stack([uc // (dims[1] * dims[2]) + origin[0], uc // dims[2] % dims[1] + origin[1], uc % dims[2] + origin[2]], 1).to(i32)
        if _stats is not None:
            _stats.append(("touched_units", n_units))
    return TsdfVolume(tsdf, weight, units, slot.reshape(dims), origin, vl, trunc)


@torch.no_grad()
def tsdf_extract(volume: TsdfVolume, _stats=None) -> Mesh:
    """The zero-level mesh of a TsdfVolume -- open3d's extract_triangle_mesh by this library's marching cubes: cells of 8 neighbouring
    voxel centres, across unit borders; a cell counts only if its 8 voxels exist and have weight > 0; a corner is inside iff
    tsdf < 0; one vertex per crossing lattice edge of a counted cell, at the linear interpolation between the two voxel centres;
    faces wound so that the right-hand normal points towards positive tsdf (the side the cameras were on), with the fixed rule of
    csrc/gen_mc_tables.py for ambiguous cells in place of open3d's table.  `normals` are the normalised tsdf central-difference
    gradient (one-sided where a neighbour is missing), interpolated along the edge, and point towards positive tsdf as well.
    Vertices come in order of (unit, voxel, axis), not of a hash map.  One host synchronisation reads the two counts."""
    tsdf, weight, units, slot, origin, vl, _ = volume
    dev = tsdf.device
    n_units = tsdf.shape[0]
    empty = Mesh(torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                 torch.empty(0, 3, dtype=torch.float32, device=dev))
    if n_units == 0:
        return empty
    import ctypes as C
    lib = L.load()
    ev = _marker(_stats)
    dims = tuple(slot.shape)
    grid6 = (C.c_int32 * 6)(*origin, *dims)
    ul = _f32(16.0 * _f32(vl))
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        u = units.to(torch.int64)
        unit_cell = (((u[:, 0] - origin[0]) * dims[1] + (u[:, 1] - origin[1])) * dims[2] + (u[:, 2] - origin[2])).to(torch.int32)
        slot_f = slot.contiguous().reshape(-1)
        nbytes = int(lib.i2sdf_tsdf_extract_workspace_bytes(n_units))
        if nbytes <= 0 or int(lib.i2sdf_tsdf_table_cells(grid6)) != slot_f.shape[0]:
            raise ValueError("tsdf_extract: volume not supported")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        blocks = torch.empty(16 * n_units, 2, dtype=torch.int64, device=dev)
        ev("start")
        L.check(lib.i2sdf_tsdf_count(grid6, L.ptr(slot_f), L.ptr(unit_cell), n_units, L.ptr(tsdf), L.ptr(weight), L.ptr(ws), L.ptr(blocks), st),
                "i2sdf_tsdf_count")
        incl = torch.cumsum(blocks, 0)
        excl = (incl - blocks).contiguous()
        n_v, n_f = incl[-1].tolist()
        if max(n_v, n_f) > 2 ** 31 - 1:
            raise L.I2SDFError(f"tsdf_extract: {n_v} vertices / {n_f} faces do not fit int32 indices")
        if n_v == 0 or n_f == 0:
            return empty
        verts = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        normals = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
        L.check(lib.i2sdf_tsdf_emit(grid6, vl, ul, L.ptr(slot_f), L.ptr(unit_cell), n_units, L.ptr(tsdf), L.ptr(weight), L.ptr(ws), L.ptr(excl),
                                    L.ptr(verts), L.ptr(normals), L.ptr(faces), n_v, n_f, st), "i2sdf_tsdf_emit")
        ev("extract")
    return Mesh(verts, faces, normals)


@torch.no_grad()
def tsdf_fuse(depths: torch.Tensor, poses, K, voxel_length: float = 0.01, sdf_trunc: float = None, depth_trunc: float = 5.0,
              depth_sampling_stride: int = 4, _stats=None) -> Mesh:
    """tsdf_extract(tsdf_integrate(...)): device depth maps in, the fused surface out (verts, faces, normals on the device).  With
    the defaults this is utils/mesh_util.py:depth2mesh; refuse() feeds it rendered depth maps.  See the two functions for the rule
    and for how far it is open3d's."""
    vol = tsdf_integrate(depths, poses, K, voxel_length, sdf_trunc, depth_trunc, depth_sampling_stride, _stats=_stats)
    return tsdf_extract(vol, _stats=_stats)


@torch.no_grad()
def refuse(mesh, poses, K, H: int, W: int, far_clip: float = 5.0, _stats=None, **tsdf_kwargs) -> Mesh:
    """utils/mesh_util.py:refuse on the device: render the mesh's depth from every camera (mesh_depth), fuse the depth maps into a
    TSDF volume with depth_trunc = far_clip and extract its mesh (tsdf_fuse).  Nothing that no camera sees survives: the outer side
    of walls, the inside of furniture, whatever lies beyond far_clip.  `tsdf_kwargs`: voxel_length, sdf_trunc, depth_sampling_stride
    of tsdf_fuse and znear, zfar, cull of mesh_depth.  No mesh, depth map or volume leaves the device.
    The result is the reference's up to what mesh_depth, tsdf_integrate and tsdf_extract say they do not imitate (the 24-bit depth
    buffer, open3d's incremental fp32 voxel coordinates, its table for ambiguous cells, its vertex order); neither open3d nor pyrender
    was available to check the restated rules against."""
    render = {k: tsdf_kwargs.pop(k) for k in ("znear", "zfar", "cull") if k in tsdf_kwargs}
    bad = set(tsdf_kwargs) - {"voxel_length", "sdf_trunc", "depth_sampling_stride"}
    if bad:
        raise ValueError(f"refuse: unknown arguments {sorted(bad)}")
    depths = mesh_depth(mesh, poses, K, H, W, _stats=_stats, **render)
    return tsdf_fuse(depths, poses, K, depth_trunc=far_clip, _stats=_stats, **tsdf_kwargs)


@torch.no_grad()
def score(pred, trgt, poses, K, H: int, W: int, far_clip: float = 5.0, threshold: float = 0.05, down_sample: float = 0.02,
          **tsdf_kwargs) -> dict:
    """The three lines of model/eval/recon.py:111-125 on the device:
        mesh = refuse(pred, poses, K, H, W); gt_mesh = refuse(trgt, poses, K, H, W, far_clip); evaluate(mesh, gt_mesh)
    -- as in the reference, the prediction is refused with the default far_clip and the target with the given one.  Equal to
    evaluate(refuse(pred, ...), refuse(trgt, ..., far_clip), threshold, down_sample) exactly; `tsdf_kwargs` go to both refuse calls.
    The scores are the reference's up to the effects listed under refuse."""
    p = refuse(pred, poses, K, H, W, **dict(tsdf_kwargs))
    t = refuse(trgt, poses, K, H, W, far_clip, **dict(tsdf_kwargs))
    return evaluate(p, t, threshold=threshold, down_sample=down_sample)


# ---------------------------------------------------------------------------------------------------------------------------------
# Ray casting (csrc/bvh.hip; include/i2sdf.h, "Ray casting", states the law)
class MeshBVH(NamedTuple):
    """A linear BVH over the faces of a device mesh (build_bvh).  It refers to the mesh's tensors: they must stay as they are."""
    verts: torch.Tensor      # (V, 3) fp32
    faces: torch.Tensor      # (F, 3) int32
    buffer: torch.Tensor     # i2sdf_bvh_bytes(F) uint8: header, nodes, leaves, build links


class RayHits(NamedTuple):
    t: torch.Tensor          # (n,) fp32, in units of the direction; t_max on a miss
    face: torch.Tensor       # (n,) int32, -1 on a miss
    bary: torch.Tensor       # (n, 2) fp32: the weights of the face's first and second vertex; 0 on a miss
    hit: torch.Tensor        # (n,) bool
    status: torch.Tensor     # (1,) int32 on the device: lib.RAYCAST_BAD_RAY | lib.RAYCAST_BAD_FACE over the call (not read back here)


RAYCAST_ROUTES = ("auto", "bvh", "brute")
RAYCAST_BRUTE_MAX_FACES = 256      # route="auto" on a bare mesh: at most one staged tile of faces per ray goes without a tree


def _raycast_mesh(mesh, what, cpu_ok=False):
    if isinstance(mesh, MeshBVH):
        return mesh
    if not isinstance(mesh, (tuple, list)) or len(mesh) < 2:
        raise ValueError(f"{what}: expected a Mesh, a (verts, faces) pair or a MeshBVH, got {type(mesh).__name__}")
    for t, dt, name in ((mesh[0], torch.float32, "verts"), (mesh[1], torch.int32, "faces")):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be a (n, 3) {dt} tensor")
    if mesh[0].device != mesh[1].device:
        raise ValueError(f"{what}: verts on {mesh[0].device}, faces on {mesh[1].device}")
    if not mesh[0].is_cuda and not cpu_ok:
        raise L.I2SDFError(f"{what}: the mesh is on {mesh[0].device}; ray casting runs on the GPU only, there is no CPU path")
    return mesh[0].contiguous(), mesh[1].contiguous()


@torch.no_grad()
def build_bvh(mesh) -> MeshBVH:
    """The BVH of a device mesh (a Mesh or a (verts, faces) pair; F = 0 is legal): Morton keys of the face centroids, one torch.sort,
    Karras' topology, boxes fitted bottom-up.  Enqueues only; 124 bytes per face stay allocated with the result."""
    m = _raycast_mesh(mesh, "build_bvh")
    if isinstance(m, MeshBVH):
        return m
    verts, faces = m
    lib = L.load()
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    with torch.cuda.device(dev):
        nbytes = int(lib.i2sdf_bvh_bytes(F))
        if nbytes <= 0:
            raise ValueError(f"build_bvh: {F} faces are more than the {L.BVH_MAX_FACES} a tree holds")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        keys = torch.empty(F, dtype=torch.int64, device=dev)
        st = L.stream_ptr()
        L.check(lib.i2sdf_bvh_keys(L.ptr(verts), V, L.ptr(faces), F, L.ptr(buf), L.ptr(keys), st), "i2sdf_bvh_keys")
        skeys = torch.sort(keys, stable=True)[0]              # (unique keys; the face index rides in their low word)
        L.check(lib.i2sdf_bvh_build(L.ptr(verts), V, L.ptr(faces), F, L.ptr(skeys), L.ptr(buf), st), "i2sdf_bvh_build")
    return MeshBVH(verts, faces, buf)


def _ray_args(origins, dirs, t_min, t_max, dev, what):
    for name, t in (("origins", origins), ("dirs", dirs)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or not t.dtype.is_floating_point:
            raise ValueError(f"{what}: {name} must be a (n, 3) floating-point tensor")
    if dirs.shape != origins.shape:
        raise ValueError(f"{what}: origins {tuple(origins.shape)} and dirs {tuple(dirs.shape)} differ")
    n = origins.shape[0]
    if origins.device != dev or dirs.device != dev:
        raise ValueError(f"{what}: the rays are on {origins.device} / {dirs.device}, the mesh on {dev}")
    bounds = []
    for name, b in (("t_min", t_min), ("t_max", t_max)):
        if torch.is_tensor(b):
            if tuple(b.shape) != (n,) or not b.dtype.is_floating_point or b.device != dev:
                raise ValueError(f"{what}: {name} must be a number or a ({n},) floating-point tensor on {dev}")
            bounds.append(b.detach().to(torch.float32).contiguous())
        elif isinstance(b, (int, float)) and not isinstance(b, bool):
            bounds.append(torch.full((n,), float(b), dtype=torch.float32, device=dev))
        else:
            raise TypeError(f"{what}: {name} must be a number or an ({n},) tensor, got {type(b).__name__}")
    c = lambda t: t.detach().to(torch.float32).contiguous()
    return c(origins), c(dirs), bounds[0], bounds[1]


@torch.no_grad()
def ray_mesh_intersect(bvh_or_mesh, origins, dirs, t_min=0.0, t_max=float("inf"), cull: str = "none", any_hit: bool = False,
                       route: str = "auto") -> RayHits:
    """The first face every ray o + t d meets with t_min < t <= t_max (numbers or per-ray tensors), by the watertight rule of
    include/i2sdf.h: the smallest t, among equal t the smallest face index -- the same bits by every route.  Directions need not be
    unit; t is in units of `dirs`.  cull="back" ignores faces whose right-hand normal points along the ray (mesh_depth's back faces).
    any_hit=True fills only `hit` (t, face, bary are None); it equals the closest-hit flag.
    route: "bvh" (a bare mesh gets its tree built first), "brute" (every ray against every face: the reference route), "auto" (the
    tree when one is given or the mesh has more than RAYCAST_BRUTE_MAX_FACES faces).  Enqueues only."""
    what = "ray_mesh_intersect"
    if cull not in L.RAYCAST_CULL:
        raise ValueError(f"{what}: cull = {cull!r} is none of {sorted(L.RAYCAST_CULL)}")
    if route not in RAYCAST_ROUTES:
        raise ValueError(f"{what}: route = {route!r} is none of {list(RAYCAST_ROUTES)}")
    m = _raycast_mesh(bvh_or_mesh, what)
    verts, faces = m[0], m[1]
    dev = verts.device
    o, d, t0, t1 = _ray_args(origins, dirs, t_min, t_max, dev, what)
    if not verts.is_cuda:
        raise L.I2SDFError(f"{what}: the mesh is on {dev}; ray casting runs on the GPU only, there is no CPU path")
    lib = L.load()
    n, V, F = o.shape[0], verts.shape[0], faces.shape[0]
    if route == "auto":
        route = "bvh" if isinstance(m, MeshBVH) or F > RAYCAST_BRUTE_MAX_FACES else "brute"
    if route == "bvh" and not isinstance(m, MeshBVH):
        m = build_bvh(m)
    with torch.cuda.device(dev):
        hit = torch.empty(n, dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        t = face = bary = None
        if not any_hit:
            t = torch.empty(n, dtype=torch.float32, device=dev)
            face = torch.empty(n, dtype=torch.int32, device=dev)
            bary = torch.empty(n, 2, dtype=torch.float32, device=dev)
        out = (L.ptr(t), L.ptr(face), L.ptr(bary), L.ptr(hit), L.ptr(status), L.stream_ptr())
        flags = (n, L.RAYCAST_CULL[cull], int(bool(any_hit)))
        if route == "bvh":
            L.check(lib.i2sdf_bvh_trace(L.ptr(m.buffer), F, L.ptr(o), L.ptr(d), L.ptr(t0), L.ptr(t1), *flags, *out), "i2sdf_bvh_trace")
        else:
            L.check(lib.i2sdf_mesh_trace_brute(L.ptr(verts), V, L.ptr(faces), F, L.ptr(o), L.ptr(d), L.ptr(t0), L.ptr(t1), *flags, *out),
                    "i2sdf_mesh_trace_brute")
    return RayHits(t, face, bary, hit.view(torch.bool), status)


def occluded(bvh_or_mesh, origins, dirs, t_min=0.0, t_max=float("inf"), cull: str = "none", route: str = "auto") -> torch.Tensor:
    """(n,) bool: is anything met with t_min < t <= t_max -- a shadow ray.  ray_mesh_intersect(..., any_hit=True).hit."""
    return ray_mesh_intersect(bvh_or_mesh, origins, dirs, t_min, t_max, cull, True, route).hit


# ---------------------------------------------------------------------------------------------------------------------------------
# Closest point (csrc/closest.hip; include/i2sdf.h, "Closest point", states the law)
class ClosestPoints(NamedTuple):
    dist: torch.Tensor       # (n,) fp32; +inf on a miss
    point: torch.Tensor      # (n, 3) fp32: the closest point of the mesh; 0 on a miss
    face: torch.Tensor       # (n,) int32, -1 on a miss
    bary: torch.Tensor       # (n, 2) fp32: the weights of the face's first and second vertex; 0 on a miss
    feature: torch.Tensor    # (n,) uint8: lib.CLOSEST_FEATURES; 0 on a miss
    sdist: torch.Tensor      # (n,) fp32: dist with the pseudonormal sign (negative inside); None without normals
    status: torch.Tensor     # (1,) int32 on the device: lib.CLOSEST_BAD_POINT | lib.CLOSEST_BAD_FACE over the call (not read back here)


class MeshNormals(NamedTuple):
    """The angle-weighted pseudonormals of a mesh (pseudonormals): not normalised, only their direction is used."""
    vertex: torch.Tensor     # (V, 3) fp32
    edge: torch.Tensor       # (F, 3, 3) fp32: [face][AB, BC, CA]


# route="auto" on a bare mesh.  profiles/closest_timing.json, 512 queries: brute 0.053 ms against build + tree 0.103 ms at 64 faces,
# 0.165 against 0.135 at 256 -- the lines cross near 180 faces; the tree alone wins from 64 faces on (0.041 ms)
CLOSEST_BRUTE_MAX_FACES = 128


def _query_points(points, dev, what):
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{what}: points must be a (n, 3) fp32 tensor")
    if points.device != dev:
        raise ValueError(f"{what}: the points are on {points.device}, the mesh on {dev}")
    if points.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{what}: points must hold at most 2^31 - 1 points")
    return points.detach().contiguous()


def _normals_arg(normals, V, F, dev, what):
    if normals is None:
        return None
    if not isinstance(normals, (tuple, list)) or len(normals) != 2:
        raise ValueError(f"{what}: normals must be a MeshNormals (pseudonormals(mesh))")
    for t, shape, name in ((normals[0], (V, 3), "vertex"), (normals[1], (F, 3, 3), "edge")):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{what}: normals.{name} must be a {shape} fp32 tensor on {dev}")
    return MeshNormals(normals[0].contiguous(), normals[1].contiguous())


@torch.no_grad()
def pseudonormals(mesh) -> MeshNormals:
    """The tables of the sign test of closest_point: per vertex the sum of angle x unit face normal over the corners there, per
    (face, edge) the sum of the unit normals of all faces on that edge -- fp64 sums in ascending face order, rounded to fp32 once
    (include/i2sdf.h, "Closest point").  Corners and half-edges are grouped by two stable torch.sort calls; no floating-point
    atomics, so the tables are bitwise reproducible.  Accepts a Mesh, a (verts, faces) pair or a MeshBVH.  Enqueues only."""
    m = _raycast_mesh(mesh, "pseudonormals", cpu_ok=True)
    verts, faces = m[0], m[1]
    if not verts.is_cuda:
        raise L.I2SDFError(f"pseudonormals: the mesh is on {verts.device}; the tables are built on the GPU only, there is no CPU path")
    lib = L.load()
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    if F > L.BVH_MAX_FACES:
        raise ValueError(f"pseudonormals: {F} faces are more than the {L.BVH_MAX_FACES} supported")
    with torch.cuda.device(dev):
        vn = torch.empty(V, 3, dtype=torch.float32, device=dev)
        en = torch.empty(F, 3, 3, dtype=torch.float32, device=dev)
        keys = torch.empty(6 * F, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        st = L.stream_ptr()
        L.check(lib.i2sdf_closest_normal_keys(L.ptr(verts), V, L.ptr(faces), F, L.ptr(keys), L.ptr(status), st), "i2sdf_closest_normal_keys")
        ck, cp = torch.sort(keys[:3 * F], stable=True)           # stable: a run stays in ascending corner, hence face, order
        ek, ep = torch.sort(keys[3 * F:], stable=True)
        skeys, perm = torch.cat([ck, ek]), torch.cat([cp, ep])
        L.check(lib.i2sdf_closest_normals(L.ptr(verts), V, L.ptr(faces), F, L.ptr(skeys), L.ptr(perm), L.ptr(vn), L.ptr(en), st),
                "i2sdf_closest_normals")
    return MeshNormals(vn, en)


@torch.no_grad()
def closest_point(bvh_or_mesh, points, max_dist: float = float("inf"), normals=None, route: str = "auto") -> ClosestPoints:
    """The point of the mesh closest to every query point within `max_dist`, by the fp64 rule of include/i2sdf.h ("Closest point"):
    the smallest squared distance, among equal ones the smallest face index -- the same bits by every route.  `feature` says whether
    it lies inside the face, on one of its edges or at one of its vertices.  With normals=pseudonormals(mesh), `sdist` carries the
    inside (-) / outside (+) sign of the angle-weighted pseudonormal test; it means something only on a closed, consistently
    oriented mesh.  A point farther than max_dist from every face (or with a non-finite coordinate) is a miss: face -1, dist +inf.
    route: "bvh" (a bare mesh gets its tree built first), "brute" (every point against every face: the reference route), "auto" (the
    tree when one is given or the mesh has more than CLOSEST_BRUTE_MAX_FACES faces).  Enqueues only."""
    what = "closest_point"
    if route not in RAYCAST_ROUTES:
        raise ValueError(f"{what}: route = {route!r} is none of {list(RAYCAST_ROUTES)}")
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise ValueError(f"{what}: max_dist = {max_dist} must be >= 0 (inf allowed)")
    m = _raycast_mesh(bvh_or_mesh, what, cpu_ok=True)
    verts, faces = m[0], m[1]
    dev = verts.device
    p = _query_points(points, dev, what)
    n, V, F = p.shape[0], verts.shape[0], faces.shape[0]
    nm = _normals_arg(normals, V, F, dev, what)
    if not verts.is_cuda:
        raise L.I2SDFError(f"{what}: the mesh is on {dev}; closest-point queries run on the GPU only, there is no CPU path")
    lib = L.load()
    if route == "auto":
        route = "bvh" if isinstance(m, MeshBVH) or F > CLOSEST_BRUTE_MAX_FACES else "brute"
    if route == "bvh" and not isinstance(m, MeshBVH):
        m = build_bvh(m)
    with torch.cuda.device(dev):
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        point = torch.empty(n, 3, dtype=torch.float32, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev)
        bary = torch.empty(n, 2, dtype=torch.float32, device=dev)
        feature = torch.empty(n, dtype=torch.uint8, device=dev)
        sdist = torch.empty(n, dtype=torch.float32, device=dev) if nm is not None else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        # (an empty tensor has no address: the tables of an empty mesh and the outputs of an empty query are never touched)
        one = torch.empty(1, dtype=torch.float32, device=dev)
        tab = (None, None) if nm is None else tuple(L.ptr(t) if t.numel() else L.ptr(one) for t in nm)
        sd = None if nm is None else (L.ptr(sdist) if n else L.ptr(one))
        args = (L.ptr(p), n, max_dist, *tab, L.ptr(dist), L.ptr(point), L.ptr(face), L.ptr(bary), L.ptr(feature), sd, L.ptr(status),
                L.stream_ptr())
        if route == "bvh":
            L.check(lib.i2sdf_closest_bvh(L.ptr(m.buffer), L.ptr(verts), V, L.ptr(faces), F, *args), "i2sdf_closest_bvh")
        else:
            L.check(lib.i2sdf_closest_brute(L.ptr(verts), V, L.ptr(faces), F, *args), "i2sdf_closest_brute")
    return ClosestPoints(dist, point, face, bary, feature, sdist, status)


SIGNED_DISTANCE_SIGNS = ("pseudonormal", "winding")


def signed_distance(bvh_or_mesh, points, normals=None, max_dist: float = float("inf"), sign: str = "pseudonormal", beta: float = 2.0,
                    moments=None) -> torch.Tensor:
    """(n,) fp32: the distance to the mesh, negative inside -- the quantity the implicit network approximates, at the same points.
    sign="pseudonormal" (the default): builds the pseudonormal tables when they are not given (keep them, and a MeshBVH, when asking
    more than once); that sign means something only on a closed, consistently oriented mesh.  sign="winding": the distance of
    closest_point, negative where `inside` (|winding_number| > 0.5, with `beta` and `moments`) -- also on open, cut or one-sided
    meshes; `normals` is not used.  +inf beyond max_dist either way."""
    if sign not in SIGNED_DISTANCE_SIGNS:
        raise ValueError(f"signed_distance: sign = {sign!r} is none of {list(SIGNED_DISTANCE_SIGNS)}")
    if sign == "winding":
        if not isinstance(bvh_or_mesh, MeshBVH) and _raycast_mesh(bvh_or_mesh, "signed_distance", cpu_ok=True)[0].is_cuda:
            bvh_or_mesh = build_bvh(bvh_or_mesh)              # (one tree for both queries; a CPU mesh is refused by closest_point)
        dist = closest_point(bvh_or_mesh, points, max_dist).dist
        return torch.where(inside(bvh_or_mesh, points, beta, moments) & torch.isfinite(dist), -dist, dist)
    if normals is None:
        normals = pseudonormals(bvh_or_mesh)
    return closest_point(bvh_or_mesh, points, max_dist, normals).sdist


# ---------------------------------------------------------------------------------------------------------------------------------
# Winding number (csrc/winding.hip; include/i2sdf.h, "Winding number", states the law)
class WindingMoments(NamedTuple):
    """The far-field table of a MeshBVH (winding_moments): per internal node the area-weighted centroid, a radius, and the moments
    N0, N1 of the faces below it.  It belongs to that tree."""
    buffer: torch.Tensor     # i2sdf_winding_moments_bytes(F) uint8: 16 fp64 per internal node (p~[3], r, N0[3], N1[9]), then the build's counters
    n_faces: int

    @property
    def table(self) -> torch.Tensor:
        """(F - 1, 16) fp64: a view of the records"""
        k = max(self.n_faces - 1, 0)
        return self.buffer[:128 * k].view(torch.float64).view(k, 16)


# route="auto" on a bare mesh.  Not closest_point's 128: a winding sum prunes nothing near the mesh, so the tree pays off later.
# profiles/winding_timing.json, 512 queries inside a soup: brute 0.072 ms against the two builds + tree 0.29 ms at 128 faces, 0.52 against
# 0.99 at 1024 (0.84 for a tree already built), 2.04 against 2.15 at 4096 (1.95): the lines cross near 4096 faces
WINDING_BRUTE_MAX_FACES = 1024


@torch.no_grad()
def winding_moments(bvh: MeshBVH) -> WindingMoments:
    """The far-field table of a tree (include/i2sdf.h, "Winding number"): one bottom-up pass over the tree's parent links, a parent
    being child 0 + child 1 in that order, so the table is bitwise reproducible.  128 bytes per face stay allocated with the result;
    the tree is only read.  Enqueues only."""
    if not isinstance(bvh, MeshBVH):
        raise ValueError(f"winding_moments: expected a MeshBVH (build_bvh), got {type(bvh).__name__}")
    lib = L.load()
    F, dev = bvh.faces.shape[0], bvh.buffer.device
    with torch.cuda.device(dev):
        buf = torch.empty(int(lib.i2sdf_winding_moments_bytes(F)), dtype=torch.uint8, device=dev)
        L.check(lib.i2sdf_winding_moments(L.ptr(bvh.buffer), F, L.ptr(buf), L.stream_ptr()), "i2sdf_winding_moments")
    return WindingMoments(buf, F)


@torch.no_grad()
def winding_number(bvh_or_mesh, points, beta: float = 2.0, moments=None, route: str = "auto") -> torch.Tensor:
    """(n,) fp64: the generalized winding number of the mesh at every point, by the law of include/i2sdf.h ("Winding number"): 1 inside
    a closed mesh with outward right-hand normals, 0 outside, and a smooth function of the point on open sheets, cut level sets and
    soups, where closest_point's sign means nothing.  NaN at a point with a non-finite coordinate.
    route: "bvh" walks the tree and takes a node's far field (orders 0 and 1 of Barill et al. 2018) when the point is farther than
    beta radii from it -- beta=float("inf") is the exact sum in tree order; a bare mesh gets its tree built first, and `moments`
    (winding_moments(bvh): keep it when asking more than once) is built when not given.  "brute": the exact sum in ascending face
    order, the reference route.  "auto": the tree when one is given or the mesh has more than WINDING_BRUTE_MAX_FACES faces.
    Each route is bitwise reproducible; the two differ by rounding (and by the far field for a finite beta).  Enqueues only."""
    what = "winding_number"
    if route not in RAYCAST_ROUTES:
        raise ValueError(f"{what}: route = {route!r} is none of {list(RAYCAST_ROUTES)}")
    beta = float(beta)
    if not beta >= 0.0:
        raise ValueError(f"{what}: beta = {beta} must be >= 0 (inf allowed)")
    m = _raycast_mesh(bvh_or_mesh, what, cpu_ok=True)
    verts, faces = m[0], m[1]
    dev = verts.device
    p = _query_points(points, dev, what)
    n, V, F = p.shape[0], verts.shape[0], faces.shape[0]
    if moments is not None and (not isinstance(moments, WindingMoments) or not isinstance(m, MeshBVH) or moments.n_faces != F
                                or moments.buffer.device != dev):
        raise ValueError(f"{what}: moments must be the WindingMoments of the MeshBVH that is passed (winding_moments(bvh))")
    if not verts.is_cuda:
        raise L.I2SDFError(f"{what}: the mesh is on {dev}; winding numbers are summed on the GPU only, there is no CPU path")
    lib = L.load()
    if route == "auto":
        route = "bvh" if isinstance(m, MeshBVH) or F > WINDING_BRUTE_MAX_FACES else "brute"
    if route == "bvh":
        if not isinstance(m, MeshBVH):
            m = build_bvh(m)
        if moments is None:
            moments = winding_moments(m)
    with torch.cuda.device(dev):
        w = torch.empty(n, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        if route == "bvh":
            L.check(lib.i2sdf_winding_bvh(L.ptr(m.buffer), L.ptr(moments.buffer), F, L.ptr(p), n, beta, L.ptr(w), L.ptr(status),
                                          L.stream_ptr()), "i2sdf_winding_bvh")
        else:
            L.check(lib.i2sdf_winding_brute(L.ptr(verts), V, L.ptr(faces), F, L.ptr(p), n, L.ptr(w), L.ptr(status), L.stream_ptr()),
                    "i2sdf_winding_brute")
    return w


def inside(bvh_or_mesh, points, beta: float = 2.0, moments=None, route: str = "auto") -> torch.Tensor:
    """(n,) bool: |winding_number| > 0.5 -- false at a point with a non-finite coordinate."""
    return winding_number(bvh_or_mesh, points, beta, moments, route).abs() > 0.5


@torch.no_grad()
def surface_scores(pred, trgt, n_samples: int, threshold: float = 0.05, draws=None, generator=None) -> dict:
    """The five numbers of `evaluate`, taken from surface to surface instead of from vertex set to vertex set: `n_samples`
    area-weighted samples of each mesh (sample_surface) against the closest point of the OTHER mesh's surface,
        'Acc' = mean(d(pred samples -> trgt)), 'Comp' = mean(d(trgt samples -> pred)), 'Prec' = mean(Acc distances < threshold),
        'Recal' = mean(Comp distances < threshold), 'F-score' = 2 Prec Recal / (Prec + Recal).
    The means are fp64 sums in a fixed order, as in evaluate.  pred, trgt: a Mesh, a (verts, faces) pair or a MeshBVH (its tree is
    used).  draws: {"pred": {...}, "trgt": {...}} of sample_surface draws; missing ones come from torch.rand with `generator`.
    The values are 0-d fp64 device tensors: nothing is read back here (so face indices are not validated: a bad one shows as
    CLOSEST_BAD_FACE does in closest_point, and its face is never drawn closest).  evaluate is unchanged."""
    what = "surface_scores"
    meshes = [_raycast_mesh(pred, what, cpu_ok=True), _raycast_mesh(trgt, what, cpu_ok=True)]      # (both shapes before any device)
    if meshes[0][0].device != meshes[1][0].device:
        raise ValueError(f"{what}: pred and trgt must be on the same device")
    if not meshes[0][0].is_cuda:
        raise L.I2SDFError(f"{what}: the meshes are on {meshes[0][0].device}; scoring runs on the GPU only, there is no CPU path")
    n_samples, threshold = int(n_samples), float(threshold)
    if n_samples <= 0:
        raise ValueError(f"{what}: n_samples must be positive")
    if threshold != threshold:
        raise ValueError(f"{what}: threshold is NaN")
    for m, name in zip(meshes, ("pred", "trgt")):
        if m[1].shape[0] == 0:
            raise ValueError(f"{what}: {name} has no faces")
    draws = draws or {}
    trees = [build_bvh(m) for m in meshes]
    samples = [sample_surface((m[0], m[1]), n_samples, draws.get(name), generator, _check=False)[0]
               for m, name in zip(meshes, ("pred", "trgt"))]
    dist2 = closest_point(trees[1], samples[0]).dist          # pred samples -> trgt surface
    dist1 = closest_point(trees[0], samples[1]).dist          # trgt samples -> pred surface
    lib = L.load()
    dev = dist1.device
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        sums = torch.empty(2, 2, dtype=torch.float64, device=dev)                  # rows: dist2 (pred), dist1 (trgt); (sum, count)
        for row, d in enumerate((dist2, dist1)):
            ws = torch.empty(int(lib.i2sdf_points_reduce_workspace_bytes(d.shape[0])), dtype=torch.uint8, device=dev)
            L.check(lib.i2sdf_points_threshold_reduce(L.ptr(d), d.shape[0], threshold, L.ptr(ws), L.ptr(sums[row]), st),
                    "i2sdf_points_threshold_reduce")
        m = sums / torch.tensor([[float(n_samples)]], dtype=torch.float64, device=dev)
        f = 2.0 * m[0, 1] * m[1, 1] / (m[0, 1] + m[1, 1])
    return {"Acc": m[0, 0], "Comp": m[1, 0], "Prec": m[0, 1], "Recal": m[1, 1], "F-score": f}


# ---------------------------------------------------------------------------------------------------------------------------------
# Simplification, cleaning, topology (csrc/simplify.hip, csrc/quadric.h; include/i2sdf.h, "Mesh simplification", states the law)
class SimplifyResult(NamedTuple):
    mesh: Mesh               # normals None when the input had none
    vertex_map: torch.Tensor  # (V,) int32: input vertex -> output vertex, -1 when its cell is referenced by no surviving face
    face_map: torch.Tensor   # (F_out,) int32: output face -> input face
    fallback: torch.Tensor   # (V_out,) bool: the quadric minimiser was not used (it left the cell, or there was no quadric): the mean


class CleanResult(NamedTuple):
    mesh: Mesh
    vertex_map: torch.Tensor  # (V,) int32: input vertex -> output vertex, -1 when no kept face references it
    face_map: torch.Tensor   # (F_out,) int32: output face -> input face


class MeshTopology:
    """The edge statistics of a mesh (topology): `counts` is a (lib.TOPO_COUNTS,) int64 device tensor indexed by lib.TOPO; nothing is
    read back until as_dict() (or one of the properties) asks, and then once."""

    def __init__(self, counts: torch.Tensor, status: torch.Tensor):
        self.counts, self.status = counts, status
        self._host = None

    def as_dict(self) -> dict:
        if self._host is None:
            c = torch.cat([self.counts, self.status.to(torch.int64)]).tolist()
            if c[-1]:
                raise _bad_faces("topology")
            t = L.TOPO
            self._host = {"edges": c[t["EDGES"]], "boundary_edges": c[t["BOUNDARY"]], "manifold_edges": c[t["MANIFOLD"]],
                          "nonmanifold_edges": c[t["NONMANIFOLD"]], "misoriented_edges": c[t["MISORIENTED"]],
                          "repeated_index_faces": c[t["REPEATED_FACES"]], "referenced_vertices": c[t["VERTICES"]], "faces": c[t["FACES"]],
                          "euler": c[t["EULER"]]}
        return dict(self._host)

    @property
    def watertight(self) -> bool:
        """no boundary edge and no non-manifold edge (an empty mesh is watertight by this rule)"""
        d = self.as_dict()
        return d["boundary_edges"] == 0 and d["nonmanifold_edges"] == 0

    @property
    def oriented(self) -> bool:
        """no 2-face edge that both faces traverse in the same direction"""
        return self.as_dict()["misoriented_edges"] == 0

    def __repr__(self):
        return f"MeshTopology({self.as_dict()})"


def _simplify_mesh(mesh, what):
    """(verts, faces, normals or None) of a Mesh / (verts, faces[, normals]) on one GPU; a CPU mesh is refused by name"""
    if not isinstance(mesh, (tuple, list)) or isinstance(mesh, MeshBVH) or len(mesh) < 2:
        raise ValueError(f"{what}: expected a Mesh or a (verts, faces[, normals]) tuple, got {type(mesh).__name__}")
    normals = mesh[2] if len(mesh) > 2 else None
    for t, dt, name in ((mesh[0], torch.float32, "verts"), (mesh[1], torch.int32, "faces"), (normals, torch.float32, "normals")):
        if t is None and name == "normals":
            continue
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be a (n, 3) {dt} tensor")
        if t.device != mesh[0].device:
            raise ValueError(f"{what}: verts on {mesh[0].device}, {name} on {t.device}")
    if normals is not None and normals.shape[0] != mesh[0].shape[0]:
        raise ValueError(f"{what}: {normals.shape[0]} normals for {mesh[0].shape[0]} vertices")
    if mesh[0].shape[0] > 2 ** 31 - 1 or mesh[1].shape[0] > (2 ** 31 - 1) // 3:
        raise ValueError(f"{what}: at most 2^31 - 1 vertices and (2^31 - 1) / 3 faces")
    if not mesh[0].is_cuda:
        raise L.I2SDFError(f"{what}: the mesh is on {mesh[0].device}; it runs on the GPU only, there is no CPU path")
    return mesh[0].contiguous(), mesh[1].contiguous(), None if normals is None else normals.contiguous()


def _sort_pairs(hi, lo):
    """stable lexicographic sort of (hi, lo) -> (sorted hi, sorted lo, perm): two stable sorts, the minor key first"""
    slo, p1 = torch.sort(lo, stable=True)
    shi, p2 = torch.sort(hi[p1], stable=True)
    return shi, slo[p2], p1[p2]


def _keep_and_compact(src_verts, src_normals, mapped, hi, lo, duplicated, status, what, ev=lambda label: None):
    """the kept faces of `mapped` (F, 3) over the table src_verts, compacted -> (Mesh, vflag, vscan, face_map)"""
    lib = L.load()
    F, n_src, dev = mapped.shape[0], src_verts.shape[0], mapped.device
    st = L.stream_ptr()
    if duplicated and F:
        shi, slo, perm = _sort_pairs(hi, lo)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)
        L.check(lib.i2sdf_simplify_run_heads(L.ptr(shi), L.ptr(slo), L.ptr(perm), F, L.ptr(keep), None, st), "i2sdf_simplify_run_heads")
    else:
        keep = ((hi != 2 ** 63 - 1) | (lo != 2 ** 63 - 1)).to(torch.uint8)
    ev("faces")
    fkeep = torch.empty(F, dtype=torch.int32, device=dev)
    vflag = torch.empty(n_src, dtype=torch.int32, device=dev)
    mstatus = _new_status(dev)
    L.check(lib.i2sdf_mesh_compact_mark(L.ptr(mapped), L.ptr(keep), F, n_src, L.ptr(fkeep), L.ptr(vflag), L.ptr(mstatus), st),
            "i2sdf_mesh_compact_mark")
    fscan = torch.cumsum(fkeep, 0, dtype=torch.int32)
    vscan = torch.cumsum(vflag, 0, dtype=torch.int32)
    last = lambda t: t[-1:] if t.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    n_f, n_v, bad, bad2 = torch.cat([last(fscan), last(vscan), status, mstatus]).tolist()      # the one host read
    if bad or bad2:
        raise _bad_faces(what)
    out_v = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_n = None if src_normals is None else torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    L.check(lib.i2sdf_mesh_compact_gather(L.ptr(src_verts), L.ptr(src_normals), n_src, L.ptr(mapped), F, L.ptr(fkeep), L.ptr(fscan), L.ptr(vflag),
                                          L.ptr(vscan), L.ptr(out_v), L.ptr(out_n), L.ptr(out_f), n_v, n_f, st), "i2sdf_mesh_compact_gather")
    face_map = torch.nonzero(fkeep).reshape(-1).to(torch.int32)
    return Mesh(out_v, out_f, out_n), vflag, vscan, face_map


def _vertex_map(table_of_vertex, vflag, vscan):
    """input vertex -> row of the compacted table, -1 where its table entry was not kept"""
    if table_of_vertex.numel() == 0 or vflag.numel() == 0:
        return torch.full_like(table_of_vertex, -1)
    idx = table_of_vertex.to(torch.int64)
    return torch.where(vflag[idx] != 0, vscan[idx] - 1, torch.full_like(table_of_vertex, -1)).to(torch.int32)


@torch.no_grad()
def simplify_vertex_clustering(mesh, voxel_size: float, contraction: str = "quadric", reg: float = 1e-3, _stats=None) -> SimplifyResult:
    """Vertex clustering on the grid of voxel_down_sample (cell edge `voxel_size`) by the law of include/i2sdf.h ("Mesh simplification"):
    every vertex goes to its cell; a cell's representative is, for contraction="quadric", the minimiser of the cell's summed face
    quadrics, regularised towards the cell mean by reg * trace and replaced by the mean (fallback) when it leaves the cell -- it keeps
    edges and corners, which the mean rounds off; for contraction="average" the mean itself, bit-equal to voxel_down_sample's row.  Faces
    with two corners in one cell are dropped, duplicates of the same orientation merged into the smallest face index; faces stay in
    input order, vertices come in ascending (ix, iy, iz).  Normals, when the mesh has them, are the normalised sums per cell.
    Clustering does not preserve manifoldness: `topology` says what came out.  fp64 sums in a fixed order: bitwise reproducible.
    A non-finite coordinate, a cell index beyond 21 bits per axis or a face index outside [0, V) raises I2SDFError.  Two host
    synchronisations size the results (the number of cells; the numbers of kept faces and referenced cells)."""
    what = "simplify_vertex_clustering"
    if contraction not in L.SIMPLIFY_CONTRACTIONS:
        raise ValueError(f"{what}: contraction = {contraction!r} is none of {sorted(L.SIMPLIFY_CONTRACTIONS)}")
    voxel_size, reg = float(voxel_size), float(reg)
    if not (0.0 < voxel_size < float("inf")):
        raise ValueError(f"{what}: voxel_size = {voxel_size} must be positive and finite")
    if not (0.0 < reg < float("inf")):
        raise ValueError(f"{what}: reg = {reg} must be positive and finite")
    verts, faces, normals = _simplify_mesh(mesh, what)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    lib = L.load()
    ev = _marker(_stats)
    i32 = torch.int32
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        if V == 0:
            if F:
                raise _bad_faces(what)
            return SimplifyResult(Mesh(verts, faces, normals), torch.empty(0, dtype=i32, device=dev), torch.empty(0, dtype=i32, device=dev),
                                  torch.empty(0, dtype=torch.bool, device=dev))
        pstatus = _points_status(dev)
        status = _new_status(dev)
        bounds = torch.empty(8, dtype=i32, device=dev)
        keys = torch.empty(V, dtype=torch.int64, device=dev)
        heads = torch.empty(V, dtype=i32, device=dev)
        ev("start")
        L.check(lib.i2sdf_points_bounds(L.ptr(verts), V, L.ptr(bounds), L.ptr(pstatus), st), "i2sdf_points_bounds")
        L.check(lib.i2sdf_points_voxel_keys(L.ptr(verts), V, L.ptr(bounds), voxel_size, L.ptr(keys), L.ptr(pstatus), st), "i2sdf_points_voxel_keys")
        skeys, perm = torch.sort(keys, stable=True)            # stable: a cell's vertices stay in ascending index order
        del keys
        L.check(lib.i2sdf_points_voxel_heads(L.ptr(skeys), V, L.ptr(heads), st), "i2sdf_points_voxel_heads")
        scan = torch.cumsum(heads, 0, dtype=i32)
        M, flags = torch.cat([scan[-1:], pstatus[:1]]).tolist()
        _raise_points_status(flags, what)
        vcell = torch.empty(V, dtype=i32, device=dev)
        cell_start = torch.empty(M + 1, dtype=i32, device=dev)
        L.check(lib.i2sdf_simplify_vertex_cells(L.ptr(skeys), L.ptr(perm), L.ptr(scan), V, M, L.ptr(vcell), L.ptr(cell_start), st),
                "i2sdf_simplify_vertex_cells")
        quadric = contraction == "quadric"
        cperm = cruns = None
        if quadric:
            ckeys = torch.empty(3 * F, dtype=i32, device=dev)
            cruns = torch.empty(M, 2, dtype=i32, device=dev)
            L.check(lib.i2sdf_simplify_corner_keys(L.ptr(faces), F, V, L.ptr(vcell), M, L.ptr(ckeys), L.ptr(status), st), "i2sdf_simplify_corner_keys")
            sck, cperm = torch.sort(ckeys, stable=True)       # stable: a cell's corners stay in ascending corner, hence face, order
            L.check(lib.i2sdf_simplify_corner_runs(L.ptr(sck), F, M, L.ptr(cruns), st), "i2sdf_simplify_corner_runs")
        ev("keys_sort")
        cell_v = torch.empty(M, 3, dtype=torch.float32, device=dev)
        cell_n = None if normals is None else torch.empty(M, 3, dtype=torch.float32, device=dev)
        cell_fb = torch.empty(M, dtype=torch.uint8, device=dev)
        L.check(lib.i2sdf_simplify_cells(L.ptr(verts), L.ptr(normals), V, L.ptr(faces), F, L.ptr(bounds), voxel_size, reg,
                                         L.SIMPLIFY_CONTRACTIONS[contraction], L.ptr(skeys), L.ptr(perm), L.ptr(cell_start), L.ptr(cperm),
                                         L.ptr(cruns), M, L.ptr(cell_v), L.ptr(cell_n), L.ptr(cell_fb), st), "i2sdf_simplify_cells")
        ev("reduce_solve")
        mapped = torch.empty(F, 3, dtype=i32, device=dev)
        hi = torch.empty(F, dtype=torch.int64, device=dev)
        lo = torch.empty(F, dtype=torch.int64, device=dev)
        L.check(lib.i2sdf_simplify_face_keys(None, V, L.ptr(faces), F, L.ptr(vcell), M, L.SIMPLIFY_DROP_REPEATED, L.ptr(mapped), L.ptr(hi), L.ptr(lo),
                                             L.ptr(status), st), "i2sdf_simplify_face_keys")
        out, vflag, vscan, face_map = _keep_and_compact(cell_v, cell_n, mapped, hi, lo, True, status, what, ev)
        vertex_map = _vertex_map(vcell, vflag, vscan)
        fallback = cell_fb[vflag != 0].view(torch.bool)
        ev("compaction")
    return SimplifyResult(out, vertex_map, face_map, fallback)


@torch.no_grad()
def clean(mesh, merge_vertices: bool = True, degenerate: bool = True, zero_area: bool = True, duplicated: bool = True) -> CleanResult:
    """A mesh without the things the consumers trip over, by the rules of include/i2sdf.h ("Mesh simplification"):
      merge_vertices  vertices with bit-equal positions (-0.0 = +0.0) become the smallest index among them (its normal is kept);
      degenerate      faces with a repeated index (after merging) are dropped;
      zero_area       so are faces whose fp64 (b - a) x (c - a) is exactly zero -- the faces closest_point never reports;
      duplicated      of the faces with the same cyclic vertex sequence the smallest index stays (opposite orientations both stay);
    then vertices that no kept face references are dropped.  Faces and vertices keep their relative order.  Nothing is moved, so the
    result is exact.  One host synchronisation sizes the result; a face index outside [0, V) raises I2SDFError."""
    what = "clean"
    verts, faces, normals = _simplify_mesh(mesh, what)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    lib = L.load()
    i32 = torch.int32
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        status = _new_status(dev)
        vmap = torch.arange(V, dtype=i32, device=dev)
        if merge_vertices and V:
            khi = torch.empty(V, dtype=torch.int64, device=dev)
            klo = torch.empty(V, dtype=torch.int64, device=dev)
            L.check(lib.i2sdf_simplify_position_keys(L.ptr(verts), V, L.ptr(khi), L.ptr(klo), st), "i2sdf_simplify_position_keys")
            shi, slo, perm = _sort_pairs(khi, klo)              # stable: the first of a run is its smallest index
            first = torch.empty(V, dtype=i32, device=dev)
            L.check(lib.i2sdf_simplify_run_heads(L.ptr(shi), L.ptr(slo), L.ptr(perm), V, None, L.ptr(first), st), "i2sdf_simplify_run_heads")
            head = torch.cummax(first, 0).values.to(torch.int64)
            vmap[perm] = perm[head].to(i32)
        flags = (L.SIMPLIFY_DROP_REPEATED if degenerate else 0) | (L.SIMPLIFY_DROP_ZERO_AREA if zero_area else 0)
        mapped = torch.empty(F, 3, dtype=i32, device=dev)
        hi = torch.empty(F, dtype=torch.int64, device=dev)
        lo = torch.empty(F, dtype=torch.int64, device=dev)
        L.check(lib.i2sdf_simplify_face_keys(L.ptr(verts), V, L.ptr(faces), F, L.ptr(vmap), V, flags, L.ptr(mapped), L.ptr(hi), L.ptr(lo),
                                             L.ptr(status), st), "i2sdf_simplify_face_keys")
        out, vflag, vscan, face_map = _keep_and_compact(verts, normals, mapped, hi, lo, bool(duplicated), status, what)
        vertex_map = _vertex_map(vmap, vflag, vscan)
    return CleanResult(out, vertex_map, face_map)


@torch.no_grad()
def topology(mesh) -> MeshTopology:
    """What kind of mesh this is, from its edges (include/i2sdf.h, "Mesh simplification", edge statistics): unique undirected edges;
    boundary (1 face), manifold (2 faces) and non-manifold (3 or more) edges; misoriented edges (a 2-face edge both faces traverse in
    the same direction); faces with a repeated index (their edges are left out); the vertices the other faces reference and the Euler
    number V_ref - E + F over them.  `.watertight` (no boundary, no non-manifold edge) and `.oriented` (no misoriented edge) are what
    signed_distance(sign="pseudonormal") needs; choose sign="winding" otherwise.  Enqueues only: the counts stay on the device until
    as_dict() reads them once."""
    what = "topology"
    verts, faces, _ = _simplify_mesh(mesh[:2] if isinstance(mesh, (tuple, list)) and not isinstance(mesh, MeshBVH) else mesh, what)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    lib = L.load()
    with torch.cuda.device(dev):
        st = L.stream_ptr()
        status = _new_status(dev)
        counts = torch.empty(L.TOPO_COUNTS, dtype=torch.int64, device=dev)
        keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        vflag = torch.empty(V, dtype=torch.int32, device=dev)
        L.check(lib.i2sdf_mesh_edge_stats_keys(L.ptr(faces), F, V, L.ptr(keys), L.ptr(vflag), L.ptr(counts), L.ptr(status), st),
                "i2sdf_mesh_edge_stats_keys")
        skeys = torch.sort(keys)[0]                             # (the order inside a run of equal keys does not change a count)
        L.check(lib.i2sdf_mesh_edge_stats(L.ptr(skeys), F, L.ptr(counts), st), "i2sdf_mesh_edge_stats")
    return MeshTopology(counts, status)
