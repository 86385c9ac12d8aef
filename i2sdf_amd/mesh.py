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
