"""Marching cubes on the device (csrc/mcubes.hip): the zero-level mesh of an SDF volume, in place of the host round trip
`volume.cpu().numpy()` -> `skimage.measure.marching_cubes` of model/eval/recon.py:53-60,91-95 and utils/plots.py:197-206.

Conventions are scikit-image's (Lewiner, gradient_direction='descent'): one vertex per lattice edge that crosses the level,
at linear interpolation; `verts` in index units x spacing (+ origin); int32 faces whose right-hand normal points towards
increasing values; `normals` pointing towards DEcreasing values (inward for an SDF).  Two differences:
  * ambiguous cells follow one fixed rule (csrc/gen_mc_tables.py) instead of Lewiner's, so on non-smooth volumes the
    triangulation of those cells differs (the mesh is still closed and consistently oriented);
  * a volume without any crossing gives empty tensors where scikit-image raises (and the reference returns None).
`values` is not returned (no reference call site reads it).
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
