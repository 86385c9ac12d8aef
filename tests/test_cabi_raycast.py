"""CPU: the ray-casting entry points of the C ABI (i2sdf_bvh_*, i2sdf_mesh_trace_brute; csrc/bvh.hip) on the cross-compiled library:
declared, exported and bound; the size query monotone, a multiple of 16, within the stated bytes per face and 0 outside its range; bad
arguments refused on the host before any launch (a launch without a device would return the HIP error code -2, not -1); the Python
front end refuses CPU tensors and bad shapes; and the kernels use no scratch, read off the in-tree build the way
tests/test_cabi_dbscan.py reads dbscan.o."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYCAST = ["i2sdf_bvh_bytes", "i2sdf_bvh_keys", "i2sdf_bvh_build", "i2sdf_bvh_trace", "i2sdf_mesh_trace_brute"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    assert "Ray casting against a triangle mesh" in text and "124 bytes per face" in text
    for name, val in (("I2SDF_RAYCAST_BAD_RAY", lib.RAYCAST_BAD_RAY), ("I2SDF_RAYCAST_BAD_FACE", lib.RAYCAST_BAD_FACE),
                      ("I2SDF_RAYCAST_CULL_NONE", lib.RAYCAST_CULL["none"]), ("I2SDF_RAYCAST_CULL_BACK", lib.RAYCAST_CULL["back"]),
                      ("I2SDF_BVH_MAX_FACES", lib.BVH_MAX_FACES)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == val, name
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_bvh_[a-z0-9_]+|i2sdf_mesh_trace_[a-z0-9_]+)\s*\(", text)) == set(RAYCAST)
    raw = C.CDLL(lib.LIB_PATH)
    for s in RAYCAST:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "bvh.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    for name in ("build_bvh", "ray_mesh_intersect", "occluded", "MeshBVH", "RayHits", "MeshTracer"):
        assert callable(getattr(i2sdf_amd, name)), name
    assert callable(i2sdf_amd.I2SDFNetwork.mesh_tracer)


def test_size_query(lib):
    h = lib.load()
    size = lambda F: int(h.i2sdf_bvh_bytes(F))
    sizes = [0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 1023, 1025, 4099, 1 << 20, (1 << 21) + 7, 1 << 27, (1 << 28) - 1, 1 << 28]
    got = [size(F) for F in sizes]
    assert all(g > 0 and g % 16 == 0 for g in got), got
    assert all(b > a for a, b in zip(got, got[1:]))
    assert all(g <= 124 * F + 304 for F, g in zip(sizes, got)), [(F, g) for F, g in zip(sizes, got) if g > 124 * F + 304]
    assert got[-1] >= 124 * (1 << 28)                              # (every record is there: 64 + 48 + 12 bytes per face)
    dense = [size(F) for F in range(0, 3000)]
    assert all(g % 16 == 0 and g <= 124 * F + 304 for F, g in enumerate(dense)) and all(b > a for a, b in zip(dense, dense[1:]))
    for bad in (-1, -(1 << 40), (1 << 28) + 1, 1 << 31, 1 << 40):
        assert size(bad) == 0, bad


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    ODD16, ODD8, ODD4 = C.c_void_p(4104), C.c_void_p(4100), C.c_void_p(4098)
    bad_mesh = (dict(F=-1), dict(F=(1 << 28) + 1), dict(F=1 << 40), dict(V=-1), dict(V=1 << 31), dict(verts=N), dict(verts=ODD4), dict(faces=N),
                dict(faces=ODD4))
    bad_rays = (dict(n=-1), dict(n=1 << 31), dict(cull=2), dict(cull=-1), dict(any_hit=2), dict(any_hit=-1), dict(orig=N), dict(orig=ODD4),
                dict(dirs=N), dict(dirs=ODD4), dict(t_min=N), dict(t_min=ODD4), dict(t_max=N), dict(t_max=ODD4), dict(t=N), dict(t=ODD4),
                dict(face=N), dict(face=ODD4), dict(bary=N), dict(bary=ODD4), dict(hit=N), dict(status=N), dict(status=ODD4))

    def keys(verts=P, V=100, faces=P, F=50, bvh=P, keys=P):
        return h.i2sdf_bvh_keys(verts, V, faces, F, bvh, keys, N)

    for kw in bad_mesh + (dict(bvh=N), dict(bvh=ODD16), dict(bvh=ODD8), dict(keys=N), dict(keys=ODD8)):
        assert keys(**kw) == -1, kw

    def build(verts=P, V=100, faces=P, F=50, skeys=P, bvh=P):
        return h.i2sdf_bvh_build(verts, V, faces, F, skeys, bvh, N)

    for kw in bad_mesh + (dict(bvh=N), dict(bvh=ODD16), dict(skeys=N), dict(skeys=ODD8)):
        assert build(**kw) == -1, kw
    assert build(F=0, verts=N, faces=N, skeys=N) == 0              # the empty tree: nothing to launch

    def trace(bvh=P, F=50, orig=P, dirs=P, t_min=P, t_max=P, n=10, cull=0, any_hit=0, t=P, face=P, bary=P, hit=P, status=P):
        return h.i2sdf_bvh_trace(bvh, F, orig, dirs, t_min, t_max, n, cull, any_hit, t, face, bary, hit, status, N)

    for kw in bad_rays + (dict(F=-1), dict(F=(1 << 28) + 1), dict(bvh=N), dict(bvh=ODD16)):
        assert trace(**kw) == -1, kw
    assert trace(any_hit=1, t=N, face=N, bary=N, hit=N) == -1      # the flag itself is still needed

    def brute(verts=P, V=100, faces=P, F=50, orig=P, dirs=P, t_min=P, t_max=P, n=10, cull=0, any_hit=0, t=P, face=P, bary=P, hit=P, status=P):
        return h.i2sdf_mesh_trace_brute(verts, V, faces, F, orig, dirs, t_min, t_max, n, cull, any_hit, t, face, bary, hit, status, N)

    for kw in bad_mesh + bad_rays:
        assert brute(**kw) == -1, kw


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    rays = torch.zeros(5, 3)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.build_bvh((verts, faces))
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.ray_mesh_intersect((verts, faces), rays, rays)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.occluded(A.Mesh(verts, faces, verts), rays, rays)
    for bad in ((verts.double(), faces), (verts, faces.long()), (verts[:, :2], faces), (verts, faces[0]), (verts,), verts, None):
        with pytest.raises(ValueError):
            A.build_bvh(bad)
        with pytest.raises(ValueError):
            A.ray_mesh_intersect(bad, rays, rays)
    with pytest.raises(ValueError, match="cull"):
        A.ray_mesh_intersect((verts, faces), rays, rays, cull="front")
    with pytest.raises(ValueError, match="route"):
        A.ray_mesh_intersect((verts, faces), rays, rays, route="gpu")
    net = A.I2SDFNetwork(A.plumbing_conf())
    with pytest.raises(I2SDFError, match="no CPU path"):
        net.mesh_tracer((verts, faces))
    with pytest.raises(ValueError, match="cull"):
        net.mesh_tracer((verts, faces), cull="front")
    with pytest.raises(TypeError):
        net.mesh_tracer((verts, faces), t_min="0")


def test_ray_arguments_are_checked():
    import torch
    from i2sdf_amd import mesh as M
    dev = torch.device("cpu")
    o = torch.zeros(5, 3)
    for bad_o, bad_d in ((torch.zeros(5, 2), o), (o, torch.zeros(4, 3)), (o.long(), o), (torch.zeros(5), o), ([[0.0] * 3], o)):
        with pytest.raises(ValueError):
            M._ray_args(bad_o, bad_d, 0.0, 1.0, dev, "t")
    for t_min, t_max in ((torch.zeros(4), 1.0), (0.0, torch.zeros(5, 1)), (torch.zeros(5, dtype=torch.int32), 1.0)):
        with pytest.raises(ValueError):
            M._ray_args(o, o, t_min, t_max, dev, "t")
    for t_min in ("0", None, True):
        with pytest.raises(TypeError):
            M._ray_args(o, o, t_min, 1.0, dev, "t")
    a, b, lo, hi = M._ray_args(o.double(), o.double(), 0, torch.full((5,), 2.0, dtype=torch.float64), dev, "t")
    assert a.dtype == b.dtype == lo.dtype == hi.dtype == torch.float32 and lo.tolist() == [0.0] * 5 and hi.tolist() == [2.0] * 5


def test_raycast_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "bvh.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/bvh.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("bvh.hip", "tri_isect.h", "blockops.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("bvh_bounds_kernel", "bvh_keys_kernel", "bvh_leaves_kernel", "bvh_topology_kernel", "bvh_boxes_kernel", "bvh_trace_kernel",
            "mesh_faces_check_kernel", "mesh_trace_brute_kernel")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in bvh.o"
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"      # the trace's stack is in LDS
        assert res["vgpr"] <= 128, (name, res)                             # room for 4 waves per SIMD
