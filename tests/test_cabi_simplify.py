"""CPU: the simplification entry points of the C ABI (i2sdf_simplify_*, i2sdf_mesh_edge_stats*; csrc/simplify.hip) on the cross-compiled
library: declared, exported and bound; the #defines equal the Python constants; bad arguments refused on the host before any launch (a
launch without a device would return the HIP error code -2, not -1); the Python front end refuses CPU tensors, wrong dtypes and shapes,
bad cell sizes, regularisations and names; and the kernels use no scratch, read off the in-tree build the way tests/test_cabi_closest.py
reads closest.o."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMPLIFY = ["i2sdf_simplify_vertex_cells", "i2sdf_simplify_corner_keys", "i2sdf_simplify_corner_runs", "i2sdf_simplify_cells",
            "i2sdf_simplify_face_keys", "i2sdf_simplify_run_heads", "i2sdf_simplify_position_keys"]
EDGE = ["i2sdf_mesh_edge_stats_keys", "i2sdf_mesh_edge_stats"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    assert "Mesh simplification --" in text and "xor butterfly" in text
    names = [("I2SDF_SIMPLIFY_QUADRIC", lib.SIMPLIFY_CONTRACTIONS["quadric"]), ("I2SDF_SIMPLIFY_AVERAGE", lib.SIMPLIFY_CONTRACTIONS["average"]),
             ("I2SDF_SIMPLIFY_BAD_FACE", lib.SIMPLIFY_BAD_FACE), ("I2SDF_SIMPLIFY_DROP_REPEATED", lib.SIMPLIFY_DROP_REPEATED),
             ("I2SDF_SIMPLIFY_DROP_ZERO_AREA", lib.SIMPLIFY_DROP_ZERO_AREA), ("I2SDF_TOPO_COUNTS", lib.TOPO_COUNTS)]
    names += [(f"I2SDF_TOPO_{k}", v) for k, v in lib.TOPO.items()]
    assert sorted(lib.TOPO.values()) == list(range(9)) and lib.TOPO_COUNTS == 10
    for name, val in names:
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == val, name
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_simplify_[a-z0-9_]+)\s*\(", text)) == set(SIMPLIFY)
    assert set(re.findall(r"\b(i2sdf_mesh_edge_stats[a-z0-9_]*)\s*\(", text)) == set(EDGE)
    raw = C.CDLL(lib.LIB_PATH)
    for s in SIMPLIFY + EDGE:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "simplify.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    for name in ("simplify_vertex_clustering", "clean", "topology", "SimplifyResult", "CleanResult", "MeshTopology"):
        assert callable(getattr(i2sdf_amd, name)), name
    assert i2sdf_amd.SimplifyResult._fields == ("mesh", "vertex_map", "face_map", "fallback")
    assert i2sdf_amd.CleanResult._fields == ("mesh", "vertex_map", "face_map")
    # the constants of the shared header and of the grid it reuses
    src = open(os.path.join(ROOT, "i2sdf_amd", "csrc", "quadric.h")).read()
    assert re.search(r"QD_VALUES = 9;", src) and "fp contract(off)" in src
    unit = open(os.path.join(ROOT, "i2sdf_amd", "csrc", "simplify.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and re.search(r"VOXEL_BITS = 21;", unit)
    assert re.search(r"VOXEL_BITS = 21;", open(os.path.join(ROOT, "i2sdf_amd", "csrc", "pointops.hip")).read())


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    ODD8, ODD4 = C.c_void_p(4100), C.c_void_p(4098)
    BIG, F_BIG = 1 << 31, (2 ** 31 - 1) // 3 + 1

    def vertex_cells(skeys=P, perm=P, scan=P, V=100, M=10, vcell=P, start=P):
        return h.i2sdf_simplify_vertex_cells(skeys, perm, scan, V, M, vcell, start, N)
    for kw in (dict(V=-1), dict(V=BIG), dict(M=-1), dict(M=101), dict(skeys=N), dict(skeys=ODD8), dict(perm=N), dict(perm=ODD8), dict(scan=N),
               dict(scan=ODD4), dict(vcell=N), dict(vcell=ODD4), dict(start=N), dict(start=ODD4)):
        assert vertex_cells(**kw) == -1, kw

    def corner_keys(faces=P, F=50, V=100, vcell=P, M=10, ckeys=P, status=P):
        return h.i2sdf_simplify_corner_keys(faces, F, V, vcell, M, ckeys, status, N)
    for kw in (dict(F=-1), dict(F=F_BIG), dict(V=-1), dict(V=BIG), dict(M=-1), dict(faces=N), dict(faces=ODD4), dict(vcell=N), dict(vcell=ODD4),
               dict(ckeys=N), dict(ckeys=ODD4), dict(status=N), dict(status=ODD4)):
        assert corner_keys(**kw) == -1, kw
    assert corner_keys(F=0, faces=N, ckeys=N, vcell=N) == 0          # nothing to do, nothing launched

    def corner_runs(sck=P, F=50, M=10, runs=P):
        return h.i2sdf_simplify_corner_runs(sck, F, M, runs, N)
    for kw in (dict(F=-1), dict(F=F_BIG), dict(M=-1), dict(M=BIG), dict(sck=N), dict(sck=ODD4), dict(runs=N), dict(runs=ODD4)):
        assert corner_runs(**kw) == -1, kw
    assert corner_runs(M=0, runs=N, sck=N) == 0

    def cells(**kw):
        a = dict(verts=P, normals=P, V=100, faces=P, F=50, bounds=P, h=0.1, reg=1e-3, mode=0, skeys=P, perm=P, start=P, cperm=P, runs=P, M=10,
                 out_v=P, out_n=P, fb=P)
        a.update(kw)
        return h.i2sdf_simplify_cells(a["verts"], a["normals"], a["V"], a["faces"], a["F"], a["bounds"], a["h"], a["reg"], a["mode"], a["skeys"],
                                      a["perm"], a["start"], a["cperm"], a["runs"], a["M"], a["out_v"], a["out_n"], a["fb"], N)
    inf, nan = float("inf"), float("nan")
    for kw in (dict(V=-1), dict(V=BIG), dict(F=-1), dict(F=F_BIG), dict(M=-1), dict(M=101), dict(h=0.0), dict(h=-1.0), dict(h=inf), dict(h=nan),
               dict(reg=0.0), dict(reg=-1e-3), dict(reg=inf), dict(reg=nan), dict(mode=2), dict(mode=-1), dict(verts=N), dict(verts=ODD4),
               dict(normals=ODD4), dict(out_n=N), dict(out_n=ODD4), dict(faces=N), dict(faces=ODD4), dict(bounds=N), dict(bounds=ODD4), dict(skeys=N),
               dict(skeys=ODD8), dict(perm=N), dict(perm=ODD8), dict(start=N), dict(start=ODD4), dict(cperm=N), dict(cperm=ODD8), dict(runs=N),
               dict(runs=ODD4), dict(out_v=N), dict(out_v=ODD4), dict(fb=N)):
        assert cells(**kw) == -1, kw
    assert cells(M=0) == 0

    def face_keys(verts=P, V=100, faces=P, F=50, vmap=P, n_map=10, flags=3, out=P, hi=P, lo=P, status=P):
        return h.i2sdf_simplify_face_keys(verts, V, faces, F, vmap, n_map, flags, out, hi, lo, status, N)
    for kw in (dict(V=-1), dict(V=BIG), dict(F=-1), dict(F=BIG), dict(n_map=-1), dict(flags=4), dict(flags=-1), dict(verts=N), dict(verts=ODD4),
               dict(faces=N), dict(faces=ODD4), dict(vmap=ODD4), dict(out=N), dict(out=ODD4), dict(hi=N), dict(hi=ODD8), dict(lo=N), dict(lo=ODD8),
               dict(status=N), dict(status=ODD4)):
        assert face_keys(**kw) == -1, kw
    assert face_keys(F=0, faces=N, out=N, hi=N, lo=N) == 0

    def run_heads(hi=P, lo=P, perm=P, n=50, keep=P, first=P):
        return h.i2sdf_simplify_run_heads(hi, lo, perm, n, keep, first, N)
    for kw in (dict(n=-1), dict(n=BIG), dict(hi=N), dict(hi=ODD8), dict(lo=N), dict(lo=ODD8), dict(perm=N), dict(perm=ODD8), dict(first=ODD4),
               dict(keep=N, first=N)):
        assert run_heads(**kw) == -1, kw
    assert run_heads(n=0) == 0

    def position_keys(verts=P, V=100, hi=P, lo=P):
        return h.i2sdf_simplify_position_keys(verts, V, hi, lo, N)
    for kw in (dict(V=-1), dict(V=BIG), dict(verts=N), dict(verts=ODD4), dict(hi=N), dict(hi=ODD8), dict(lo=N), dict(lo=ODD8)):
        assert position_keys(**kw) == -1, kw
    assert position_keys(V=0, verts=N) == 0

    def stats_keys(faces=P, F=50, V=100, keys=P, vflag=P, counts=P, status=P):
        return h.i2sdf_mesh_edge_stats_keys(faces, F, V, keys, vflag, counts, status, N)
    for kw in (dict(F=-1), dict(F=F_BIG), dict(V=-1), dict(V=BIG), dict(faces=N), dict(faces=ODD4), dict(keys=N), dict(keys=ODD8), dict(vflag=N),
               dict(vflag=ODD4), dict(counts=N), dict(counts=ODD8), dict(status=N), dict(status=ODD4)):
        assert stats_keys(**kw) == -1, kw

    def stats(skeys=P, F=50, counts=P):
        return h.i2sdf_mesh_edge_stats(skeys, F, counts, N)
    for kw in (dict(F=-1), dict(F=F_BIG), dict(skeys=N), dict(skeys=ODD8), dict(counts=N), dict(counts=ODD8)):
        assert stats(**kw) == -1, kw


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for call in (lambda m: A.simplify_vertex_clustering(m, 0.1), A.clean, A.topology):
        with pytest.raises(I2SDFError, match="no CPU path"):
            call((verts, faces))
        with pytest.raises(I2SDFError, match="no CPU path"):
            call(A.Mesh(verts, faces, verts))
        for bad in ((verts.double(), faces), (verts, faces.long()), (verts[:, :2], faces), (verts, faces[0]), (verts,), verts, None,
                    (verts, faces, verts[:3]), (verts, faces, verts.double())):
            if call is A.topology and isinstance(bad, tuple) and len(bad) == 3:
                continue                                           # (topology reads no normals)
            with pytest.raises(ValueError):
                call(bad)
    for h in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="voxel_size"):
            A.simplify_vertex_clustering((verts, faces), h)
    for reg in (0.0, -1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="reg"):
            A.simplify_vertex_clustering((verts, faces), 0.1, reg=reg)
    with pytest.raises(ValueError, match="contraction"):
        A.simplify_vertex_clustering((verts, faces), 0.1, contraction="median")
    import inspect
    sig = inspect.signature(A.I2SDFNetwork.extract_mesh)
    assert sig.parameters["simplify"].default is None and sig.parameters["contraction"].default == "quadric"


def test_simplify_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "simplify.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/simplify.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("simplify.hip", "quadric.h", "blockops.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("sm_vertex_cells", "sm_corner_keys", "sm_corner_runs", "sm_cells", "sm_face_keys", "sm_run_heads", "sm_position_keys", "sm_edge_keys",
            "sm_edge_runs")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in simplify.o"
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"
        assert res["vgpr"] <= 128, (name, res)                             # room for 4 waves per SIMD
