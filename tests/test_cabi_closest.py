"""CPU: the closest-point entry points of the C ABI (i2sdf_closest_*; csrc/closest.hip) on the cross-compiled library: declared,
exported and bound; the #defines equal the Python constants; bad arguments refused on the host before any launch (a launch without
a device would return the HIP error code -2, not -1); the Python front end refuses CPU tensors, wrong dtypes and shapes and unknown
routes; and the kernels use no scratch, read off the in-tree build the way tests/test_cabi_dbscan.py reads dbscan.o."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSEST = ["i2sdf_closest_bvh", "i2sdf_closest_brute", "i2sdf_closest_normal_keys", "i2sdf_closest_normals"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    assert "Closest point --" in text and "MEANS NOTHING" in text
    names = [("I2SDF_CLOSEST_BAD_POINT", lib.CLOSEST_BAD_POINT), ("I2SDF_CLOSEST_BAD_FACE", lib.CLOSEST_BAD_FACE)]
    names += [(f"I2SDF_CLOSEST_{k}", v) for k, v in lib.CLOSEST_FEATURES.items()]
    assert len(lib.CLOSEST_FEATURES) == 7 and sorted(lib.CLOSEST_FEATURES.values()) == list(range(7))
    for name, val in names:
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == val, name
    assert lib.CLOSEST_BAD_FACE == lib.RAYCAST_BAD_FACE            # (the tree's header carries that bit to both queries)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_closest_[a-z0-9_]+)\s*\(", text)) == set(CLOSEST)
    raw = C.CDLL(lib.LIB_PATH)
    for s in CLOSEST:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "closest.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    for name in ("closest_point", "pseudonormals", "signed_distance", "surface_scores", "ClosestPoints", "MeshNormals"):
        assert callable(getattr(i2sdf_amd, name)), name
    assert i2sdf_amd.MeshBVH._fields == ("verts", "faces", "buffer")
    assert i2sdf_amd.ClosestPoints._fields == ("dist", "point", "face", "bary", "feature", "sdist", "status")
    # the header's feature codes are the shared header's
    src = open(os.path.join(ROOT, "i2sdf_amd", "csrc", "tri_closest.h")).read()
    m = re.search(r"CP_FACE = (\d), CP_EDGE_AB = (\d), CP_EDGE_BC = (\d), CP_EDGE_CA = (\d), CP_VERT_A = (\d), CP_VERT_B = (\d), CP_VERT_C = (\d)", src)
    assert m and [int(x) for x in m.groups()] == [lib.CLOSEST_FEATURES[k] for k in ("FACE", "EDGE_AB", "EDGE_BC", "EDGE_CA", "VERT_A", "VERT_B", "VERT_C")]


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    ODD16, ODD8, ODD4 = C.c_void_p(4104), C.c_void_p(4100), C.c_void_p(4098)
    bad_mesh = (dict(F=-1), dict(F=(1 << 28) + 1), dict(F=1 << 40), dict(V=-1), dict(V=1 << 31), dict(verts=N), dict(verts=ODD4), dict(faces=N),
                dict(faces=ODD4))
    bad_query = (dict(n=-1), dict(n=1 << 31), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=-float("inf")),
                 dict(points=N), dict(points=ODD4), dict(dist=N), dict(dist=ODD4), dict(point=N), dict(point=ODD4), dict(face=N),
                 dict(face=ODD4), dict(bary=N), dict(bary=ODD4), dict(feature=N), dict(status=N), dict(status=ODD4),
                 dict(vnormal=N), dict(enormal=N), dict(sdist=N), dict(vnormal=N, enormal=N), dict(vnormal=ODD4), dict(enormal=ODD4),
                 dict(sdist=ODD4), dict(vnormal=P, enormal=N, sdist=N, _plain=True), dict(sdist=P, _plain=True))

    def query(fn, head, kw):
        a = dict(points=P, n=10, max_dist=1.0, vnormal=P, enormal=P, dist=P, point=P, face=P, bary=P, feature=P, sdist=P, status=P)
        if kw.pop("_plain", False):
            a.update(vnormal=N, enormal=N, sdist=N)
        a.update(kw)
        return fn(*head, a["points"], a["n"], a["max_dist"], a["vnormal"], a["enormal"], a["dist"], a["point"], a["face"], a["bary"],
                  a["feature"], a["sdist"], a["status"], N)

    def mesh(kw):
        a = dict(verts=P, V=100, faces=P, F=50)
        for k in list(kw):
            if k in a:
                a[k] = kw.pop(k)
        return (a["verts"], a["V"], a["faces"], a["F"])

    for kw in bad_mesh + bad_query + (dict(bvh=N), dict(bvh=ODD16), dict(bvh=ODD8)):
        kw = dict(kw)
        bvh = kw.pop("bvh", P)
        assert query(h.i2sdf_closest_bvh, (bvh,) + mesh(kw), kw) == -1, kw
    for kw in bad_mesh + bad_query:
        kw = dict(kw)
        assert query(h.i2sdf_closest_brute, mesh(kw), kw) == -1, kw

    def keys(verts=P, V=100, faces=P, F=50, keys=P, status=P):
        return h.i2sdf_closest_normal_keys(verts, V, faces, F, keys, status, N)

    for kw in bad_mesh + (dict(keys=N), dict(keys=ODD8), dict(status=N), dict(status=ODD4)):
        assert keys(**kw) == -1, kw

    def normals(verts=P, V=100, faces=P, F=50, skeys=P, perm=P, vnormal=P, enormal=P):
        return h.i2sdf_closest_normals(verts, V, faces, F, skeys, perm, vnormal, enormal, N)

    for kw in bad_mesh + (dict(skeys=N), dict(skeys=ODD8), dict(perm=N), dict(perm=ODD8), dict(vnormal=N), dict(vnormal=ODD4), dict(enormal=N),
                          dict(enormal=ODD4)):
        assert normals(**kw) == -1, kw
    assert normals(V=0, F=0, verts=N, faces=N, skeys=N, perm=N, vnormal=N, enormal=N) == 0      # nothing to do, nothing launched


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    pts = torch.zeros(5, 3)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.closest_point((verts, faces), pts)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.pseudonormals((verts, faces))
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.signed_distance(A.Mesh(verts, faces, verts), pts)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.surface_scores((verts, faces), (verts, faces), 10)
    for bad in ((verts.double(), faces), (verts, faces.long()), (verts[:, :2], faces), (verts, faces[0]), (verts,), verts, None):
        for call in (lambda m: A.closest_point(m, pts), A.pseudonormals, lambda m: A.signed_distance(m, pts),
                     lambda m: A.surface_scores(m, (verts, faces), 10), lambda m: A.surface_scores((verts, faces), m, 10)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError, match="route"):
        A.closest_point((verts, faces), pts, route="gpu")
    for md in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            A.closest_point((verts, faces), pts, max_dist=md)


def test_query_arguments_are_checked():
    import torch
    from i2sdf_amd import mesh as M
    dev = torch.device("cpu")
    for bad in (torch.zeros(5, 2), torch.zeros(5), torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.int32), [[0.0] * 3], None):
        with pytest.raises(ValueError):
            M._query_points(bad, dev, "t")
    assert M._query_points(torch.zeros(7, 3)[::2], dev, "t").is_contiguous()
    vn, en = torch.zeros(4, 3), torch.zeros(2, 3, 3)
    assert M._normals_arg(None, 4, 2, dev, "t") is None
    assert isinstance(M._normals_arg((vn, en), 4, 2, dev, "t"), M.MeshNormals)
    for bad in ((vn,), vn, (vn, en[:1]), (vn[:3], en), (vn.double(), en), (vn, en.reshape(2, 9)), (en, vn)):
        with pytest.raises(ValueError):
            M._normals_arg(bad, 4, 2, dev, "t")


def test_closest_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "closest.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/closest.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("closest.hip", "tri_closest.h", "bvh_tree.h", "blockops.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("closest_bvh_kernel", "closest_brute_kernel", "closest_faces_check_kernel", "closest_normal_keys_kernel",
            "closest_normal_reduce_kernel")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in closest.o"
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"      # the walk's stack is in LDS
        assert res["vgpr"] <= 128, (name, res)                             # room for 4 waves per SIMD
