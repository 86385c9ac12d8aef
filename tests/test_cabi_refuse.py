"""CPU: the visibility-culling entry points of the C ABI (i2sdf_raster_*, csrc/raster.hip; i2sdf_tsdf_*, csrc/tsdf.hip) on the
cross-compiled library: declared, exported and bound; size queries monotone and 0 for what is not supported; bad arguments refused on
the host before any launch (no call below reaches a launch: a launch without a device would return the HIP error code -2, not -1)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RASTER = ["i2sdf_raster_workspace_bytes", "i2sdf_raster_depth"]
TSDF = ["i2sdf_tsdf_table_cells", "i2sdf_tsdf_extract_workspace_bytes", "i2sdf_tsdf_bounds", "i2sdf_tsdf_mark", "i2sdf_tsdf_integrate",
        "i2sdf_tsdf_count", "i2sdf_tsdf_emit"]
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    m = re.search(r"#define\s+I2SDF_RASTER_SMALL_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == lib.RASTER_SMALL_MAX
    assert re.search(r"#define\s+I2SDF_TSDF_MAX_CELLS\s+\(1 << 24\)", text) and lib.TSDF_MAX_CELLS == 1 << 24
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_raster_[a-z0-9_]+)\s*\(", text)) == set(RASTER)
    assert set(re.findall(r"\b(i2sdf_tsdf_[a-z0-9_]+)\s*\(", text)) == set(TSDF)
    raw = C.CDLL(lib.LIB_PATH)
    for s in RASTER + TSDF:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    build = open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    assert "raster.hip" in build and "tsdf.hip" in build
    import i2sdf_amd
    for name in ("mesh_depth", "tsdf_fuse", "refuse", "score"):
        assert callable(getattr(i2sdf_amd, name))


def test_size_queries_are_monotone_and_zero_for_unsupported_sizes(lib):
    h = lib.load()
    sizes = [1, 2, 255, 256, 257, 5000, 10 ** 5, 10 ** 6, 2 * 10 ** 6, 10 ** 8, INT32_MAX]
    for n_cam in (1, 6, 200, 65535):
        got = [int(h.i2sdf_raster_workspace_bytes(n, n, n_cam)) for n in sizes]
        assert all(g > 0 for g in got), got
        assert all(b >= a for a, b in zip(got, got[1:])), got
        # one camera's projected vertices (12 bytes each) and triangle list (4 bytes each) always fit
        assert all(g >= 12 * n + 4 * n for g, n in zip(got, sizes))
    for V, F in ((1000, 2000), (10 ** 6, 2 * 10 ** 6)):
        got = [int(h.i2sdf_raster_workspace_bytes(V, F, c)) for c in (1, 2, 3, 10, 100, 200, 1000, 65535)]
        assert all(b >= a for a, b in zip(got, got[1:])), got
    # the chunk of cameras held at once is capped: 200 cameras of a 2 M-face mesh need no more than 256 MiB
    assert h.i2sdf_raster_workspace_bytes(10 ** 6, 2 * 10 ** 6, 200) <= 256 << 20
    for bad in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (-1, 8, 1), (8, -1, 1), (8, 8, -1), (INT32_MAX + 1, 8, 1), (8, INT32_MAX + 1, 1), (8, 8, 65536)):
        assert h.i2sdf_raster_workspace_bytes(*bad) == 0, bad
    units = [1, 2, 100, 10 ** 4, 10 ** 6, 1 << 24]
    got = [int(h.i2sdf_tsdf_extract_workspace_bytes(n)) for n in units]
    assert all(g >= 7 * 4096 * n for g, n in zip(got, units)) and all(b > a for a, b in zip(got, got[1:]))
    for bad in (0, -1, (1 << 24) + 1):
        assert h.i2sdf_tsdf_extract_workspace_bytes(bad) == 0
    g6 = lambda *a: (C.c_int32 * 6)(*a)
    assert h.i2sdf_tsdf_table_cells(g6(-3, 0, 5, 7, 5, 4)) == 140
    assert h.i2sdf_tsdf_table_cells(g6(0, 0, 0, 256, 256, 256)) == 1 << 24
    assert h.i2sdf_tsdf_table_cells(g6(0, 0, 0, 257, 256, 256)) == 0          # more than 2^24 cells
    assert h.i2sdf_tsdf_table_cells(g6(0, 0, 0, 1 << 30, 1 << 30, 4)) == 0     # (and no overflow on the way)
    assert h.i2sdf_tsdf_table_cells(g6(0, 0, 0, 0, 4, 4)) == 0 and h.i2sdf_tsdf_table_cells(g6(0, 0, 0, 4, -1, 4)) == 0
    assert h.i2sdf_tsdf_table_cells(g6(1 << 22, 0, 0, 4, 4, 4)) == 0
    assert h.i2sdf_tsdf_table_cells(None) == 0


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    K4 = (C.c_float * 4)(50.0, 50.0, 32.0, 24.0)
    g6 = (C.c_int32 * 6)(0, 0, 0, 4, 4, 4)
    big6 = (C.c_int32 * 6)(0, 0, 0, 257, 256, 256)

    # raster_depth: verts, V, faces, F, w2c, n_cam, K4, H, W, znear, zfar, cull, workspace, depth, counters, status, stream
    def depth(verts=P, V=8, faces=P, F=4, w2c=P, n_cam=2, K=K4, H=48, W=64, znear=0.05, zfar=100.0, cull=1, ws=P, out=P, cnt=P, status=P):
        return h.i2sdf_raster_depth(verts, V, faces, F, w2c, n_cam, K, H, W, znear, zfar, cull, ws, out, cnt, status, N)

    assert depth(n_cam=0) == 0                                             # no cameras: nothing to do
    for kw in (dict(V=-1), dict(F=-1), dict(n_cam=-1), dict(V=INT32_MAX + 1), dict(F=INT32_MAX + 1), dict(n_cam=65536), dict(H=0), dict(W=0),
               dict(H=-4), dict(H=1 << 16, W=1 << 16), dict(K=N), dict(cull=2), dict(cull=-1), dict(znear=0.0), dict(znear=-1.0),
               dict(znear=float("nan")), dict(zfar=0.01), dict(zfar=float("inf")), dict(zfar=float("nan")), dict(verts=N), dict(faces=N),
               dict(w2c=N), dict(ws=N), dict(out=N), dict(cnt=N), dict(status=N)):
        assert depth(**kw) == -1, kw
    for k, bad in ((0, 0.0), (0, -50.0), (1, float("nan")), (1, float("inf")), (2, float("inf")), (3, float("nan"))):
        Kb = (C.c_float * 4)(*K4)
        Kb[k] = bad
        assert depth(K=Kb) == -1 and depth(K=Kb, n_cam=0) == -1, (k, bad)   # (refused even with nothing to do)

    # tsdf_bounds: depths, n_cam, H, W, c2w, K4, voxel_length, unit_length, sdf_trunc, depth_trunc, stride, bounds, stream
    def bounds(d=P, n_cam=2, H=48, W=64, c2w=P, K=K4, vl=0.02, ul=0.32, tr=0.06, dt=5.0, stride=4, b=P):
        return h.i2sdf_tsdf_bounds(d, n_cam, H, W, c2w, K, vl, ul, tr, dt, stride, b, N)

    assert bounds(n_cam=0) == 0
    common = (dict(n_cam=-1), dict(n_cam=65536), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 16), dict(K=N), dict(vl=0.0), dict(vl=-0.02),
              dict(vl=float("nan")), dict(vl=float("inf")), dict(ul=0.0), dict(ul=float("inf")), dict(tr=0.0), dict(tr=float("nan")),
              dict(tr=float("inf")), dict(dt=0.0), dict(dt=float("nan")), dict(d=N), dict(c2w=N))
    for kw in common + (dict(stride=0), dict(stride=-4), dict(b=N)):
        assert bounds(**kw) == -1, kw

    # tsdf_mark: depths, n_cam, cam, H, W, c2w, K4, vl, ul, trunc, dtrunc, stride, grid6, slot, n_units, stamp, list, list_count, flag, stream
    def mark(d=P, n_cam=2, cam=0, H=48, W=64, c2w=P, K=K4, vl=0.02, ul=0.32, tr=0.06, dt=5.0, stride=4, g=g6, slot=P, n_units=8, stamp=P,
             lst=P, cnt=P, flag=P):
        return h.i2sdf_tsdf_mark(d, n_cam, cam, H, W, c2w, K, vl, ul, tr, dt, stride, g, slot, n_units, stamp, lst, cnt, flag, N)

    assert mark(n_cam=0) == 0 and mark(n_cam=0, slot=N) == 0
    for kw in common + (dict(stride=0), dict(g=N), dict(g=big6), dict(stamp=N), dict(flag=N), dict(cam=-1), dict(cam=2), dict(lst=N),
                        dict(cnt=N), dict(n_units=0), dict(n_units=-1), dict(n_units=(1 << 24) + 1)):
        assert mark(**kw) == -1, kw
    for kw in (dict(g=big6), dict(stamp=N), dict(flag=N), dict(d=N), dict(stride=0)):   # the union pass (no slot table) is checked alike
        assert mark(slot=N, lst=N, cnt=N, n_units=0, **kw) == -1, kw

    # tsdf_integrate: depths, n_cam, cam, H, W, w2c, K4, vl, ul, trunc, dtrunc, grid6, unit_cell, n_units, list, list_count, tsdf, weight, stream
    def integrate(d=P, n_cam=2, cam=1, H=48, W=64, w2c=P, K=K4, vl=0.02, ul=0.32, tr=0.06, dt=5.0, g=g6, uc=P, n_units=8, lst=P, cnt=P,
                  tsdf=P, weight=P):
        return h.i2sdf_tsdf_integrate(d, n_cam, cam, H, W, w2c, K, vl, ul, tr, dt, g, uc, n_units, lst, cnt, tsdf, weight, N)

    for kw in tuple(k for k in common if "c2w" not in k) + (dict(n_cam=0), dict(w2c=N), dict(g=N), dict(g=big6), dict(cam=-1), dict(cam=2),
                                                              dict(uc=N), dict(lst=N), dict(cnt=N), dict(tsdf=N), dict(weight=N),
                                                              dict(n_units=0), dict(n_units=(1 << 24) + 1)):
        assert integrate(**kw) == -1, kw

    # tsdf_count: grid6, slot, unit_cell, n_units, tsdf, weight, workspace, blocks, stream
    def count(g=g6, slot=P, uc=P, n_units=8, tsdf=P, weight=P, ws=P, blocks=P):
        return h.i2sdf_tsdf_count(g, slot, uc, n_units, tsdf, weight, ws, blocks, N)

    for kw in (dict(g=N), dict(g=big6), dict(slot=N), dict(uc=N), dict(n_units=0), dict(n_units=-1), dict(n_units=(1 << 24) + 1), dict(tsdf=N),
               dict(weight=N), dict(ws=N), dict(blocks=N)):
        assert count(**kw) == -1, kw

    # tsdf_emit: grid6, vl, ul, slot, unit_cell, n_units, tsdf, weight, workspace, blocks_excl, verts, normals, faces, cap_v, cap_f, stream
    def emit(g=g6, vl=0.02, ul=0.32, slot=P, uc=P, n_units=8, tsdf=P, weight=P, ws=P, be=P, verts=P, normals=P, faces=P, cap_v=10, cap_f=10):
        return h.i2sdf_tsdf_emit(g, vl, ul, slot, uc, n_units, tsdf, weight, ws, be, verts, normals, faces, cap_v, cap_f, N)

    assert emit(cap_v=0) == 0 and emit(cap_f=0, verts=N) == 0               # no room: nothing is written
    for kw in (dict(g=N), dict(g=big6), dict(vl=0.0), dict(vl=float("nan")), dict(ul=-1.0), dict(slot=N), dict(uc=N), dict(n_units=0),
               dict(tsdf=N), dict(weight=N), dict(ws=N), dict(be=N), dict(verts=N), dict(normals=N), dict(faces=N), dict(cap_v=-1),
               dict(cap_f=-1), dict(cap_v=INT32_MAX + 1), dict(cap_f=INT32_MAX + 1)):
        assert emit(**kw) == -1, kw


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    """Everything that can be judged without touching a device is: the mesh / depth arguments come first and must be device tensors,
    so a CPU tensor there raises ValueError before the library is even loaded."""
    import torch
    import i2sdf_amd as A
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    poses, K = torch.eye(4)[None], torch.tensor([[50.0, 0, 32], [0, 50.0, 24], [0, 0, 1]])
    with pytest.raises(ValueError):
        A.mesh_depth((v, f), poses, K, 48, 64)                            # not on a GPU
    with pytest.raises(ValueError):
        A.tsdf_fuse(torch.zeros(1, 48, 64), poses, K)
    with pytest.raises(ValueError):
        A.refuse((v, f), poses, K, 48, 64)
    with pytest.raises(ValueError):
        A.score((v, f), (v, f), poses, K, 48, 64)
