"""CPU: the bubble entry points of the C ABI (i2sdf_bubble_*, i2sdf_depth_unproject_*, csrc/bubble.hip) on the cross-compiled library:
declared, exported and bound; the size queries monotone and 0 for what is not supported; bad arguments refused on the host before any
launch (no call below reaches a launch: a launch without a device would return the HIP error code -2, not -1); and the new kernels
use no scratch, read off the in-tree build the way tests/test_kernel_resources.py reads the hot kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUBBLE = ["i2sdf_bubble_sample_workspace_bytes", "i2sdf_bubble_sample", "i2sdf_bubble_keys"]
UNPROJECT = ["i2sdf_depth_unproject_workspace_bytes", "i2sdf_depth_unproject_count", "i2sdf_depth_unproject_write"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    m = re.search(r"#define\s+I2SDF_BUBBLE_MAX_K\s+(\d+)", text)
    assert m and int(m.group(1)) == lib.BUBBLE_MAX_K == 4096
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_bubble_[a-z0-9_]+)\s*\(", text)) == set(BUBBLE)
    assert set(re.findall(r"\b(i2sdf_depth_unproject_[a-z0-9_]+)\s*\(", text)) == set(UNPROJECT)
    raw = C.CDLL(lib.LIB_PATH)
    for s in BUBBLE + UNPROJECT:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "bubble.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    assert callable(i2sdf_amd.depth_unproject)
    for name in ("from_depth", "sample_bubble", "sample_bubble_device", "sampler_state", "load_sampler_state", "shortfall"):
        assert callable(getattr(i2sdf_amd.BubblePDF, name)), name


def test_workspace_queries(lib):
    h = lib.load()
    got = [int(h.i2sdf_bubble_sample_workspace_bytes(k)) for k in range(1, 4097)]
    assert all(g > 0 and g % 16 == 0 for g in got)
    assert all(b > a for a, b in zip(got, got[1:]))                       # monotone in k
    assert got[-1] - got[0] == 16 * 4095 and got[-1] < 1 << 17           # 2k records of 8 bytes next to fixed histograms: ~100 KB at most
    for bad in (0, -1, 4097, 1 << 40):
        assert h.i2sdf_bubble_sample_workspace_bytes(bad) == 0, bad
    ws = lambda n, H, W: int(h.i2sdf_depth_unproject_workspace_bytes(n, H, W))
    sizes = [ws(n, 480, 640) for n in (0, 1, 2, 150, 1000)]
    assert all(g > 0 for g in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert ws(150, 480, 640) < 150 * 480 * 640 // 50                      # per-block counts, not per-pixel state
    for bad in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (1, 1 << 16, 1 << 15), (1 << 20, 1 << 10, 1 << 10)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None

    # weights, n, pointcloud, k, seed, draw, workspace, idx, points, sample_count, status, stream
    def sample(w=P, n=1000, pc=P, k=16, ws=P, idx=P, pts=P, sc=P, st=P):
        return h.i2sdf_bubble_sample(w, n, pc, k, 1, 0, ws, idx, pts, sc, st, N)

    for kw in (dict(k=0), dict(k=-1), dict(k=4097), dict(n=1 << 31), dict(n=-1), dict(n=1 << 40), dict(idx=N), dict(ws=N),
               dict(ws=C.c_void_p(4100)), dict(k=0, n=0), dict(k=4097, w=N)):
        assert sample(**kw) == -1, kw

    # weights, n, seed, draw, keys_out, stream
    assert h.i2sdf_bubble_keys(P, 0, 1, 0, N, N) == 0                      # nothing to do
    for n, out in ((-1, P), (1 << 31, P), (10, N)):
        assert h.i2sdf_bubble_keys(P, n, 1, 0, out, N) == -1, (n, out)

    # depth, n_img, H, W, lo, hi, workspace, depth_masks, n_points (host), stream
    n_pts = C.c_int64(-7)

    def count(d=P, n=2, H=5, W=7, ws=P, masks=P, out=C.byref(n_pts)):
        return h.i2sdf_depth_unproject_count(d, n, H, W, 1e-3, 6.0, ws, masks, out, N)

    assert count(n=0) == 0 and n_pts.value == 0                            # no images: no points, nothing launched
    sizes = (dict(n=-1), dict(H=0), dict(W=0), dict(H=-5), dict(H=1 << 16, W=1 << 15), dict(n=1 << 30, H=1 << 10, W=1 << 10))
    for kw in sizes + (dict(d=N), dict(ws=N), dict(out=None)):
        assert count(**kw) == -1, kw

    # depth, intrinsics, pose, n_img, H, W, lo, hi, workspace, n_points, pointlinks, pixlinks, pointcloud, stream
    def write(d=P, K=P, M=P, n=2, H=5, W=7, ws=P, n_points=10, links=P, pix=P, cloud=P):
        return h.i2sdf_depth_unproject_write(d, K, M, n, H, W, 1e-3, 6.0, ws, n_points, links, pix, cloud, N)

    assert write(n=0, n_points=0) == 0 and write(links=N, pix=N, cloud=N) == 0
    for kw in sizes + (dict(d=N), dict(ws=N), dict(n_points=-1), dict(n_points=71), dict(K=N), dict(M=N)):
        assert write(**kw) == -1, kw


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    with pytest.raises(I2SDFError):
        A.BubblePDF(torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), device="cpu", sampler="device")
    with pytest.raises(I2SDFError):
        A.depth_unproject(torch.zeros(1, 12), torch.eye(4)[None], torch.eye(4)[None], (3, 4), device="cpu")


def test_bubble_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "bubble.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/bubble.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("bubble.hip", "philox.h", "blockops.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("bubble_keys_kernel", "bubble_hist_kernel", "bubble_pick_kernel", "bubble_collect_kernel", "bubble_finish_kernel",
            "unproject_count_kernel", "unproject_scan_kernel", "unproject_write_kernel")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in bubble.o"
    assert sum("bubble_hist_kernel" in name for name in kernels) == 3      # one instantiation per digit of the select
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"
        assert res["vgpr"] <= 128, (name, res)                             # streaming kernels: room for 4 waves per SIMD
