"""CPU: the point-set entry points of the C ABI (i2sdf_points_*, csrc/pointops.hip) on the cross-compiled library: declared,
exported and bound; workspace queries positive and monotone; bad arguments refused on the host before any launch (no call below
reaches a launch: a launch without a device would return the HIP error code -2, not -1)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["i2sdf_points_bounds", "i2sdf_points_voxel_keys", "i2sdf_points_voxel_heads", "i2sdf_points_voxel_mean",
           "i2sdf_points_grid_workspace_bytes", "i2sdf_points_grid_keys", "i2sdf_points_grid_build", "i2sdf_points_nn_query",
           "i2sdf_points_nn_fallback", "i2sdf_points_reduce_workspace_bytes", "i2sdf_points_threshold_reduce"]
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(i2sdf_points_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    raw = C.CDLL(lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "pointops.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()


def test_workspace_queries_are_positive_and_monotone(lib):
    h = lib.load()
    sizes = [1, 2, 31, 32, 33, 1000, 1024, 1025, 5108, 10 ** 5, 10 ** 6, 2 * 10 ** 6, 10 ** 7, 10 ** 9, INT32_MAX]
    for fn in (h.i2sdf_points_grid_workspace_bytes, h.i2sdf_points_reduce_workspace_bytes):
        got = [int(fn(n)) for n in sizes]
        assert all(g > 0 for g in got), got
        assert all(b >= a for a, b in zip(got, got[1:])), got
        assert fn(0) == 0 and fn(-1) == 0 and fn(INT32_MAX + 1) == 0
    # the grid's tables are capped (2^22 cells, two int32 tables) however many points, and hold about two cells per point below
    assert h.i2sdf_points_grid_workspace_bytes(INT32_MAX) == h.i2sdf_points_grid_workspace_bytes(10 ** 8) <= 2 * 4 * 2 ** 22 + 4096
    assert h.i2sdf_points_grid_workspace_bytes(10 ** 5) >= 2 * 4 * 2 * 10 ** 5
    assert h.i2sdf_points_reduce_workspace_bytes(2 * 10 ** 6) >= 16 * (2 * 10 ** 6 // 1024)


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P = C.c_void_p(4096)
    N = None
    # bounds: points, n, bounds, status, stream
    assert h.i2sdf_points_bounds(P, -1, P, P, N) == -1
    assert h.i2sdf_points_bounds(P, INT32_MAX + 1, P, P, N) == -1
    assert h.i2sdf_points_bounds(N, 8, P, P, N) == -1
    assert h.i2sdf_points_bounds(P, 8, N, P, N) == -1
    assert h.i2sdf_points_bounds(P, 8, P, N, N) == -1
    # voxel_keys: points, n, bounds, voxel_size, keys, status, stream
    assert h.i2sdf_points_voxel_keys(P, 0, P, 0.02, P, P, N) == 0                 # nothing to do
    for bad in (0.0, -0.02, float("nan"), float("inf")):
        assert h.i2sdf_points_voxel_keys(P, 8, P, bad, P, P, N) == -1
        assert h.i2sdf_points_voxel_keys(P, 0, P, bad, P, P, N) == -1             # (refused even with nothing to do)
    assert h.i2sdf_points_voxel_keys(P, -1, P, 0.02, P, P, N) == -1
    for k in range(4):
        a = [P, P, P, P]
        a[k] = N
        assert h.i2sdf_points_voxel_keys(a[0], 8, a[1], 0.02, a[2], a[3], N) == -1
    # voxel_heads: sorted_keys, n, heads, stream
    assert h.i2sdf_points_voxel_heads(P, 0, P, N) == 0
    assert h.i2sdf_points_voxel_heads(P, -1, P, N) == -1
    assert h.i2sdf_points_voxel_heads(N, 8, P, N) == -1 and h.i2sdf_points_voxel_heads(P, 8, N, N) == -1
    # voxel_mean: points, n, sorted_keys, perm, head_scan, out_points, out_counts, cap_m, stream
    assert h.i2sdf_points_voxel_mean(P, 0, P, P, P, P, P, 0, N) == 0
    assert h.i2sdf_points_voxel_mean(P, 8, P, P, P, P, P, 0, N) == 0              # no room: nothing is written
    assert h.i2sdf_points_voxel_mean(P, -1, P, P, P, P, P, 4, N) == -1
    assert h.i2sdf_points_voxel_mean(P, 8, P, P, P, P, P, -1, N) == -1
    for k in range(6):
        a = [P] * 6
        a[k] = N
        assert h.i2sdf_points_voxel_mean(a[0], 8, a[1], a[2], a[3], a[4], a[5], 4, N) == -1
    # grid_keys: ref, n_ref, workspace, keys, status, stream
    for n in (0, -1, INT32_MAX + 1):
        assert h.i2sdf_points_grid_keys(P, n, P, P, P, N) == -1
    for k in range(4):
        a = [P] * 4
        a[k] = N
        assert h.i2sdf_points_grid_keys(a[0], 8, a[1], a[2], a[3], N) == -1
    # grid_build: ref, n_ref, sorted_keys, perm, workspace, sorted_ref, stream
    for n in (0, -1, INT32_MAX + 1):
        assert h.i2sdf_points_grid_build(P, n, P, P, P, P, N) == -1
    for k in range(5):
        a = [P] * 5
        a[k] = N
        assert h.i2sdf_points_grid_build(a[0], 8, a[1], a[2], a[3], a[4], N) == -1
    # nn_query: query, n_query, sorted_ref, n_ref, workspace, max_ring, dist, index, fallback_list, status, stream
    assert h.i2sdf_points_nn_query(P, 0, P, 8, P, 4, P, P, P, P, N) == 0          # no queries
    assert h.i2sdf_points_nn_query(P, -1, P, 8, P, 4, P, P, P, P, N) == -1
    assert h.i2sdf_points_nn_query(P, 8, P, 0, P, 4, P, P, P, P, N) == -1         # nothing to search in
    assert h.i2sdf_points_nn_query(P, 0, P, 0, P, 4, P, P, P, P, N) == -1
    assert h.i2sdf_points_nn_query(P, 8, P, -1, P, 4, P, P, P, P, N) == -1
    assert h.i2sdf_points_nn_query(P, 8, P, 8, P, -1, P, P, P, P, N) == -1        # a negative ring budget
    for k in range(7):
        a = [P] * 7
        a[k] = N
        assert h.i2sdf_points_nn_query(a[0], 8, a[1], 8, a[2], 4, a[3], a[4], a[5], a[6], N) == -1
    # nn_fallback: query, n_query, ref, n_ref, fallback_list, status, dist, index, stream
    assert h.i2sdf_points_nn_fallback(P, 0, P, 8, P, P, P, P, N) == 0
    assert h.i2sdf_points_nn_fallback(P, -1, P, 8, P, P, P, P, N) == -1
    assert h.i2sdf_points_nn_fallback(P, 8, P, 0, P, P, P, P, N) == -1
    for k in range(6):
        a = [P] * 6
        a[k] = N
        assert h.i2sdf_points_nn_fallback(a[0], 8, a[1], 8, a[2], a[3], a[4], a[5], N) == -1
    # threshold_reduce: dist, n, threshold, workspace, out, stream
    for n in (0, -1, INT32_MAX + 1):
        assert h.i2sdf_points_threshold_reduce(P, n, 0.05, P, P, N) == -1
    assert h.i2sdf_points_threshold_reduce(P, 8, float("nan"), P, P, N) == -1
    for k in range(3):
        a = [P] * 3
        a[k] = N
        assert h.i2sdf_points_threshold_reduce(a[0], 8, 0.05, a[1], a[2], N) == -1
