"""CPU: the sizes callers allocate workspaces by.  tests/golden/workspace_bytes.json holds what every `*_workspace_bytes` entry point
of the geometry translation units returned BEFORE their scans and reductions moved into csrc/blockops.h, for a fixed list of
arguments: the sizes at which a scan level appears (1024 items per workgroup per level), ordinary ones, and one refused argument
each.  The library must still return exactly those -- with one exception: i2sdf_mesh_scan_workspace_bytes lost a redundant
one-element top level, so it may return less than the record, never more, and 0 exactly where 0 was recorded.

(Recorded with `I2SDF_LIB_PATH=<a build of that commit> python tests/test_cabi_workspace.py record`.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")

K = 1024                     # items per scan workgroup
ARGS = {
    # 256 points per block pair: one scan level up to 1024 blocks (64^3 points), two up to 1024^2 blocks (2^28 points), then three
    "i2sdf_marching_cubes_workspace_bytes": [(2, 2, 2), (16, 16, 16), (17, 33, 9), (64, 64, 64), (64, 64, 65), (131, 97, 331), (256, 256, 256),
                                             (1024, 512, 512), (1024, 512, 513), (2048, 2048, 2048), (1, 5, 5), (16384, 16384, 2048)],
    "i2sdf_mesh_scan_workspace_bytes": [(0,), (1,), (255,), (256,), (257,), (K - 1,), (K,), (K + 1,), (2 * K,), (2 * K + 1,), (K * K,), (K * K + 1,),
                                        (2_000_003,), (K * K * K,), (K * K * K + 1,), (2 ** 31 - 1,), (2 ** 31,), (-1,)],
    "i2sdf_depth_unproject_workspace_bytes": [(0, 4, 4), (1, 1, 1), (1, 32, 32), (1, 32, 33), (3, 480, 640), (257, 1024, 1024), (-1, 4, 4),
                                              (1, 0, 4), (2 ** 20, 1024, 1024)],
    "i2sdf_tsdf_extract_workspace_bytes": [(1,), (7,), (4096,), (2 ** 24,), (0,), (2 ** 24 + 1,)],
    "i2sdf_points_reduce_workspace_bytes": [(1,), (K,), (K + 1,), (K * K,), (K * K + 1,), (2 ** 31 - 1,), (0,), (2 ** 31,)],
    "i2sdf_image_workspace_bytes": [(1, 1, 1), (1, 11, 11), (1, 10, 64), (2, 32, 32), (3, 480, 640), (1, 26, 42), (1, 27, 43), (65535, 16, 16),
                                    (0, 16, 16), (65536, 16, 16), (1, 0, 16)],
    "i2sdf_kmeans_workspace_bytes": [(1, 1), (5, 5), (1000, 3), (K * K + 1, 256), (2 ** 31 - 1, 256), (4, 5), (100, 257), (0, 1), (2 ** 31, 2)],
    "i2sdf_bubble_sample_workspace_bytes": [(1,), (2,), (1000,), (0,), (2 ** 40,)],
    "i2sdf_shade_backward_workspace_bytes": [(0, 1), (1, 1), (256, 1), (257, 1), (1000, 64), (1000, 100), (2 ** 20, 128), (-1, 4), (4, 0), (2 ** 31, 1)],
}


def _table(handle):
    return {name: [[list(a), int(getattr(handle, name)(*a))] for a in rows] for name, rows in ARGS.items()}


@pytest.fixture(scope="module")
def handle():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L.load()


def test_workspace_sizes_are_the_recorded_ones(handle):
    want = json.load(open(TABLE))
    got = _table(handle)
    assert sorted(want) == sorted(ARGS)
    for name, rows in got.items():
        assert [a for a, _ in rows] == [a for a, _ in want[name]], f"{name}: the recorded argument list is not this test's"
        assert any(b == 0 for _, b in want[name]) and any(b > 0 for _, b in want[name]), name      # a refused argument, an accepted one
        for (a, new), (_, old) in zip(rows, want[name]):
            if name == "i2sdf_mesh_scan_workspace_bytes" and old > 0:
                assert 0 < new <= old, f"{name}{tuple(a)} = {new}, recorded {old}"
            else:
                assert new == old, f"{name}{tuple(a)} = {new}, recorded {old}"


def test_mesh_scan_levels(handle):
    """8 bytes per chunk sum, one more level whenever a level no longer fits one workgroup; never below 16 bytes."""
    f = handle.i2sdf_mesh_scan_workspace_bytes
    assert f(0) == f(1) == f(K) == f(2 * K) == 16
    assert f(2 * K + 1) == 8 * 3 and f(K * K) == 8 * K
    assert f(K * K + 1) == 8 * (K + 1) + 8 * 2
    assert f(K * K * K + 1) == 8 * (K * K + 1) + 8 * (K + 1) + 8 * 2


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    sys.path.insert(0, ROOT)
    from i2sdf_amd import lib as L
    with open(TABLE, "w") as fh:                  # one line per entry point
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in _table(L.load()).items()) + "\n}\n")
    print(f"recorded {TABLE} from {L.LIB_PATH}")
