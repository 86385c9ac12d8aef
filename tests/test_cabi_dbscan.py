"""CPU: the density-clustering entry points of the C ABI (i2sdf_dbscan_*, csrc/dbscan.hip) on the cross-compiled library: declared,
exported and bound; the size query monotone, a multiple of 16, within its cap and 0 for what is not supported; bad arguments refused on
the host before any launch (no call below reaches a launch: a launch without a device would return the HIP error code -2, not -1); the
Python front end refuses CPU tensors and bad shapes; and the kernels use no scratch and stay within the streaming kernels' register
budget, read off the in-tree build the way tests/test_cabi_kmeans.py reads kmeans.o."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBSCAN = ["i2sdf_dbscan_workspace_bytes", "i2sdf_dbscan_cell_keys", "i2sdf_dbscan_label"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    assert "Density clustering" in text and "RESTATEMENT" in text and "where the library was importable" in text
    for name, bit in (("I2SDF_DBSCAN_NONFINITE", lib.DBSCAN_NONFINITE), ("I2SDF_DBSCAN_CELLS", lib.DBSCAN_CELLS)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == bit
    assert (lib.DBSCAN_NONFINITE, lib.DBSCAN_CELLS) == (1, 2)              # status bits 0 and 1
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_dbscan_[a-z0-9_]+)\s*\(", text)) == set(DBSCAN)
    raw = C.CDLL(lib.LIB_PATH)
    for s in DBSCAN:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "dbscan.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    assert callable(i2sdf_amd.DBSCAN) and callable(i2sdf_amd.DBSCAN.fit_predict) and callable(i2sdf_amd.dbscan_seeds)
    assert isinstance(i2sdf_amd.DBSCAN.core_sample_indices_, property)
    db = i2sdf_amd.DBSCAN()
    assert (db.eps, db.min_samples) == (0.5, 5)                            # the library's defaults
    assert db.labels_ is None and db.core_sample_mask_ is None and db.n_clusters_ is None and db.status_ is None


def test_workspace_query(lib):
    h = lib.load()
    ws = lambda n: int(h.i2sdf_dbscan_workspace_bytes(n))
    sizes = [1, 2, 3, 15, 16, 17, 63, 64, 65, 1000, 1023, 1024, 1025, 4099, 1 << 20, (1 << 20) + 1, 1 << 24, (1 << 30) + 5, (1 << 31) - 1]
    got = [ws(n) for n in sizes]
    assert all(g > 0 and g % 16 == 0 for g in got), got
    assert all(b >= a for a, b in zip(got, got[1:])) and got[-1] > got[0]
    assert all(g <= 96 * n + 65536 for n, g in zip(sizes, got)), [(n, g) for n, g in zip(sizes, got) if g > 96 * n + 65536]
    dense = [ws(n) for n in range(1, 3000)]
    assert all(g % 16 == 0 and g <= 96 * n + 65536 for n, g in zip(range(1, 3000), dense)) and all(b >= a for a, b in zip(dense, dense[1:]))
    for bad in (0, -1, -(1 << 40), 1 << 31, (1 << 31) + 1, 1 << 40):
        assert ws(bad) == 0, bad


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    ODD16, ODD8, ODD4 = C.c_void_p(4104), C.c_void_p(4100), C.c_void_p(4098)
    bad_n = (dict(n=0), dict(n=-1), dict(n=1 << 31), dict(n=1 << 40))
    bad_eps = (dict(eps=0.0), dict(eps=-0.5), dict(eps=math.nan), dict(eps=math.inf), dict(eps=-math.inf), dict(eps=1e200), dict(eps=1e-200))

    # points, n, eps, workspace, keys, status, stream
    def keys(pts=P, n=1000, eps=0.5, ws=P, keys=P, status=P):
        return h.i2sdf_dbscan_cell_keys(pts, n, eps, ws, keys, status, N)

    for kw in bad_n + bad_eps + (dict(pts=N), dict(pts=ODD4), dict(ws=N), dict(ws=ODD16), dict(ws=ODD8), dict(keys=N), dict(keys=ODD8),
                                 dict(status=N), dict(status=ODD4)):
        assert keys(**kw) == -1, kw

    # points, n, eps, min_samples, sorted_keys, perm, workspace, labels, core, n_clusters, status, stream
    def label(pts=P, n=1000, eps=0.5, min_samples=5, skeys=P, perm=P, ws=P, labels=P, core=P, n_clusters=P, status=P):
        return h.i2sdf_dbscan_label(pts, n, eps, min_samples, skeys, perm, ws, labels, core, n_clusters, status, N)

    for kw in bad_n + bad_eps + (dict(min_samples=0), dict(min_samples=-1), dict(min_samples=-(1 << 31)), dict(pts=N), dict(pts=ODD4),
                                 dict(skeys=N), dict(skeys=ODD8), dict(perm=N), dict(perm=ODD8), dict(ws=N), dict(ws=ODD16), dict(ws=ODD8),
                                 dict(labels=N), dict(labels=ODD8), dict(core=N), dict(n_clusters=N), dict(n_clusters=ODD4),
                                 dict(status=N), dict(status=ODD4)):
        assert label(**kw) == -1, kw


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    pts = torch.zeros(16, 3)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.DBSCAN().fit_predict(pts)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.dbscan_seeds(pts, 2, route="device")
    for bad in (torch.zeros(16, 2), torch.zeros(16, 3, dtype=torch.float64), torch.zeros(16), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match=r"expected \(n, 3\) float32"):
            A.DBSCAN().fit_predict(bad)
        with pytest.raises(ValueError, match=r"expected \(n, 3\) float32"):
            A.dbscan_seeds(bad, 2, route="device")
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=math.nan), dict(eps=math.inf), dict(min_samples=0), dict(min_samples=-3),
               dict(min_samples=2.5), dict(min_samples=1 << 31)):
        with pytest.raises(ValueError):
            A.DBSCAN(**kw)
    with pytest.raises(RuntimeError, match="nothing fitted"):
        A.DBSCAN().core_sample_indices_
    with pytest.raises(ValueError, match="route"):
        A.dbscan_seeds(pts, 2, route="gpu")
    net = A.I2SDFNetwork(A.plumbing_conf())
    for bad in ("nonsense", "host", 1, 0, None):
        with pytest.raises(ValueError, match="use_dbscan"):
            net.init_emission_groups(2, pts, use_dbscan=bad)
    with pytest.raises(I2SDFError, match="no CPU path"):
        net.init_emission_groups(2, pts, use_dbscan="device")
    assert not hasattr(net, "emissions") and "emissions" not in net.state_dict()      # a refused call leaves the module as it was


def test_dbscan_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "dbscan.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/dbscan.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("dbscan.hip", "unionfind.h", "blockops.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("db_keys_kernel", "db_status_kernel", "db_gather_kernel", "db_cells_kernel", "db_core_kernel", "db_pairs_kernel",
            "db_roots_kernel", "db_labels_kernel", "scan_reduce_kernel", "scan_chunks_kernel")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in dbscan.o"
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"
        assert res["vgpr"] <= 128, (name, res)                             # streaming kernels: room for 4 waves per SIMD
