"""CPU: the clustering entry points of the C ABI (i2sdf_kmeans_*, csrc/kmeans.hip) on the cross-compiled library: declared, exported and
bound; the size query monotone and 0 for what is not supported; bad arguments refused on the host before any launch (no call below reaches
a launch: a launch without a device would return the HIP error code -2, not -1); the Python front end refuses CPU tensors; and the
kernels use no scratch and stay within the streaming kernels' register budget, read off the in-tree build the way
tests/test_cabi_bubble.py reads bubble.o."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMEANS = ["i2sdf_kmeans_workspace_bytes", "i2sdf_kmeans_pp", "i2sdf_kmeans_fit", "i2sdf_kmeans_assign"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    m = re.search(r"#define\s+I2SDF_KMEANS_MAX_K\s+(\d+)", text)
    assert m and int(m.group(1)) == lib.KMEANS_MAX_K == 256
    assert "has NOT been checked against the library" in text            # the Lloyd rule is a restatement: the header says so
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_kmeans_[a-z0-9_]+)\s*\(", text)) == set(KMEANS)
    raw = C.CDLL(lib.LIB_PATH)
    for s in KMEANS:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "kmeans.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    assert callable(i2sdf_amd.kmeans_pp_centroid) and callable(i2sdf_amd.KMeans)
    for name in ("fit_predict", "predict"):
        assert callable(getattr(i2sdf_amd.KMeans, name)), name
    assert isinstance(i2sdf_amd.KMeans.centroids, property) and i2sdf_amd.KMeans.centroids.fset is not None
    assert callable(i2sdf_amd.I2SDFNetwork.init_emission_groups)


def test_workspace_query(lib):
    h = lib.load()
    ws = lambda n, k: int(h.i2sdf_kmeans_workspace_bytes(n, k))
    by_k = [ws(1 << 20, k) for k in range(1, 257)]
    assert all(g > 0 and g % 16 == 0 for g in by_k) and all(b >= a for a, b in zip(by_k, by_k[1:])) and by_k[-1] > by_k[0]
    by_n = [ws(n, 8) for n in (8, 9, 100, 4099, 1 << 20, (1 << 31) - 1)]
    assert all(g > 0 and g % 16 == 0 for g in by_n) and all(b >= a for a, b in zip(by_n, by_n[1:])) and by_n[2] > by_n[0]
    assert ws(1 << 20, 16) < 4 * (1 << 20) + (1 << 14)                     # the distances (4 B a point) and O(k) state, nothing (k, n)-sized
    assert ws(1, 1) > 0 and ws(256, 256) > 0
    for bad in ((0, 1), (-1, 1), (10, 0), (10, -1), (10, 11), (1000, 257), (1 << 31, 8), (1 << 40, 8), (255, 256)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N, ODD = C.c_void_p(4096), None, C.c_void_p(4100)

    # points, n, k, seed, workspace, idx_out, centroids_out, stream
    def pp(pts=P, n=1000, k=8, ws=P, idx=P, cent=P):
        return h.i2sdf_kmeans_pp(pts, n, k, 1, ws, idx, cent, N)

    sizes = (dict(k=0), dict(k=-1), dict(k=257), dict(k=8, n=7), dict(n=0), dict(n=-1), dict(n=1 << 31), dict(n=1 << 40))
    for kw in sizes + (dict(pts=N), dict(ws=N), dict(ws=ODD), dict(idx=N), dict(cent=N)):
        assert pp(**kw) == -1, kw

    # points, n, k, centroids, max_iter, tol, workspace, labels, n_iter, stream
    def fit(pts=P, n=1000, k=8, cent=P, max_iter=100, tol=1e-4, ws=P, labels=P, n_iter=P):
        return h.i2sdf_kmeans_fit(pts, n, k, cent, max_iter, tol, ws, labels, n_iter, N)

    for kw in sizes + (dict(pts=N), dict(cent=N), dict(ws=N), dict(ws=ODD), dict(labels=N), dict(n_iter=N), dict(max_iter=0),
                       dict(max_iter=-3), dict(tol=-1e-9), dict(tol=math.nan), dict(tol=-math.inf)):
        assert fit(**kw) == -1, kw

    # points, n, centroids, k, labels, dist2, stream
    def assign(pts=P, n=1000, cent=P, k=8, labels=P, d2=P):
        return h.i2sdf_kmeans_assign(pts, n, cent, k, labels, d2, N)

    assert assign(n=0) == 0 and assign(n=0, pts=N, labels=N) == 0          # nothing to label: a no-op
    # k > n is refused by _pp and _fit (above) and deliberately NOT by _assign: predict on a few new points against many centroids.
    # n = 0 with k = 8 shows it here without a launch; the header says so and tests/test_gpu_kmeans.py::test_rules runs k = 5 on 2 points
    assert assign(n=0, k=8) == 0 and pp(n=0, k=8) == -1 and fit(n=0, k=8) == -1
    assert "Here k may exceed n" in open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    for kw in (dict(k=0), dict(k=-1), dict(k=257), dict(n=-1), dict(n=1 << 31), dict(n=1 << 40), dict(n=0, k=0), dict(pts=N), dict(cent=N),
               dict(labels=N)):
        assert assign(**kw) == -1, kw


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    pts = torch.zeros(16, 3)
    with pytest.raises(I2SDFError, match="no CPU path"):
        A.kmeans_pp_centroid(pts, 2)
    km = A.KMeans(2)
    with pytest.raises(I2SDFError, match="no CPU path"):
        km.fit_predict(pts)
    with pytest.raises(I2SDFError, match="no CPU path"):
        km.centroids = torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no centroids"):
        km.predict(pts)
    for bad in (torch.zeros(16, 2), torch.zeros(16, 3, dtype=torch.float64), torch.zeros(16), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match=r"expected \(n, 3\) float32"):
            A.kmeans_pp_centroid(bad, 2)
    for k in (0, 257):
        with pytest.raises(ValueError):
            A.KMeans(k)
    with pytest.raises(ValueError):
        A.KMeans(2, max_iter=0)
    with pytest.raises(ValueError):
        A.KMeans(2, tol=-1.0)
    net = A.I2SDFNetwork(A.plumbing_conf())
    with pytest.raises(I2SDFError, match="no CPU path"):
        net.init_emission_groups(2, pts)
    assert not hasattr(net, "emissions") and "emissions" not in net.state_dict()      # a refused call leaves the module as it was


def test_kmeans_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "kmeans.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/kmeans.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("kmeans.hip", "philox.h", "blockops.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("kmeans_pp_first_kernel", "kmeans_pp_round_kernel", "kmeans_pp_emit_kernel", "kmeans_range_kernel", "kmeans_assign_kernel",
            "kmeans_update_kernel", "kmeans_fit_begin_kernel")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in kmeans.o"
    assert sum("kmeans_assign_kernel" in name for name in kernels) == 2     # with and without the per-cluster sums
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"
        assert res["vgpr"] <= 128, (name, res)                             # streaming kernels: room for 4 waves per SIMD
