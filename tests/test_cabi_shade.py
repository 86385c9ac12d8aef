"""CPU: the shading entry points of the C ABI (i2sdf_shade_*, csrc/shade.hip) on the cross-compiled library: declared, exported and bound;
every refusal include/i2sdf.h lists answered on the host with I2SDF_EINVAL and a reason, before any launch (no call below reaches a launch:
a launch without a device would return the HIP error code -2, not -1); the new kernels use no scratch, read off the in-tree build the way
tests/test_cabi_bubble.py does; and the Python front end refuses what it must without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADE = ["i2sdf_shade_draws", "i2sdf_shade_sample", "i2sdf_shade_reduce", "i2sdf_shade_backward_workspace_bytes", "i2sdf_shade_backward"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_shade_[a-z0-9_]+)\s*\(", text)) == set(SHADE)
    raw = C.CDLL(lib.LIB_PATH)
    for s in SHADE:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "shade.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    assert callable(i2sdf_amd.RenderingLayer) and callable(i2sdf_amd.get_rendering_parameters) and callable(i2sdf_amd.shade_draws)
    assert callable(i2sdf_amd.I2SDFNetwork.get_incident_radiance)


def test_workspace_query(lib):
    h = lib.load()
    ws = lambda bn, spp: int(h.i2sdf_shade_backward_workspace_bytes(bn, spp))
    assert ws(0, 1) > 0 and ws(4096, 64) % 16 == 0
    assert ws(4096, 64) >= 4096 // 4 * 12 and ws(4096, 1) >= 4096 // 256 * 12          # three floats per workgroup
    assert ws(1 << 20, 64) >= ws(4096, 64)
    for bad in ((-1, 4), (4, 0), (4, -1), (1 << 31, 1), (1 << 25, 64), (1 << 40, 8)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_return_einval_with_a_reason_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    seed = C.byref(C.c_uint64(7))
    why = lambda: h.i2sdf_last_hip_error().decode()

    def sample(x=P, v=P, n=P, kd=P, ks=P, r=P, u=N, s=seed, bn=8, spp=4, d=P, p=P, m=P):
        return h.i2sdf_shade_sample(x, v, n, kd, ks, r, u, s, bn, spp, d, p, m, N)

    def reduce(v=P, n=P, kd=P, ks=P, r=P, u=N, s=seed, rad=P, sc=N, bn=8, spp=4, cd=P, cs=P):
        return h.i2sdf_shade_reduce(v, n, kd, ks, r, u, s, rad, sc, bn, spp, cd, cs, N)

    def backward(v=P, n=P, kd=P, ks=P, r=P, u=N, s=seed, rad=P, sc=N, gcd=P, gcs=P, gd=N, gp=N, bn=8, spp=4, ws=P, gkd=P, gks=P, gr=P,
                 grad=N, gsc=N):
        return h.i2sdf_shade_backward(v, n, kd, ks, r, u, s, rad, sc, gcd, gcs, gd, gp, bn, spp, ws, gkd, gks, gr, grad, gsc, N)

    sizes = (dict(bn=-1), dict(spp=0), dict(spp=-3), dict(bn=1 << 31, spp=1), dict(bn=1 << 25, spp=64), dict(bn=1 << 40))
    source = (dict(u=P), dict(s=None))                                   # both samples and seed; neither
    for fn, ptrs in ((sample, ("x", "v", "n", "kd", "ks", "r", "d", "p", "m")), (reduce, ("v", "n", "kd", "ks", "r", "rad", "cd", "cs")),
                     (backward, ("v", "n", "kd", "ks", "r", "gr"))):
        assert fn(bn=0) == 0                                             # nothing to do, nothing launched
        for kw in sizes + source + tuple({k: N} for k in ptrs):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert why(), (fn.__name__, kw)
    assert sample(spp=0) == -1 and "spp < 1" in why()
    assert sample(u=P) == -1 and "both" in why()
    assert sample(s=None) == -1 and "neither" in why()
    assert sample(bn=1 << 25, spp=64) == -1 and "2^31" in why()
    # the backward's two groups of upstream gradients
    for kw in (dict(gcd=N), dict(gcs=N), dict(rad=N), dict(gkd=N), dict(gks=N),          # the colour group goes together
               dict(gcd=N, gcs=N),                                                      # no upstream gradient at all
               dict(gcd=N, gcs=N, gd=P, grad=P), dict(gcd=N, gcs=N, gd=P, gsc=P),       # radiance gradients need the colour group
               dict(gsc=P, ws=N)):                                                      # the scale gradient needs the workspace
        assert backward(**kw) == -1, kw
        assert why(), kw
    assert backward(bn=0, gcd=N, gcs=N, gd=P, rad=N, gkd=N, gks=N) == 0                  # the ray group alone is a valid call
    # draws: seed, bn, spp, samples, stream
    assert h.i2sdf_shade_draws(1, 0, 4, P, N) == 0
    for bn, spp, out in ((-1, 4, P), (4, 0, P), (1 << 31, 1, P), (4, 4, N)):
        assert h.i2sdf_shade_draws(1, bn, spp, out, N) == -1, (bn, spp, out)


def test_python_front_end_refuses_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd.lib import I2SDFError
    layer = A.RenderingLayer(4, 100)
    z = torch.zeros(5, 3)
    with pytest.raises(I2SDFError):
        layer(None, z, z, z, z, z, torch.zeros(5, 1))
    with pytest.raises(ValueError, match="h, w"):
        layer(None, z, z, z, z, torch.zeros(5, 3, 2, 2), torch.zeros(5, 1))
    with pytest.raises(I2SDFError):
        A.shade_draws(1, 4, 4, device="cpu")
    net = A.I2SDFNetwork(A.plumbing_conf())
    with pytest.raises(NotImplementedError, match="intersect_func"):
        net.get_incident_radiance(z, z, intersect_func=lambda *a: None)


def test_shade_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _kernels_of, OBJ, CSRC, LLVM
    obj = os.path.join(OBJ, "shade.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/shade.o) or no LLVM binutils")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("shade.hip", "brdf_dev.h", "philox.h")):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    want = ("shade_draws_kernel", "shade_sample_kernel", "shade_reduce_kernel", "shade_backward_kernel", "shade_scale_sum_kernel")
    for frag in want:
        assert any(frag in name for name in kernels), f"{frag} not found in shade.o"
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"
        # the forward kernels leave room for 4 waves per SIMD and more, the backward (a value and a tangent per quantity) for 3
        assert res["vgpr"] <= (168 if "shade_backward_kernel" in name else 128), (name, res)
