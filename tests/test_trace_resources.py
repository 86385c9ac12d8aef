"""CPU: register / scratch budget of the sphere-tracing kernels (csrc/mlp_trace.hip), read from the in-tree build as
tests/test_kernel_resources.py reads the others.  The fused kernels wrap the layer chain of the bf16x3 sdf-only forwards in the marching loop;
the 256-wide one belongs to the two-waves-per-SIMD family and sits at its 256-register cap: a ray's state kept in registers across the chain,
or the unit built with SLP vectorisation, tips it into scratch."""
import os

import pytest

from test_kernel_resources import CSRC, LLVM, OBJ, _kernels_of


def test_trace_kernels_use_no_scratch(tmp_path):
    obj = os.path.join(OBJ, "mlp_trace.o")
    if not os.path.exists(obj) or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("no in-tree build (i2sdf_amd/lib/obj/mlp_trace.o) or no LLVM binutils")
    srcs = ("mlp_trace.hip", "trace_rule.h", "x3.h", "x3h.h", "common.h", "mlp_common.h", "mlp_args.h")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in srcs):
        pytest.skip("in-tree object is older than the source: run __graft_entry__.build()")
    kernels = _kernels_of(obj, str(tmp_path))
    for frag in ("trace_init_kernel", "trace_step_kernel", "sdf_trace3_kernel", "sdf_trace3h_kernel"):
        assert any(frag in name for name in kernels), f"{frag} not found in mlp_trace.o"
    for name, res in kernels.items():
        assert res["scratch"] == 0, f"{name}: {res['scratch']} B of scratch per lane: {res}"
        if "sdf_trace3h_kernel" in name:
            assert res["vgpr"] <= 256, (name, res)
        elif "sdf_trace3_kernel" in name:
            assert res["vgpr"] + res["agpr"] <= 512, (name, res)
        else:
            assert res["vgpr"] <= 64, (name, res)
