"""CPU: the sphere-tracing entry points of the C ABI (i2sdf_trace_*, csrc/mlp_trace.hip) on the cross-compiled library: declared, exported
and bound; every refusal include/i2sdf.h lists answered on the host with I2SDF_EINVAL and a reason before any launch (a launch without a
device would return the HIP error code -2, not -1); and the Python layer (RenderEngine.trace_rays' argument checks, I2SDFNetwork.trace_surface /
render_surface / sphere_tracer / get_incident_radiance) refusing what it must without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = ["i2sdf_trace_workspace_floats", "i2sdf_trace_rays"]


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_trace_[a-z0-9_]+)\s*\(", text)) == set(TRACE)
    raw = C.CDLL(lib.LIB_PATH)
    for s in TRACE:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "mlp_trace.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    # the constants of the header and their Python twins
    for name, val in (("HIT", lib.TRACE_HIT), ("MISS", lib.TRACE_MISS), ("UNRESOLVED", lib.TRACE_UNRESOLVED), ("INSIDE", lib.TRACE_INSIDE),
                      ("AUTO", lib.TRACE_ROUTES["auto"]), ("STEPWISE", lib.TRACE_ROUTES["stepwise"]), ("FUSED", lib.TRACE_ROUTES["fused"]),
                      ("MAX_STEPS", lib.TRACE_MAX_STEPS)):
        assert int(re.search(r"#define I2SDF_TRACE_%s (\d+)" % name, text).group(1)) == val, name
    assert (lib.TRACE_HIT, lib.TRACE_MISS, lib.TRACE_UNRESOLVED, lib.TRACE_INSIDE) == (1, 2, 3, 4)
    assert C.sizeof(lib.TraceCfg) == 16
    import i2sdf_amd
    assert callable(i2sdf_amd.SphereTracer) and callable(i2sdf_amd.RenderEngine.trace_rays)
    for m in ("trace_surface", "render_surface", "sphere_tracer"):
        assert callable(getattr(i2sdf_amd.I2SDFNetwork, m))


def test_workspace_query(lib):
    h = lib.load()
    ws = lambda n: int(h.i2sdf_trace_workspace_floats(n))
    assert ws(-1) == 0 and ws(0) == 0 and ws(1) >= 1 and ws(389) >= 389 and ws(1 << 20) >= ws(1 << 19)


def test_bad_arguments_return_einval_with_a_reason_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None
    why = lambda: h.i2sdf_last_hip_error().decode()

    def call(plan=P, packed=P, cfg="ok", cam=P, dirs=P, t_min=P, t_max=P, n=8, t=P, status=P, steps=P, f=N, ws=P, **c):
        kw = dict(eps=1e-4, step_scale=1.0, max_steps=64, route=0)
        kw.update(c)
        cfg_p = C.byref(lib.TraceCfg(**kw)) if cfg == "ok" else None
        return h.i2sdf_trace_rays(plan, packed, cfg_p, cam, dirs, t_min, t_max, n, t, status, steps, f, ws, N)

    assert call(n=0) == 0                                                    # nothing to do, nothing launched
    assert call(n=0, f=P) == 0
    inf, nan = float("inf"), float("nan")
    for kw, word in ((dict(eps=0.0), "eps"), (dict(eps=-1e-4), "eps"), (dict(eps=inf), "eps"), (dict(eps=nan), "eps"),
                     (dict(step_scale=0.0), "step_scale"), (dict(step_scale=-0.5), "step_scale"), (dict(step_scale=1.0001), "step_scale"),
                     (dict(step_scale=nan), "step_scale"), (dict(step_scale=inf), "step_scale"),
                     (dict(max_steps=0), "max_steps"), (dict(max_steps=-3), "max_steps"), (dict(max_steps=1025), "max_steps"),
                     (dict(route=3), "route"), (dict(route=-1), "route"),
                     (dict(n=-1), "N"), (dict(cfg=None), "cfg"), (dict(plan=N), "plan")):
        for n0 in ({}, {"n": 0}) if "n" not in kw else ({},):                # a bad configuration is refused for an empty batch too
            assert call(**kw, **n0) == -1, kw
            assert word in why(), (kw, why())
    for name in ("packed", "cam", "dirs", "t_min", "t_max", "t", "status", "steps", "ws"):
        assert call(**{name: N}) == -1, name
        assert "NULL" in why(), (name, why())
    # the limits themselves are inside
    for kw in (dict(step_scale=1.0, max_steps=1024, n=0), dict(step_scale=1e-3, max_steps=1, n=0), dict(eps=1e-30, n=0), dict(route=1, n=0)):
        assert call(**kw) == 0, kw
    assert call(n=1 << 31) == -1 and "2^31" in why()
    # (route 2 on a plan without a fused kernel reads the plan, which needs a device to exist: tests/test_gpu_trace.py)
    assert call(route=2, plan=N) == -1 and "plan" in why()


def test_python_front_end_refuses_without_a_gpu():
    import torch
    import i2sdf_amd as A
    from i2sdf_amd import trace as T
    z = torch.zeros(5, 3)
    # the configuration
    for kw, word in ((dict(eps=0.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps="1e-4"), "eps"), (dict(step_scale=0.0), "step_scale"),
                     (dict(step_scale=1.5), "step_scale"), (dict(max_steps=0), "max_steps"), (dict(max_steps=1025), "max_steps"),
                     (dict(max_steps=2.5), "max_steps"), (dict(route="fastest"), "route")):
        with pytest.raises(ValueError, match=word):
            T.check_trace_cfg(**kw)
    cfg = T.check_trace_cfg(eps=1e-3, max_steps=7, step_scale=0.5, route="stepwise")
    assert (cfg.max_steps, cfg.route) == (7, 1) and abs(cfg.eps - 1e-3) < 1e-9 and cfg.step_scale == 0.5
    # the rays
    for args, word in (((torch.zeros(5, 2), z, 0.0, 1.0), "cam_loc"), ((z, torch.zeros(4, 3), 0.0, 1.0), "differ"), ((z, z.long(), 0.0, 1.0), "dirs"),
                       ((z, z, torch.zeros(4), 1.0), "t_min"), ((z, z, 0.0, torch.zeros(5, 1)), "t_max"), ((z, z, 0.0, torch.zeros(5).long()), "t_max")):
        with pytest.raises(ValueError, match=word):
            T.check_trace_rays(*args)
    with pytest.raises(TypeError, match="t_min"):
        T.check_trace_rays(z, z, None, 1.0)
    with pytest.raises(TypeError, match="cam_loc"):
        T.check_trace_rays([[0.0, 0.0, 0.0]], z, 0.0, 1.0)
    cam, dirs, t0, t1 = T.check_trace_rays(z.double(), z, 0.25, torch.arange(5.0))
    assert cam.dtype == torch.float32 and tuple(t0.shape) == tuple(t1.shape) == (5,) and float(t0[3]) == 0.25 and float(t1[3]) == 3.0
    # the module
    net = A.I2SDFNetwork(A.plumbing_conf())
    rays = {"uv": z, "rays": {"cam_loc": z, "dirs": z, "dnorm": torch.ones(5)}}
    for fn in (net.trace_surface, net.render_surface):
        with pytest.raises(RuntimeError, match="MI355X"):                  # valid arguments: only the device is missing
            fn(rays)
        with pytest.raises(ValueError, match="max_steps"):
            fn(rays, max_steps=0)
        with pytest.raises(ValueError, match="rays"):
            fn({"uv": z, "rays": {"cam_loc": z, "dirs": z}})
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            fn({"uv": z, "rays": {"cam_loc": z, "dirs": torch.zeros(4, 3), "dnorm": torch.ones(5)}})
        with pytest.raises(ValueError, match="pose"):
            fn({"uv": torch.zeros(1, 5, 2)})
        with pytest.raises(ValueError, match="input"):
            fn(z)
    with pytest.raises(ValueError, match="split_n_pixels"):
        net.render_surface(rays, split_n_pixels=0)
    assert net.training                                                     # a refused call leaves the module's mode alone
    # tracers
    with pytest.raises(ValueError, match="eps"):
        net.sphere_tracer(eps=-1.0)
    with pytest.raises(TypeError, match="unknown"):
        net.sphere_tracer(tolerance=1.0)
    tracer = net.sphere_tracer(max_steps=32)
    assert isinstance(tracer, A.SphereTracer) and tracer.net is net and tracer.kw == {"max_steps": 32}
    with pytest.raises(RuntimeError, match="MI355X"):                      # this module's tracer is accepted: only the device is missing
        net.get_incident_radiance(z, z, intersect_func=tracer)
    other = A.I2SDFNetwork(A.plumbing_conf())
    for bad in (lambda *a: None, other.sphere_tracer(), "tracer", 1):
        with pytest.raises(NotImplementedError, match="intersect_func"):
            net.get_incident_radiance(z, z, intersect_func=bad)
