"""GPU: sphere tracing of the SDF (include/i2sdf.h: i2sdf_trace_rays; RenderEngine.trace_rays; I2SDFNetwork.trace_surface / render_surface /
sphere_tracer) on the plumbing, plumbing-with-skip and synthetic.yml nets (init_params(seed=3), perturb_params(0.05)).

Rays (tests/trace_ref.py: make_rays): origins on radii 1.5..2.5 aimed into the cube of +-0.9, interval [0, exit of the bounding sphere].
Sizes 1, 37, 133 (a partial 128-ray tile behind a full one) and 389: three tiles and a bit, the second tile all misses, the third one
grazing ray among misses.  max_steps 1, 2 (a ray cut off at every possible place) and 64.

What is held:
  1. replay     the fp32 rule of tests/trace_ref.py run on the device's own f_trace reproduces t, status, steps bit for bit, and f_trace is
                written exactly where the rule takes a step;
  2. f is sdf   every written f_trace entry is, bit for bit, implicit_network.get_sdf_vals at o + t d of that step (the point rebuilt on the
                device as the kernels form it -- ONE rounding per component, see _point); implicit_network(x)[:, 0], another kernel, agrees
                at that route's own 1e-5;
  3. routes     every route the plan has gives the same bits, twice; canaries around every output and the workspace stay intact;
  4. fp64       against the fp64 tracer on the fp64 oracle net, 1500 rays per net: status differs on <= 1 % of the rays; >= 90 % of the
                common hits are well posed (|d . grad sdf| >= 0.2 at the fp64 hit); for those |t - t_ref| <= (2 eps + 2 delta) / |d . grad sdf|
                -- both tracers stop within eps of zero of THEIR sdf, the two sdf differ by at most delta, and the slope converts that to t.
                delta = 1e-5 max|sdf| over the cube of +-2.5: the bar tests/test_gpu_sdf_forward.py holds these forward kernels to.
                Measured on the MI355X, the same figures on both routes (their bits agree): status differs on 0 of 1500 rays on every
                net; common hits 417 / 661 / 485 (plumbing / plumbing_skip / synthetic), 98.1 / 95.6 / 96.1 % of them well posed; largest
                used fraction of the bound 0.149 / 0.131 / 0.0034 (median 2e-4 .. 3e-4); delta 5.4e-5 / 4.3e-5 / 4.2e-5; every hit within
                63 steps, 5 / 6 / 6 grazing rays UNRESOLVED after 64.
  5. surface    trace_surface / render_surface against the public routes at o + t d; exact zeros without a hit; both radiance modes;
  6. get_incident_radiance(pts, dirs, intersect_func=net.sphere_tracer()) is render_surface;  7. a lambda is still refused."""
import numpy as np
import pytest
import torch

import idr_ref
import trace_ref as TR
from helpers import assert_close
from oracle import i2sdf_oracle as orc

pytestmark = pytest.mark.gpu

NETS = ("plumbing", "plumbing_skip", "synthetic")
SIZES = (1, 37, 133, 389)
STEPS = (1, 2, 64)
CANARY = 64
_CACHE = {}


def _ocfg(which):
    return orc.synthetic_cfg() if which == "synthetic" else orc.plumbing_cfg(skip=which.endswith("skip"))


def _weights(which):
    return orc.perturb_params(orc.init_params(_ocfg(which), seed=3), 0.05)


def _net(which, idr=False):
    key = ("net", which, idr)
    if key not in _CACHE:
        from i2sdf_amd import I2SDFNetwork
        from i2sdf_amd.config import plumbing_conf, synthetic_conf
        conf = synthetic_conf() if which == "synthetic" else plumbing_conf(skip=which.endswith("skip"))
        sd = _weights(which)
        if idr:
            conf = idr_ref.idr_conf(conf)
            sd_idr = orc.perturb_params(idr_ref.init_params(_ocfg(which), seed=3), 0.05)
            sd = {k: (sd[k] if k.startswith("implicit_network") or k == "density.beta" else v) for k, v in sd_idr.items()}
        net = I2SDFNetwork(conf)
        net.load_state_dict(sd)
        _CACHE[key] = net.cuda().eval()
    return _CACHE[key]


def _engine(which):
    return _net(which)._engine_for(torch.device("cuda:0"))


def _routes(which):
    """the routes this plan has: the stepwise one always; the fused one unless the library refuses it with that reason"""
    key = ("routes", which)
    if key not in _CACHE:
        from i2sdf_amd.lib import I2SDFError
        z = torch.zeros(1, 3, device="cuda")
        try:
            _engine(which).trace_rays(z, z, 0.0, 1.0, max_steps=1, route="fused")
            _CACHE[key] = ("stepwise", "fused")
        except I2SDFError as e:
            assert "fused" in str(e)
            _CACHE[key] = ("stepwise",)
    return _CACHE[key]


def _graze(which):
    """a ray that just catches the surface: the impact parameter b of the rays (b, 0, -2) + t (0, 0, 1) bisected between a hit and a miss
    with the fp32 tracer on the oracle's net, then stepped 2e-3 back towards the hit"""
    key = ("graze", which)
    if key not in _CACHE:
        f = TR.oracle_sdf(_weights(which), _ocfg(which), np.float32)
        d = np.array([[0.0, 0.0, 1.0]], np.float32)
        hit = lambda b: TR.trace(f, np.array([[b, 0.0, -2.0]], np.float32), d, 0.0, 4.5)[1][0] == TR.HIT
        lo, hi = 0.0, 2.0
        assert hit(lo) and not hit(hi)
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if hit(mid) else (lo, mid)
        _CACHE[key] = np.array([lo - 2e-3, 0.0, -2.0], np.float32)
    return _CACHE[key]


def _rays(which, N):
    o, d, t0, t1 = TR.make_rays(N, seed=100 + N)
    if N == 389:
        # second tile: every ray points away from the scene; third tile: the same, but for one grazing ray
        out = o[128:384] / np.linalg.norm(o[128:384], axis=1, keepdims=True)
        d[128:384] = out.astype(np.float32)
        o[300], d[300] = _graze(which), np.array([0.0, 0.0, 1.0], np.float32)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        b = (o64 * d64).sum(1)
        t1 = (-b + np.sqrt(b * b - ((o64 * o64).sum(1) - 9.0))).astype(np.float32)
    return o, d, t0, t1


def _device_trace(which, N, max_steps, route, run=0):
    """one traced batch, every buffer the library writes cut out of a canary-filled allocation; cached (as numpy) per case"""
    key = ("trace", which, N, max_steps, route, run)
    if key in _CACHE:
        return _CACHE[key]
    eng = _engine(which)
    o, d, t0, t1 = _rays(which, N)
    n_ws = int(eng._lib.i2sdf_trace_workspace_floats(N))
    pat = {torch.float32: -7.25, torch.int32: -77}

    def guarded(n, dtype):
        buf = torch.full((n + 2 * CANARY,), pat[dtype], dtype=dtype, device="cuda")
        return buf, buf[CANARY:CANARY + n]

    bufs = {"t": guarded(N, torch.float32), "status": guarded(N, torch.int32), "steps": guarded(N, torch.int32),
            "f_trace": guarded(max_steps * N, torch.float32), "ws": guarded(n_ws, torch.float32)}
    bufs["f_trace"][1].fill_(float("nan"))
    out = {"t": bufs["t"][1], "status": bufs["status"][1], "steps": bufs["steps"][1], "f_trace": bufs["f_trace"][1].view(max_steps, N)}
    c = lambda a: torch.from_numpy(a).cuda()
    res = eng.trace_rays(c(o), c(d), c(t0), c(t1), max_steps=max_steps, route=route, return_f=True, workspace=bufs["ws"][1], out=out)
    assert res.t.data_ptr() == out["t"].data_ptr() and res.f_trace.data_ptr() == out["f_trace"].data_ptr()
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        p = pat[buf.dtype]
        assert bool((buf[:CANARY] == p).all()) and bool((buf[-CANARY:] == p).all()), f"{name}: canary overwritten ({which}, N={N}, {route})"
    r = {k: v.cpu().numpy().copy() for k, v in out.items()}
    _CACHE[key] = r
    return r


def _point(o, d, t):
    """o + t d as the kernels form it: hipcc contracts fetch_point's multiply and add, so a component is fma(t, d, o), rounded ONCE
    (include/i2sdf.h says so for the traced points).  Here: the product of two fp32 is exact in fp64, the sum is rounded to 53 bits and
    then to 24 -- the same value unless the 53-bit sum falls exactly between two fp32, which none of these fixed inputs does."""
    return (o.double() + t.double().unsqueeze(1) * d.double()).float()


def _same_bits(a, b, what):
    for k in ("t", "status", "steps", "f_trace"):
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


CASES = [(w, n, s) for w in NETS for n in SIZES for s in STEPS]


@pytest.mark.parametrize("which,N,max_steps", CASES)
def test_replay_of_the_device_f_trace_reproduces_the_march(which, N, max_steps):
    o, d, t0, t1 = _rays(which, N)
    for route in _routes(which):
        dev = _device_trace(which, N, max_steps, route)
        t, status, steps, f_ref = TR.trace(None, o, d, t0, t1, max_steps=max_steps, replay=dev["f_trace"], return_f=True)
        assert np.array_equal(np.isnan(dev["f_trace"]), np.isnan(f_ref)), f"{route}: f_trace written where no step was taken, or not where one was"
        assert dev["t"].tobytes() == t.tobytes(), route
        assert np.array_equal(dev["status"], status) and np.array_equal(dev["steps"], steps), route
        assert set(np.unique(status)) <= {TR.HIT, TR.MISS, TR.UNRESOLVED, TR.INSIDE}
    if N == 389:
        if max_steps == 64:
            assert (status[128:256] == TR.MISS).all()
            third = status[256:384]
            assert (np.delete(third, 300 - 256) == TR.MISS).all() and third[300 - 256] in (TR.HIT, TR.UNRESOLVED)
            assert (status == TR.HIT).sum() >= 20


@pytest.mark.parametrize("which,N,max_steps", CASES)
def test_every_f_trace_entry_is_the_sdf_at_the_point_of_its_step(which, N, max_steps):
    net = _net(which)
    o, d, t0, t1 = _rays(which, N)
    oc, dc = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    for route in _routes(which):
        dev = _device_trace(which, N, max_steps, route)
        t_tr = TR.trace(None, o, d, t0, t1, max_steps=max_steps, replay=dev["f_trace"], return_t=True)[3]
        took = ~np.isnan(t_tr)
        s_idx, r_idx = np.nonzero(took)
        assert s_idx.size >= N
        r = torch.from_numpy(r_idx).cuda()
        tt = torch.from_numpy(t_tr[took]).cuda()
        x = _point(oc[r], dc[r], tt)
        want = net.implicit_network.get_sdf_vals(x)[:, 0].cpu().numpy()
        assert dev["f_trace"][took].tobytes() == want.tobytes(), route
        full = net.implicit_network(x)[:, 0].cpu()
        assert_close(torch.from_numpy(dev["f_trace"][took]), full, 1e-5, "f_trace vs implicit_network(x)[:, 0]")


@pytest.mark.parametrize("which,N,max_steps", CASES)
def test_routes_agree_bit_for_bit_and_repeat(which, N, max_steps):
    routes = _routes(which)
    first = _device_trace(which, N, max_steps, routes[0])
    for route in routes:
        a, b = _device_trace(which, N, max_steps, route, 0), _device_trace(which, N, max_steps, route, 1)
        _same_bits(a, b, f"{route}, two runs")
        _same_bits(a, first, f"{route} against {routes[0]}")


def test_the_fused_route_is_there_or_refused_with_the_reason():
    """bf16x3 plans (the default of every net here) have a fused kernel; `bf16x3: false` plans have none: route 2 is refused with the reason,
    nothing is launched, and route 0 takes the stepwise route there"""
    from i2sdf_amd import I2SDFNetwork
    from i2sdf_amd.config import synthetic_conf
    from i2sdf_amd.lib import I2SDFError
    for which in NETS:
        assert _routes(which) == ("stepwise", "fused"), which
        z = torch.zeros(3, 3, device="cuda")
        r = _engine(which).trace_rays(z[:0], z[:0], route="fused")          # an empty batch: empty results, nothing launched
        assert r.t.shape == (0,) and r.status.dtype == torch.int32 and r.steps.shape == (0,)
    conf = synthetic_conf()
    conf["bf16x3"] = False
    net = I2SDFNetwork(conf)
    net.load_state_dict(_weights("synthetic"))
    eng = net.cuda().eval()._engine_for(torch.device("cuda:0"))
    o, d, t0, t1 = (torch.from_numpy(a).cuda() for a in _rays("synthetic", 133))
    for n in (0, 133):
        with pytest.raises(I2SDFError, match="fused"):
            eng.trace_rays(o[:n], d[:n], t0[:n], t1[:n], route="fused")
    a, b = eng.trace_rays(o, d, t0, t1, route="auto", return_f=True), eng.trace_rays(o, d, t0, t1, route="stepwise", return_f=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a.f_trace.cpu().numpy().tobytes() == b.f_trace.cpu().numpy().tobytes()
    ref = TR.trace(None, o.cpu().numpy(), d.cpu().numpy(), t0.cpu().numpy(), t1.cpu().numpy(), replay=a.f_trace.cpu().numpy())
    assert a.t.cpu().numpy().tobytes() == ref[0].tobytes() and np.array_equal(a.status.cpu().numpy(), ref[1])


@pytest.mark.parametrize("which", NETS)
def test_replay_with_a_step_scale_below_one(which):
    """step_scale 0.7: t + step_scale * f must be two roundings on the device too (a contracted multiply-add would differ in the last bit)"""
    o, d, t0, t1 = _rays(which, 389)
    c = lambda a: torch.from_numpy(a).cuda()
    got = {}
    for route in _routes(which):
        r = _engine(which).trace_rays(c(o), c(d), c(t0), c(t1), step_scale=0.7, eps=3e-5, route=route, return_f=True)
        t, status, steps = TR.trace(None, o, d, t0, t1, step_scale=0.7, eps=3e-5, replay=r.f_trace.cpu().numpy())
        assert r.t.cpu().numpy().tobytes() == t.tobytes() and np.array_equal(r.status.cpu().numpy(), status) and np.array_equal(r.steps.cpu().numpy(), steps)
        got[route] = r
    for route in got:
        assert all(torch.equal(x, y) for x, y in zip(got[route][:3], got["stepwise"][:3])), route


@pytest.mark.parametrize("which", NETS)
def test_against_the_fp64_tracer_on_the_fp64_oracle_net(which):
    n, eps = 1500, 1e-4
    ocfg, sd = _ocfg(which), _weights(which)
    sd64 = {k: v.double() for k, v in sd.items()}
    o, d, t0, t1 = TR.make_rays(n, seed=7)
    t_ref, s_ref, n_ref = TR.trace(TR.oracle_sdf(sd, ocfg, np.float64), o, d, t0, t1, eps=eps, dtype=np.float64)
    g = torch.Generator().manual_seed(17)
    box = (torch.rand(4096, 3, generator=g, dtype=torch.float64) * 2 - 1) * 2.5
    delta = 1e-5 * float(orc.sdf_forward(sd64, ocfg.sdf, box)[:, 0].abs().max())
    both_ref = s_ref == TR.HIT
    x = torch.from_numpy(TR.points(o.astype(np.float64), d.astype(np.float64), t_ref))
    slope = np.abs((orc.sdf_gradient(sd64, ocfg.sdf, x).numpy() * d.astype(np.float64)).sum(1))
    c = lambda a: torch.from_numpy(a).cuda()
    for route in _routes(which):
        r = _engine(which).trace_rays(c(o), c(d), c(t0), c(t1), eps=eps, max_steps=64, route=route)
        t, status, steps = r.t.cpu().numpy(), r.status.cpu().numpy(), r.steps.cpu().numpy()
        differ = float((status != s_ref).mean())
        both = both_ref & (status == TR.HIT)
        well = both & (slope >= 0.2)
        frac_well = well.sum() / max(both.sum(), 1)
        used = np.abs(t[well].astype(np.float64) - t_ref[well]) * slope[well] / (2 * eps + 2 * delta)
        print(f"{which} / {route}: status differs on {differ * 100:.2f} % of {n} rays; {both.sum()} common hits, {frac_well * 100:.1f} % well posed; "
              f"used fraction of (2 eps + 2 delta) / slope: max {used.max():.4f}, median {np.median(used):.4f}; delta {delta:.2e}; "
              f"steps of hits <= {steps[both].max()}, {int((status == TR.UNRESOLVED).sum())} unresolved")
        assert differ <= 0.01
        assert both.sum() >= n // 5
        assert frac_well >= 0.9
        assert used.max() <= 1.0


def _public_routes_at(net, eng, o, d, t):
    """value, normal, features and radiance at o + t d through the module's public per-point routes (explicit points)"""
    x = _point(o, d, t)
    fw = eng.sdf_forward_grad(points=x, want_grad=True, save=False)
    grad = net.implicit_network.gradient(x)
    assert torch.equal(grad, fw["grad"])
    if eng.idr:
        rgb, _, _ = eng.rgb_forward(d, 1, fw["feat"], x.shape[0], save=False, points=x, normals=grad)
    else:
        rgb, _, _ = eng.rgb_forward(d, 1, fw["feat"], x.shape[0], save=False)
    return x, grad, fw["feat"][: x.shape[0]], rgb


@pytest.mark.parametrize("which,idr", [("plumbing", False), ("plumbing_skip", True), ("synthetic", False), ("synthetic", True)])
def test_trace_surface_and_render_surface(which, idr):
    net = _net(which, idr)
    eng = net._engine_for(torch.device("cuda:0"))
    assert eng.idr == idr
    N = 389
    o, d, t0, t1 = (torch.from_numpy(a).cuda() for a in _rays(which, N))
    dnorm = torch.linspace(1.0, 2.0, N, device="cuda")
    inp = {"uv": o, "rays": {"cam_loc": o, "dirs": d, "dnorm": dnorm}}
    net.train()
    ts = net.trace_surface(inp, t_min=t0, t_max=t1)
    rs = net.render_surface(inp, t_min=t0, t_max=t1)
    rs_chunked = net.render_surface(inp, split_n_pixels=150, t_min=t0, t_max=t1)
    assert net.training
    net.eval()
    tr = eng.trace_rays(o, d, t0, t1)
    hit = tr.status == 1
    assert 20 <= int(hit.sum()) < N
    for out in (ts, rs, rs_chunked):
        assert torch.equal(out["status"], tr.status) and torch.equal(out["hit"], hit) and out["t"].data_ptr() != tr.t.data_ptr()
        assert out["t"].cpu().numpy().tobytes() == tr.t.cpu().numpy().tobytes()
        assert torch.equal(out["depth_values"], tr.t / dnorm)
    assert "rgb_values" not in ts and set(rs) == set(ts) | {"rgb_values"} == set(rs_chunked)
    x, grad, feat, rgb = _public_routes_at(net, eng, o, d, tr.t)
    nohit = ~hit
    for out in (ts, rs, rs_chunked):
        assert torch.equal(out["points"][hit], x[hit])
        # the same kernel on the same points, formed from the rays in one case and read in the other: the routes' own bars, mostly the same bits
        assert_close(out["normal_map"][hit], torch.nn.functional.normalize(grad, dim=1)[hit], 1e-5, "normal_map")
        assert_close(out["feature_vectors"][hit], feat[hit], 1e-5, "feature_vectors")
        for k in ("points", "normal_map", "feature_vectors") + (("rgb_values",) if "rgb_values" in out else ()):
            assert out[k].shape[0] == N and bool((out[k][nohit] == 0).all()) and not bool(torch.isnan(out[k]).any()), k
    for out in (rs, rs_chunked):
        assert_close(out["rgb_values"][hit], rgb[hit], 2e-5, "rgb_values")
        assert float(out["rgb_values"][hit].min()) > 0.0
    # the camera form of the input: the rays ray_setup makes, the renderer's own default interval
    from helpers import camera_inputs
    cin = {k: v.cuda() for k, v in camera_inputs(77, (0.0, 0.2, -1.8), train_layout=False).items()}
    cs = net.render_surface(cin)
    cam, dirs, dn = eng.ray_setup(cin["uv"], cin["pose"], cin["intrinsics"])
    ct = eng.trace_rays(cam, dirs)
    assert torch.equal(cs["status"], ct.status) and torch.equal(cs["depth_values"], ct.t / dn) and cs["rgb_values"].shape == (77, 3)
    assert int(cs["hit"].sum()) >= 10


@pytest.mark.parametrize("which,idr", [("plumbing", False), ("synthetic", True)])
def test_get_incident_radiance_with_a_tracer_is_render_surface(which, idr):
    net = _net(which, idr)
    o, d, _, _ = (torch.from_numpy(a).cuda() for a in _rays(which, 133))
    tracer = net.sphere_tracer(max_steps=48, eps=2e-4)
    got = net.get_incident_radiance(o, d, intersect_func=tracer)
    want = net.render_surface({"uv": o, "rays": {"cam_loc": o, "dirs": d, "dnorm": torch.ones(133, device="cuda")}}, max_steps=48, eps=2e-4)
    assert got.shape == (133, 3) and torch.equal(got, want["rgb_values"]) and int(want["hit"].sum()) >= 10
    assert torch.equal(tracer(o, d)["status"], want["status"])
    # through the shading layer, which hands the hook on
    from i2sdf_amd import RenderingLayer
    layer = RenderingLayer(4, 100)
    n = 16
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.rand(*s, generator=g).cuda()
    nrm = torch.nn.functional.normalize(r(n, 3) - 0.5, dim=1)
    a = layer(net, r(n, 3) - 0.5, nrm, r(n, 3), r(n, 3), nrm, r(n, 1) * 0.5 + 0.2, intersect_func=tracer, samples=r(n, 4, 3))
    assert all(torch.isfinite(v).all() for v in a if isinstance(v, torch.Tensor))


def test_any_other_intersect_func_is_still_refused():
    net = _net("plumbing")
    z = torch.zeros(4, 3, device="cuda")
    with pytest.raises(NotImplementedError, match="intersect_func"):
        net.get_incident_radiance(z, z, intersect_func=lambda *a: None)
    with pytest.raises(NotImplementedError, match="intersect_func"):
        net.get_incident_radiance(z, z, intersect_func=_net("plumbing_skip").sphere_tracer())
