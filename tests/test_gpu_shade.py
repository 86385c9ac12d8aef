"""GPU: i2sdf_amd.RenderingLayer (csrc/shade.hip) against the reference's fp64 run recorded in tests/golden/g23_shade_*.npz and against the
fp64 restatement tests/shade_ref.py at the shapes where the kernels can go wrong, and I2SDFNetwork.get_incident_radiance.

Bars (max-norm relative over the rows with wi_mask true; the rows with the view behind the surface are checked for finiteness only: there the
reference itself returns 1e9 .. 1e11 that differ between its fp32 and fp64 runs by 1e-3 .. 1e-2, and every caller masks them):
  forward (colorDiffuse, colorSpec, direction, points)   2e-5, the project's forward bar
  gKd, gKs, g_radiance, g_radiance_scale                 1e-4, the project's gradient bar
  grough                                                 1e-4 on the well-posed fixture; max(1e-4, 2 x the fp32 REFERENCE's recorded deviation
                                                         from its fp64 run) on the wide one (`dev.grough` / `dev.grough_const` of the .npz): the
                                                         reference's own rounding noise there is 4e-4, the factor 2 covers a different but
                                                         equally valid operation order (fma contraction, hardware sine)
At the other shapes the inputs are drawn here, well-posed in the same sense as the first fixture (see _random_case), and every bar is the
flat one: 2e-5 forward, 1e-4 for every gradient, grough included."""
import functools
import os

import numpy as np
import pytest
import torch

import shade_ref as SR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (257, 37), (5, 130), (64, 64)]      # a lone sample; spp no multiple of the lanes that share a point; spp past one stride of
#                                                       64 lanes with a partial last one; bn no multiple of the points of a workgroup (4, 4, 4, 4)


class Tap:
    """the stand-in model on the device; keeps what it was asked and hands out radiance whose gradient can be read afterwards"""

    def __init__(self, graph):
        self.graph, self.pts, self.dirs, self.out = graph, [], [], []

    def get_incident_radiance(self, pts, dirs, intersect_func=None):
        self.pts.append(pts.detach())
        self.dirs.append(dirs.detach())
        with torch.set_grad_enabled(self.graph):
            r = SR.standin_radiance(pts, dirs)
        r = r + 0.0 if r.requires_grad else r.clone().requires_grad_(True)
        r.retain_grad()
        self.out.append(r)
        return r


@functools.lru_cache(maxsize=None)
def _fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"g23_shade_{name}.npz")))
    return g


def _draw_case(bn, spp, seed):
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    nrm = torch.nn.functional.normalize(torch.randn(bn, 3, generator=g, dtype=torch.float64), dim=1)
    tang = torch.nn.functional.normalize(torch.cross(nrm, torch.randn(bn, 3, generator=g, dtype=torch.float64), dim=1), dim=1)
    cos = 0.2 + 0.8 * R(bn, 1)
    f = lambda t: t.float().numpy()
    inp = dict(surface_points=f(R(bn, 3) * 2 - 1), view_direction=f(cos * nrm + torch.sqrt(1 - cos * cos) * tang), normal=f(nrm * (0.5 + R(bn, 1))),
               Kd=f(R(bn, 3)), Ks=f((R(bn, 3) * 0.6).clamp_min(0.04)), rough=f(0.2 + 0.8 * R(bn, 1)),
               radiance_scale=np.array([1.5, 0.7, 1.1], np.float32), samples=f(R(bn, spp, 3)))
    inp["w_diffuse"], inp["w_spec"] = f(torch.randn(bn, 3, generator=g, dtype=torch.float64)), f(torch.randn(bn, 3, generator=g, dtype=torch.float64))
    return inp


FORWARD = ("colorDiffuse", "colorSpec", "direction", "points")
GRADS = ("gKd", "gKs", "g_radiance", "g_scale", "grough")


@functools.lru_cache(maxsize=None)
def _random_case(bn, spp):
    """Inputs drawn here (views at least cos 0.2 above the surface, rough in [0.2, 1], normals of length 0.5 .. 1.5) and the fp64 restatement's
    results with and without the model's graph.  As the goldens' generator does for the well-posed fixture, the seed is redrawn until the case
    is well-posed for the REFERENCE's arithmetic: the restatement run in fp32 on the CPU -- the reference's operation order -- stays within half
    of every bar of its own fp64 run.  (One sample with u1 -> 1, a grazing micro-normal whose z is the root of a cancelling difference, under a
    small pdf, puts any fp32 evaluation at 2e-5 on the forward and 2e-4 on grough; the first seed of (257, 37) has one.)  The kernels' output
    takes no part in the choice."""
    for seed in range(1000 * bn + spp, 1000 * bn + spp + 50):
        inp = _draw_case(bn, spp, seed)
        runs = {(dt, graph): SR.run(inp, inp["w_diffuse"], inp["w_spec"], dt, graph) for dt in (torch.float32, torch.float64) for graph in (True, False)}
        dev = lambda k, graph: _rel(runs[torch.float32, graph][k], runs[torch.float64, graph][k])
        if all(dev(k, gr) <= 1e-5 for k in FORWARD for gr in (True, False)) and all(dev(k, gr) <= 5e-5 for k in GRADS for gr in (True, False)):
            break
    else:
        raise AssertionError("no well-posed case in 50 seeds")
    out = dict(inp)
    r64 = runs[torch.float64, True]
    out["grough.f64"], out["grough_const.f64"] = r64["grough"].numpy(), runs[torch.float64, False]["grough"].numpy()
    for k in ("colorDiffuse", "colorSpec", "gKd", "gKs", "g_scale", "direction", "points", "g_radiance"):
        out[k + ".f64"] = r64[k].numpy()
    out["wi_mask"] = r64["wi_mask"].numpy()
    out["seed"] = seed
    assert out["wi_mask"].all()
    return out


def _rel(a, b, rows=None):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    if rows is not None:
        n = rows.shape[0]
        a, b = a.reshape(n, -1)[rows], b.reshape(n, -1)[rows]
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _run_layer(g, graph, scale=True, samples=True, seed=None):
    from i2sdf_amd import RenderingLayer
    dev = torch.device("cuda")
    c = lambda k: torch.as_tensor(g[k]).to(dev)
    bn, spp = g["samples"].shape[:2]
    Kd, Ks, rough = c("Kd").requires_grad_(True), c("Ks").requires_grad_(True), c("rough").requires_grad_(True)
    sc = c("radiance_scale").requires_grad_(True) if scale is True else scale
    model = Tap(graph)
    if seed is not None:
        torch.manual_seed(seed)
    cd, cs, mask = RenderingLayer(spp, 1 << 30)(model, c("surface_points"), c("view_direction"), Kd, Ks, c("normal"), rough, sc,
                                                samples=c("samples") if samples else None)
    ((cd * c("w_diffuse")).sum() + (cs * c("w_spec")).sum()).backward()
    return dict(colorDiffuse=cd.detach(), colorSpec=cs.detach(), wi_mask=mask, direction=torch.cat(model.dirs), points=torch.cat(model.pts),
                gKd=Kd.grad, gKs=Ks.grad, grough=rough.grad, g_radiance=torch.cat([r.grad for r in model.out]),
                g_scale=sc.grad if isinstance(sc, torch.Tensor) and sc.requires_grad else None)


def _check(g, name, well_posed):
    above = torch.as_tensor(g["wi_mask"])
    for graph in (False, True):
        r = _run_layer(g, graph)
        assert r["wi_mask"].dtype == torch.bool and torch.equal(r["wi_mask"].cpu(), above)
        for k in ("colorDiffuse", "colorSpec", "direction", "points", "gKd", "gKs", "grough", "g_radiance", "g_scale"):
            assert bool(torch.isfinite(r[k]).all()), (name, k)
        tag = "grough" if graph else "grough_const"
        bars = {k: 2e-5 for k in ("colorDiffuse", "colorSpec", "direction", "points")}
        bars.update({k: 1e-4 for k in ("gKd", "gKs", "g_radiance")})
        errs = {k: _rel(r[k], g[k + ".f64"], above) for k in bars}
        errs["g_scale"], bars["g_scale"] = _rel(r["g_scale"], g["g_scale.f64"]), 1e-4
        errs["grough"], bars["grough"] = _rel(r["grough"], g[tag + ".f64"], above), 1e-4 if well_posed else max(1e-4, 2 * float(g["dev." + tag]))
        print(f"{name} graph={graph}: " + ", ".join(f"{k} {errs[k]:.2e} (bar {bars[k]:.1e})" for k in bars))
        for k in bars:
            assert errs[k] <= bars[k], (name, graph, k, errs[k], bars[k])


@pytest.mark.parametrize("name", ["well", "wide"])
def test_fixture_forward_and_gradients(name):
    _check(_fixture(name), name, well_posed=(name == "well"))


@pytest.mark.parametrize("bn,spp", SHAPES)
def test_shapes_forward_and_gradients(bn, spp):
    _check(_random_case(bn, spp), f"({bn}, {spp})", well_posed=True)


def test_seed_route_is_the_samples_route_and_runs_repeat():
    from i2sdf_amd import shade_draws
    g = dict(_random_case(257, 37))
    torch.manual_seed(4321)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())          # what the layer takes from torch's CPU generator
    a = _run_layer(g, True, samples=False, seed=4321)
    b = _run_layer(g, True, samples=False, seed=4321)
    u = shade_draws(seed, 257, 37)
    g["samples"] = u.cpu().numpy()
    c = _run_layer(g, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k                       # two runs, bit for bit
        assert torch.equal(a[k], c[k]), k                       # the seed is nothing but its uniforms
    d = _run_layer(g, True, samples=False, seed=4322)
    assert not torch.equal(a["direction"], d["direction"])      # torch.manual_seed decides the run
    assert u.shape == (257, 37, 3) and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    n = u.numel()
    assert abs(float(u.double().mean()) - 0.5) <= 4.0 / (12.0 * n) ** 0.5
    assert torch.unique(u.reshape(-1, 3), dim=0).shape[0] == 257 * 37          # no (point, sample) repeats another's triple
    small = shade_draws(seed, 16, 8)                                           # 384 values of 2^24: a repeat has probability 4e-3
    assert torch.unique(small).numel() == small.numel()
    assert torch.equal(small.reshape(-1, 3), shade_draws(seed, 1, 128).reshape(-1, 3))      # the counter is point spp + s


def test_without_a_scale_equals_a_scale_of_ones():
    g = _random_case(64, 64)
    a = _run_layer(g, True, scale=None)
    b = _run_layer(g, True, scale=torch.ones(3, device="cuda"))
    for k in ("colorDiffuse", "colorSpec", "gKd", "gKs", "grough", "g_radiance"):
        assert torch.equal(a[k], b[k]), k
    assert a["g_scale"] is None


def test_geometry_that_requires_grad_is_refused():
    from i2sdf_amd import RenderingLayer
    g = _random_case(5, 130)
    c = lambda k: torch.as_tensor(g[k]).cuda()
    for bad in ("normal", "view_direction", "surface_points"):
        args = {k: c(k) for k in ("surface_points", "view_direction", "Kd", "Ks", "normal", "rough")}
        args[bad].requires_grad_()
        with pytest.raises(NotImplementedError, match="frozen"):
            RenderingLayer(130, 1000)(Tap(False), args["surface_points"], args["view_direction"], args["Kd"], args["Ks"], args["normal"], args["rough"])


def _plumbing_net():
    from oracle import i2sdf_oracle as orc
    from i2sdf_amd import I2SDFNetwork, plumbing_conf
    sd = orc.perturb_params(orc.init_params(orc.plumbing_cfg(), seed=1), 0.05, seed=2)
    sd["density.beta"] = torch.tensor(0.05)
    net = I2SDFNetwork(plumbing_conf())
    net.load_state_dict(sd)
    return net.cuda()


def test_get_incident_radiance_and_the_layer_end_to_end():
    from i2sdf_amd import RenderingLayer
    net = _plumbing_net().train()
    g = torch.Generator().manual_seed(9)
    pts = ((torch.rand(300, 3, generator=g) * 2 - 1) * 0.8).cuda()               # interior points
    dirs = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=1).cuda()
    got = net.get_incident_radiance(pts, dirs)
    assert net.training and got.shape == (300, 3) and not got.requires_grad
    with torch.no_grad():
        want = net.eval()({"uv": pts, "rays": {"cam_loc": pts, "dirs": dirs, "dnorm": torch.ones(300, device="cuda")}}, predict_only=True)["rgb_values"]
    assert torch.equal(got, want)
    with pytest.raises(NotImplementedError, match="intersect_func"):
        net.get_incident_radiance(pts, dirs, intersect_func=lambda *a: None)

    calls = []

    class Counting:
        def get_incident_radiance(self, p, d, f=None):
            calls.append(int(p.shape[0]))
            return net.get_incident_radiance(p, d, f)

    bn, spp = 64, 8
    x = ((torch.rand(bn, 3, generator=g) * 2 - 1) * 0.5).cuda()
    normal = torch.nn.functional.normalize(torch.randn(bn, 3, generator=g), dim=1).cuda()
    view = torch.nn.functional.normalize(normal + 0.5 * torch.randn(bn, 3, generator=g).cuda(), dim=1)
    Kd, Ks = torch.rand(bn, 3, generator=g).cuda().requires_grad_(True), (torch.rand(bn, 3, generator=g) * 0.5 + 0.04).cuda().requires_grad_(True)
    rough = (0.2 + 0.7 * torch.rand(bn, 1, generator=g)).cuda().requires_grad_(True)
    torch.manual_seed(5)
    cd, cs, mask = RenderingLayer(spp, 200)(Counting(), x, view, Kd, Ks, normal, rough)
    assert calls == [200, 200, 112]                                               # three chunks, the last partial
    assert cd.shape == (bn, 3) and cs.shape == (bn, 3) and mask.shape == (bn,) and mask.dtype == torch.bool
    assert bool(torch.isfinite(cd).all()) and bool(torch.isfinite(cs).all())
    (cd.sum() + cs.sum()).backward()
    for t_ in (Kd, Ks, rough):
        assert t_.grad is not None and bool(torch.isfinite(t_.grad).all())
    assert rough.is_leaf and float(rough.grad.abs().max()) > 0
