"""Surface shading restated per sample in torch (any dtype, any device; fp64 on the CPU is the tests' yardstick): what
i2sdf_amd/csrc/brdf_dev.h computes, written as whole-tensor operations so that torch's autograd supplies every gradient.  Held to the
goldens tests/golden/g23_shade_*.npz and to the reference itself by tests/test_shade_ref.py.

Shapes: per-point tensors (bn, c); uniforms (bn, spp, 3); per-sample results (bn, spp, ...)."""
import math

import torch

LUM = (0.212671, 0.715160, 0.072169)


def standin_radiance(pts, dirs):
    """The closed-form stand-in for the model's incident radiance (the goldens' generator has the same lines): smooth, positive
    (0.25 .. 1.45), a function of the origin and of the direction."""
    a = pts * 1.7 + dirs.roll(1, -1) * 0.9
    b = dirs * 2.3 - pts.roll(1, -1) * 0.6
    shift = torch.tensor([0.3, 1.1, 2.0], dtype=pts.dtype, device=pts.device)
    return 0.85 + 0.35 * torch.sin(a + shift) + 0.25 * torch.cos(b - shift)


class StandinModel:
    """get_incident_radiance of the stand-in; graph=False cuts the graph as a model that renders under no_grad does"""

    def __init__(self, graph=True):
        self.graph, self.calls = graph, []

    def get_incident_radiance(self, pts, dirs, intersect_func=None):
        self.calls.append(int(pts.shape[0]))
        if self.graph:
            return standin_radiance(pts, dirs)
        with torch.no_grad():
            return standin_radiance(pts, dirs)


def lum(c):
    return c[..., 0:1] * LUM[0] + c[..., 1:2] * LUM[1] + c[..., 2:3] * LUM[2]


def sq(x):
    return torch.sqrt(torch.clamp(x, min=1e-8))


def unit(v, eps):
    return v / torch.clamp(torch.sqrt((v * v).sum(-1, keepdim=True)), min=eps)


def frame(normal):
    z = unit(normal, 1e-6)
    zx, zy, zz = z[:, 0], z[:, 1], z[:, 2]
    s = torch.where(zz >= 0, torch.ones_like(zz), -torch.ones_like(zz))
    a = -1.0 / (s + zz)
    b = zx * zy * a
    x = torch.stack([1.0 + s * zx * zx * a, s * b, -s * zx], 1)
    y = torch.stack([b, s + zy * zy * a, -zy], 1)
    return x, y, z


def local_view(normal, view):
    """(x, y, z), wi (bn, 3) with wi_z raised to 1e-5 and re-normalised, wi_mask (bn)"""
    x, y, z = frame(normal)
    wi = torch.stack([(x * view).sum(1), (y * view).sum(1), (z * view).sum(1)], 1)
    mask = wi[:, 2] >= 1e-5
    wi = torch.cat([wi[:, :2], torch.clamp(wi[:, 2:], min=1e-5)], 1)
    return (x, y, z), unit(wi, 1e-6), mask


def specular_probability(Kd, Ks):
    lD, lS = torch.clamp(lum(Kd), min=0.01), torch.clamp(lum(Ks), min=0.01)
    return (lS / (lD + lS)).detach()            # (bn, 1): a constant of the backward


def sample_wo(wi, rough, pS, u):
    """wo (bn, spp, 3) in the local frame; wi (bn, 3), rough (bn, 1), pS (bn, 1), u (bn, spp, 3)"""
    u0, u1, u2 = u[..., 0:1], u[..., 1:2], u[..., 2:3]
    w = wi[:, None, :]
    # cosine hemisphere
    r = sq(u2)
    wo_d = torch.cat([torch.cos(2 * math.pi * u1) * r, torch.sin(2 * math.pi * u1) * r, sq(torch.clamp(1 - u2, min=0))], -1)
    # visible normals of the GGX distribution
    alpha = (rough * rough)[:, None, :]
    Vh = unit(torch.cat([alpha * w[..., 0:1], alpha * w[..., 1:2], w[..., 2:3]], -1), 1e-8)
    q = Vh[..., 0:1] ** 2 + Vh[..., 1:2] ** 2
    zero, one = torch.zeros_like(q), torch.ones_like(q)
    T1 = torch.where(q > 0, torch.cat([-Vh[..., 1:2], Vh[..., 0:1], zero], -1) / sq(q), torch.cat([one, zero, zero], -1))
    T2 = torch.cross(Vh, T1, dim=-1)
    rr = sq(u1)
    t1, t2 = rr * torch.cos(2 * math.pi * u2), rr * torch.sin(2 * math.pi * u2)
    s = 0.5 * (1 + Vh[..., 2:3])
    e0 = sq(1 - t1 * t1)
    t2 = torch.where(s < 0.5, e0 + s * (t2 - e0), t2 - (t2 - e0) * (1 - s))
    Nh = t1 * T1 + t2 * T2 + sq(torch.clamp(1 - t1 * t1 - t2 * t2, min=0)) * Vh
    h = unit(torch.cat([alpha * Nh[..., 0:1], alpha * Nh[..., 1:2], torch.clamp(Nh[..., 2:3], min=0)], -1), 1e-8)
    wo_s = 2 * (w * h).sum(-1, keepdim=True) * h - w
    return torch.where(u0 >= pS[:, None, :], wo_d, wo_s.expand_as(wo_d))


def sample_terms(wi, rough, pS, Ks, wo):
    """pdf (bn, spp, 1) after its substitutes and its floor, f_spec (bn, spp, 3)"""
    w = wi[:, None, :]
    nv, nl = w[..., 2:3], wo[..., 2:3]
    a2 = ((rough * rough) ** 2)[:, None, :]
    H = unit(w + wo, 1e-8)
    A = torch.clamp(a2, min=1e-5)
    D = A / (math.pi * ((A - 1) * H[..., 2:3] ** 2 + 1) ** 2)
    G1 = 2 / (sq((a2 * (1 - nv * nv) + nv * nv) / (nv * nv)) + 1)
    p = pS[:, None, :]
    pdf = p * D * G1 / (4 * nv) + (1 - p) * nl / math.pi
    small = torch.full_like(pdf, 1e-4)
    pdf = torch.where(nv <= 1e-4, small, pdf)
    pdf = torch.where(nl <= 1e-4, small, pdf)
    pdf = torch.clamp(pdf, min=1e-5)
    G2 = 0.5 / (nv * sq(a2 + nl * (nl - a2 * nl)) + nl * sq(a2 + nv * (nv - a2 * nv)))
    f90 = torch.clamp(25.0 * lum(Ks), max=1)[:, None, :]
    ks = Ks[:, None, :]
    F = ks + (f90 - ks) * (1 - (wo * H).sum(-1, keepdim=True)) ** 5
    f_spec = torch.where(nl < 1e-4, torch.full_like(F, 1e-4), F * G2 * D)
    return pdf, f_spec


def shade(model, surface_points, view_direction, Kd, Ks, normal, rough, radiance_scale, samples, split=None):
    """The whole layer.  Returns a dict: colorDiffuse, colorSpec (bn, 3), wi_mask (bn), direction, points, radiance (bn spp, 3), wo, pdf,
    f_spec per sample."""
    bn, spp = samples.shape[:2]
    (x, y, z), wi, mask = local_view(normal, view_direction)
    pS = specular_probability(Kd, Ks)
    wo = sample_wo(wi, rough, pS, samples)
    pdf, f_spec = sample_terms(wi, rough, pS, Ks, wo)
    direction = (wo[..., 0:1] * x[:, None, :] + wo[..., 1:2] * y[:, None, :] + wo[..., 2:3] * z[:, None, :]).reshape(-1, 3)
    points = surface_points[:, None, :].expand(bn, spp, 3).reshape(-1, 3) + direction * 0.01
    split = split or points.shape[0]
    radiance = torch.cat([model.get_incident_radiance(p_, d_, None) for p_, d_ in zip(points.split(split), direction.split(split))], 0)
    L = radiance.view(bn, spp, 3)
    if radiance_scale is not None:
        L = L * radiance_scale[None, None, :]
    wgt = torch.clamp(wo[..., 2:3], min=0) / pdf
    cd = (Kd[:, None, :] / math.pi * wgt * L).mean(1)
    cs = (f_spec * wgt * L).mean(1)
    return dict(colorDiffuse=cd, colorSpec=cs, wi_mask=mask, direction=direction, points=points, radiance=radiance, wo=wo, pdf=pdf, f_spec=f_spec)


def run(inputs, w_diffuse, w_spec, dtype=torch.float64, graph=True, device="cpu"):
    """Runs `shade` on the arrays of `inputs` (surface_points, view_direction, Kd, Ks, normal, rough, radiance_scale or None, samples) with the
    stand-in model and differentiates sum(colorDiffuse w_diffuse) + sum(colorSpec w_spec).  -> dict of detached outputs and gKd, gKs, grough,
    g_scale, g_radiance (taken at the model's output, so it is the same with and without the model's graph)"""
    t = lambda k: None if inputs.get(k) is None else torch.as_tensor(inputs[k]).to(device=device, dtype=dtype).clone()
    Kd, Ks, rough = t("Kd").requires_grad_(True), t("Ks").requires_grad_(True), t("rough").requires_grad_(True)
    scale = t("radiance_scale")
    if scale is not None:
        scale.requires_grad_(True)
    leaf = []

    class Tap(StandinModel):
        def get_incident_radiance(self, pts, dirs, intersect_func=None):
            r = super().get_incident_radiance(pts, dirs, intersect_func)
            r = r + 0.0 if r.requires_grad else r.clone().requires_grad_(True)
            r.retain_grad()
            leaf.append(r)
            return r

    out = shade(Tap(graph), t("surface_points"), t("view_direction"), Kd, Ks, t("normal"), rough, scale, t("samples"))
    wd, ws = torch.as_tensor(w_diffuse).to(device=device, dtype=dtype), torch.as_tensor(w_spec).to(device=device, dtype=dtype)
    ((out["colorDiffuse"] * wd).sum() + (out["colorSpec"] * ws).sum()).backward()
    res = {k: v.detach() for k, v in out.items()}
    res.update(gKd=Kd.grad, gKs=Ks.grad, grough=rough.grad, g_radiance=torch.cat([r.grad for r in leaf], 0),
               g_scale=None if scale is None else scale.grad)
    return res
