#!/usr/bin/env python3
"""Generate tests/golden/g23_shade_*.npz by RUNNING THE REFERENCE: its `RenderingLayer` (model/rendering/__init__.py) with the BRDF library
behind it (model/rendering/brdf.py), in fp32 and in fp64, `torch.rand` replaced by recorded uniforms and the model by a closed-form stand-in
(the same lines as tests/shade_ref.py: standin_radiance).  Needs the reference next to this checkout (tests/golden/ref_import.py); only data
is written.

    python tests/golden/gen_golden_shade.py

  g23_shade_well   bn 96, spp 24: unit normals, every view at least cos 0.2 above its surface, rough in [0.2, 1]; the seed is also redrawn
                   until the reference's own fp32 grough is within 5e-5 (max-norm, relative) of its fp64 grough
  g23_shade_wide   bn 96, spp 24: rough in [0.01, 1] with the 0.01 clamp hit, views down to cos 0.05, normals of length 0.5 .. 1.5, Ks with the
                   0.04 clamp hit, 5 .. 10 % of the rows with the view behind the surface (wi_mask false)

Each file: the inputs (surface_points, view_direction, normal, Kd, Ks, rough, radiance_scale, samples) and two output weights (w_diffuse,
w_spec, zero on the rows with wi_mask false, which every caller masks); the reference's fp32 results colorDiffuse, colorSpec, wi_mask and its
autograd gradients of sum(colorDiffuse w_diffuse) + sum(colorSpec w_spec): gKd, gKs, g_scale, grough (the model's radiance carries a graph to the directions) and grough_const (it does not);
the same from the fp64 run as `<name>.f64`, there also direction, points and g_radiance (the gradient at the model's output);
`dev.<name>`: the max-norm relative deviation of the fp32 run from the fp64 run over the rows with wi_mask true -- the reference's own
rounding noise, which the bar on grough of the wide fixture is made of; and for every fourth point (`sub_points`) the per-sample
`sub.rows.f64` (n, spp, 14): wo (local), pdf, f_spec and d / d rough of these seven, from the reference's functions called per sample.

A seed is redrawn until no sample sits on a branch: |u0 - pS| >= 1e-5, and wi_z, wo_z, 25 lum(Ks) and the clamped luminances keep 1e-6, alpha^4
and the pdf 1e-7, from every threshold they are tested against.  No sample is left out."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402
import gen_golden as G  # noqa: E402
import shade_ref as SR  # noqa: E402

torch.set_num_threads(4)
BN, SPP = 96, 24


class Standin:
    def __init__(self, graph):
        self.graph = graph
        self.outputs = []

    def get_incident_radiance(self, pts, dirs, intersect_func=None):
        with torch.set_grad_enabled(self.graph):
            a = pts * 1.7 + dirs.roll(1, -1) * 0.9
            b = dirs * 2.3 - pts.roll(1, -1) * 0.6
            shift = torch.tensor([0.3, 1.1, 2.0], dtype=pts.dtype)
            r = 0.85 + 0.35 * torch.sin(a + shift) + 0.25 * torch.cos(b - shift)
        r = r + 0.0 if r.requires_grad else r.clone().requires_grad_(True)
        r.retain_grad()
        self.outputs.append(r)
        return r


def make_inputs(seed, wide):
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    nrm = torch.nn.functional.normalize(torch.randn(BN, 3, generator=g, dtype=torch.float64), dim=1)
    tang = torch.nn.functional.normalize(torch.cross(nrm, torch.randn(BN, 3, generator=g, dtype=torch.float64), dim=1), dim=1)
    lo = 0.05 if wide else 0.2
    cos = lo + (1 - lo) * R(BN, 1)
    if wide:
        behind = torch.zeros(BN, dtype=torch.bool)
        behind[torch.randperm(BN, generator=g)[:7]] = True                       # 7 of 96 rows: 7.3 %
        cos = torch.where(behind[:, None], -(0.05 + 0.85 * R(BN, 1)), cos)
    view = cos * nrm + torch.sqrt(1 - cos * cos) * tang
    normal = nrm * (0.5 + R(BN, 1)) if wide else nrm
    Kd = R(BN, 3)
    Ks = (R(BN, 3) * 0.6).clamp_min(0.04)
    rough = (R(BN, 1) * 1.03 - 0.03).clamp_min(0.01) if wide else 0.2 + 0.8 * R(BN, 1)
    f = lambda t: t.float().numpy()
    return dict(surface_points=f(R(BN, 3) * 2 - 1), view_direction=f(view), normal=f(normal), Kd=f(Kd), Ks=f(Ks), rough=f(rough),
                radiance_scale=np.array([1.5, 0.7, 1.1], np.float32), samples=f(R(BN, SPP, 3)),
                w_diffuse=f(torch.randn(BN, 3, generator=g, dtype=torch.float64)), w_spec=f(torch.randn(BN, 3, generator=g, dtype=torch.float64)))


def away(x, thr, margin=1e-6):
    return bool(((x - thr).abs() >= margin).all())


def no_branch_flips(inp):
    """the fp64 restatement's intermediate values keep their distance from every threshold"""
    t = lambda k: torch.as_tensor(inp[k]).double()
    (x, y, z), wi, mask = SR.local_view(t("normal"), t("view_direction"))
    raw_z = (z * t("view_direction")).sum(1)
    pS = SR.specular_probability(t("Kd"), t("Ks"))
    wo = SR.sample_wo(wi, t("rough"), pS, t("samples"))
    pdf, _ = SR.sample_terms(wi, t("rough"), pS, t("Ks"), wo)
    a2 = t("rough") ** 4
    return ((t("samples")[..., 0] - pS).abs().min() >= 1e-5 and away(raw_z, 1e-5) and away(wi[:, 2], 1e-4) and away(wo[..., 2], 1e-4)
            and away(wo[..., 2], 0.0) and away(a2, 1e-5, 1e-7) and away(25 * SR.lum(t("Ks")), 1.0) and away(pdf, 1e-5, 1e-7)
            and away(SR.lum(t("Kd")), 0.01) and away(SR.lum(t("Ks")), 0.01))


def run_reference(RL, inp, dtype, graph):
    c = lambda k: torch.as_tensor(inp[k]).to(dtype)
    Kd, Ks, rough, scale = [c(k).requires_grad_(True) for k in ("Kd", "Ks", "rough", "radiance_scale")]
    model = Standin(graph)
    keep = torch.rand
    torch.rand = lambda *a, **k: c("samples")
    try:
        cd, cs, mask = RL(SPP, 1000)(model, c("surface_points"), c("view_direction"), Kd, Ks, c("normal"), rough, scale)
    finally:
        torch.rand = keep
    ((cd * c("w_diffuse")).sum() + (cs * c("w_spec")).sum()).backward()
    g_rad = torch.cat([r.grad for r in model.outputs], 0)
    return dict(colorDiffuse=cd.detach(), colorSpec=cs.detach(), wi_mask=mask, gKd=Kd.grad, gKs=Ks.grad, grough=rough.grad, g_scale=scale.grad,
                g_radiance=g_rad)


def directions(inp):
    """direction and points in fp64 as the layer forms them, with the reference's functions"""
    import model.rendering.brdf as B
    c = lambda k: torch.as_tensor(inp[k]).double()
    normal, view, samples = c("normal"), c("view_direction"), c("samples")
    cx, cy, cz = B.create_frame(normal)
    wi = torch.stack([(cx * view).sum(1), (cy * view).sum(1), (cz * view).sum(1)], 1)
    wi[:, 2] = torch.where(wi[:, 2] < 0.00001, torch.ones_like(wi[:, 2]) * 0.00001, wi[:, 2])
    wi = torch.nn.functional.normalize(wi, dim=1, eps=1e-6).unsqueeze(1)
    pS = B.probabilityToSampleSpecular(c("Kd"), c("Ks"))
    wo = torch.where((samples[:, :, 0] >= pS).unsqueeze(2).expand(BN, SPP, 3), B.square_to_cosine_hemisphere(samples[:, :, 1:]),
                     B.sample_ggx_specular(samples[:, :, 1:], c("rough"), wi))
    d = B.to_global(wo, cx.unsqueeze(1), cy.unsqueeze(1), cz.unsqueeze(1)).reshape(-1, 3)
    return d, c("surface_points").unsqueeze(1).expand(BN, SPP, 3).reshape(-1, 3) + d * 0.01, wi.squeeze(1)


def per_sample_rows(inp, wi, sub):
    """every (point, sample) of the points `sub` as a point of its own with one sample, so that autograd gives d / d rough per sample"""
    import model.rendering.brdf as B
    c = lambda k: torch.as_tensor(inp[k]).double()[sub].repeat_interleave(SPP, 0)
    n = len(sub) * SPP
    samples = torch.as_tensor(inp["samples"]).double()[sub].reshape(n, 1, 3)
    Kd, Ks, w = c("Kd"), c("Ks"), wi[sub].repeat_interleave(SPP, 0).unsqueeze(1)
    rough = c("rough").requires_grad_(True)
    pS = B.probabilityToSampleSpecular(Kd, Ks)
    wo = torch.where((samples[:, :, 0] >= pS).unsqueeze(2).expand(n, 1, 3), B.square_to_cosine_hemisphere(samples[:, :, 1:]),
                     B.sample_ggx_specular(samples[:, :, 1:], rough, w))
    pdf = torch.clamp(B.pdf_ggx(Kd, Ks, rough, w, wo, 0.0).unsqueeze(2), min=0.00001)
    _, spec, _ = B.eval_ggx(Kd, Ks, rough, w, wo)
    cols = torch.cat([wo, pdf, spec.expand(n, 1, 3)], 2).reshape(n, 7)
    grads = []
    for k in range(7):
        gk, = torch.autograd.grad(cols[:, k].sum(), rough, retain_graph=True, allow_unused=True)
        grads.append(torch.zeros(n, 1, dtype=torch.float64) if gk is None else gk)
    return torch.cat([cols.detach(), torch.cat(grads, 1)], 1).reshape(len(sub), SPP, 14)


def rel(a, b, rows):
    a, b = a.double().reshape(BN, -1)[rows], b.double().reshape(BN, -1)[rows]
    return float((a - b).abs().max() / b.abs().max())


def main():
    ref_model, _ = ref_import.import_reference()
    RL = ref_model.RenderingLayer
    for name, wide in (("g23_shade_well", False), ("g23_shade_wide", True)):
        seed = 2300 + (50 if wide else 0)
        while True:
            inp = make_inputs(seed, wide)
            above = SR.local_view(torch.as_tensor(inp["normal"]).double(), torch.as_tensor(inp["view_direction"]).double())[2].numpy()
            inp["w_diffuse"][~above] = 0          # every caller masks the rows with the view behind the surface: so do the output weights
            inp["w_spec"][~above] = 0
            ok = no_branch_flips(inp)
            if ok:
                r32, r64 = run_reference(RL, inp, torch.float32, True), run_reference(RL, inp, torch.float64, True)
                ok = bool((r32["wi_mask"] == r64["wi_mask"]).all())
            if ok:
                c32, c64 = run_reference(RL, inp, torch.float32, False), run_reference(RL, inp, torch.float64, False)
                # well-posed means well-posed for the reference: its own fp32 grough stays within half of the tests' 1e-4 of its fp64 one.
                # (A single sample with u1 -> 1, a grazing micro-normal under a small pdf, is enough to put the REFERENCE at 2e-4.)
                ok = wide or max(rel(r32["grough"], r64["grough"], r64["wi_mask"]), rel(c32["grough"], c64["grough"], r64["wi_mask"])) <= 5e-5
            if ok:
                break
            seed += 1
        mask = r64["wi_mask"]
        frac = 1 - float(mask.double().mean())
        assert (0.05 <= frac <= 0.10) if wide else frac == 0, frac
        if wide:
            assert (inp["rough"] == np.float32(0.01)).any() and (inp["Ks"] == np.float32(0.04)).any()
        for k in ("colorDiffuse", "colorSpec", "gKd", "gKs", "g_scale", "g_radiance"):      # the model's graph changes none of these
            assert torch.equal(r64[k], c64[k]), k
        d64, p64, wi64 = directions(inp)
        sub = np.arange(0, BN, 4)
        arrs = dict(inp)
        arrs["sub_points"] = sub
        arrs["sub.rows.f64"] = per_sample_rows(inp, wi64, torch.as_tensor(sub))
        arrs["wi_mask"] = mask
        arrs["direction.f64"], arrs["points.f64"], arrs["g_radiance.f64"] = d64, p64, r64["g_radiance"]
        r32["grough_const"], r64["grough_const"] = c32["grough"], c64["grough"]
        for k in ("colorDiffuse", "colorSpec", "gKd", "gKs", "grough", "grough_const", "g_scale", "g_radiance"):
            if k != "g_radiance":
                arrs[k], arrs[k + ".f64"] = r32[k], r64[k]
            rows = slice(None) if k == "g_scale" else mask
            arrs["dev." + k] = np.float64(rel(r32[k], r64[k], rows) if k != "g_scale" else
                                          float((r32[k].double() - r64[k]).abs().max() / r64[k].abs().max()))
        print(name, "seed", seed, "wi_mask false %.1f %%" % (100 * frac), {k: "%.2e" % float(v) for k, v in arrs.items() if k.startswith("dev.")})
        G.save(name, **arrs)
        assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 300 * 1024


if __name__ == "__main__":
    main()
