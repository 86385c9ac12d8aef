"""Surface shading (the reference's model/rendering): `RenderingLayer` and `get_rendering_parameters`.

For every surface point the layer draws `spp` outgoing directions from the diffuse / GGX mixture, asks the model for the incident radiance
along each (`model.get_incident_radiance(pts, dirs, intersect_func)`, in chunks of `split_n_pixels` rays) and averages f cos / pdf L into a
diffuse and a specular colour.  Everything but the model call is HIP (csrc/shade.hip, csrc/brdf_dev.h; include/i2sdf.h states every
formula): one launch before the model call, one after it, one or two in the backward.  Nothing per-sample is kept for the backward but the
radiance itself: the kernels recompute the sampled directions from the uniforms, which are a 64-bit seed unless the caller passes them.

Imitated: RenderingLayer.forward for (bn, c) inputs; create_frame, probabilityToSampleSpecular, square_to_cosine_hemisphere,
sample_ggx_specular, pdf_ggx, eval_ggx, get_rendering_parameters (with baseColorToSpecularF0).  Not imitated: eval_disney / pdf_disney /
sample_disney_specular and the weight form sample_ggx (the layer does not call them), and the trailing `h, w` dimensions the reference's BRDF
functions allow (image-shaped inputs): flatten them to (bn, c) first.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import lib as L_


def _check(rc, what):
    L_.check(rc, what, reason=True)


def _seed_arg(seed):
    return None if seed is None else C.byref(C.c_uint64(int(seed)))


def _f32(t, name, shape, dev):
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name}: expected {tuple(shape)} float32 on {dev}, got {got} (image-shaped inputs with trailing h, w are not supported: "
                         "flatten them to (bn, c))")
    return t.detach().contiguous()


def shade_draws(seed: int, bn: int, spp: int, device="cuda") -> torch.Tensor:
    """The uniforms (bn, spp, 3) that `seed` stands for inside the shading kernels (for tests and debugging)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L_.I2SDFError("shade_draws needs a ROCm device (there is no CPU path)")
    lib = L_.load()
    out = torch.empty(bn, spp, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.i2sdf_shade_draws(int(seed), bn, spp, L_.ptr(out), L_.stream_ptr()), "i2sdf_shade_draws")
    return out


def _backward(st, radiance, scale, g_cd, g_cs, g_dir, g_pts, want_rad, want_scale):
    """one i2sdf_shade_backward call -> gKd, gKs, grough, g_radiance, g_scale (None where not asked for)"""
    lib = L_.load()
    bn, spp, dev = st["bn"], st["spp"], st["dev"]
    colour = g_cd is not None
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    gKd, gKs = (new(bn, 3), new(bn, 3)) if colour else (None, None)
    grough = new(bn, 1)
    g_rad = new(bn * spp, 3) if want_rad else None
    g_scale = new(3) if want_scale else None
    ws = None
    if want_scale:
        ws = torch.empty(int(lib.i2sdf_shade_backward_workspace_bytes(bn, spp)), dtype=torch.uint8, device=dev)
    c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    g_cd, g_cs, g_dir, g_pts = c(g_cd), c(g_cs), c(g_dir), c(g_pts)
    with torch.cuda.device(dev):
        _check(lib.i2sdf_shade_backward(L_.ptr(st["view"]), L_.ptr(st["normal"]), L_.ptr(st["Kd"]), L_.ptr(st["Ks"]), L_.ptr(st["rough"]),
                                        L_.ptr(st["samples"]), _seed_arg(st["seed"]), L_.ptr(radiance), L_.ptr(scale), L_.ptr(g_cd), L_.ptr(g_cs),
                                        L_.ptr(g_dir), L_.ptr(g_pts), bn, spp, L_.ptr(ws), L_.ptr(gKd), L_.ptr(gKs), L_.ptr(grough),
                                        L_.ptr(g_rad), L_.ptr(g_scale), L_.stream_ptr()), "i2sdf_shade_backward")
    return gKd, gKs, grough, g_rad, g_scale


class _SampleFn(torch.autograd.Function):
    """rough -> (direction, points): the secondary rays.  Its backward runs only when the model's radiance carries a graph to them."""

    @staticmethod
    def forward(ctx, rough, st):
        lib = L_.load()
        bn, spp, dev = st["bn"], st["spp"], st["dev"]
        direction = torch.empty(bn * spp, 3, dtype=torch.float32, device=dev)
        points = torch.empty(bn * spp, 3, dtype=torch.float32, device=dev)
        mask = torch.empty(bn, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _check(lib.i2sdf_shade_sample(L_.ptr(st["x"]), L_.ptr(st["view"]), L_.ptr(st["normal"]), L_.ptr(st["Kd"]), L_.ptr(st["Ks"]),
                                          L_.ptr(st["rough"]), L_.ptr(st["samples"]), _seed_arg(st["seed"]), bn, spp, L_.ptr(direction),
                                          L_.ptr(points), L_.ptr(mask), L_.stream_ptr()), "i2sdf_shade_sample")
        ctx.st = st
        mask = mask.bool()
        ctx.mark_non_differentiable(mask)
        return direction, points, mask

    @staticmethod
    def backward(ctx, g_dir, g_pts, _g_mask):
        if g_dir is None and g_pts is None:
            return None, None
        return _backward(ctx.st, None, None, None, None, g_dir, g_pts, False, False)[2], None


class _ReduceFn(torch.autograd.Function):
    """(Kd, Ks, rough, radiance, radiance_scale) -> (colorDiffuse, colorSpec)"""

    @staticmethod
    def forward(ctx, Kd, Ks, rough, radiance, scale, st):
        lib = L_.load()
        bn, spp, dev = st["bn"], st["spp"], st["dev"]
        radiance = radiance.detach().contiguous()
        scale_c = None if scale is None else scale.detach().contiguous()
        cd = torch.empty(bn, 3, dtype=torch.float32, device=dev)
        cs = torch.empty(bn, 3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(lib.i2sdf_shade_reduce(L_.ptr(st["view"]), L_.ptr(st["normal"]), L_.ptr(st["Kd"]), L_.ptr(st["Ks"]), L_.ptr(st["rough"]),
                                          L_.ptr(st["samples"]), _seed_arg(st["seed"]), L_.ptr(radiance), L_.ptr(scale_c), bn, spp, L_.ptr(cd),
                                          L_.ptr(cs), L_.stream_ptr()), "i2sdf_shade_reduce")
        ctx.st, ctx.radiance, ctx.scale = st, radiance, scale_c
        return cd, cs

    @staticmethod
    def backward(ctx, g_cd, g_cs):
        zeros = lambda: torch.zeros(ctx.st["bn"], 3, dtype=torch.float32, device=ctx.st["dev"])
        g_cd = zeros() if g_cd is None else g_cd
        g_cs = zeros() if g_cs is None else g_cs
        want_rad = ctx.needs_input_grad[3]
        want_scale = ctx.scale is not None and ctx.needs_input_grad[4]
        gKd, gKs, grough, g_rad, g_scale = _backward(ctx.st, ctx.radiance, ctx.scale, g_cd, g_cs, None, None, want_rad, want_scale)
        return gKd, gKs, grough, g_rad, g_scale, None


class RenderingLayer(torch.nn.Module):
    """The reference's RenderingLayer(spp, split_n_pixels, preserve_light=True); `preserve_light` is accepted and unused, as there."""

    def __init__(self, spp: int, split_n_pixels: int, preserve_light: bool = True) -> None:
        super().__init__()
        self.spp = int(spp)
        self.split_n_pixels = int(split_n_pixels)
        self.preserve_light = preserve_light

    def forward(self, model, surface_points, view_direction, Kd, Ks, normal, rough, radiance_scale=None, intersect_func=None,
                samples: Optional[torch.Tensor] = None):
        """-> (colorDiffuse (bn, 3), colorSpec (bn, 3), wi_mask (bn) bool).  All inputs (bn, c) float32 on one ROCm device; rough (bn, 1);
        radiance_scale (3) or None.  samples: explicit uniforms (bn, spp, 3) in [0, 1); by default a 62-bit seed is taken from torch's CPU
        generator (torch.manual_seed decides the run) and the kernels draw from it (i2sdf_amd.shade_draws shows what).

        Gradients reach Kd, Ks, rough and radiance_scale, and the model's radiance and the rays' direction / origin where the model's
        output and inputs carry a graph.  normal, view_direction and surface_points are constants of this stage."""
        if not isinstance(normal, torch.Tensor) or normal.dim() != 2:
            raise ValueError("RenderingLayer takes (bn, c) inputs; image-shaped inputs with trailing h, w are not supported: flatten them first")
        dev = normal.device
        if dev.type != "cuda":
            raise L_.I2SDFError("RenderingLayer needs a ROCm device (there is no CPU path)")
        for name, t in (("normal", normal), ("view_direction", view_direction), ("surface_points", surface_points)):
            if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError(f"{name} requires grad: the geometry is frozen at the material stage, RenderingLayer has no gradient "
                                          f"by normal, view_direction or surface_points -- detach it")
        bn, spp = int(normal.shape[0]), self.spp
        st = {"bn": bn, "spp": spp, "dev": dev, "x": _f32(surface_points, "surface_points", (bn, 3), dev),
              "view": _f32(view_direction, "view_direction", (bn, 3), dev), "normal": _f32(normal, "normal", (bn, 3), dev),
              "Kd": _f32(Kd, "Kd", (bn, 3), dev), "Ks": _f32(Ks, "Ks", (bn, 3), dev), "rough": _f32(rough, "rough", (bn, 1), dev)}
        if radiance_scale is not None:
            _f32(radiance_scale, "radiance_scale", (3,), dev)
        if samples is not None:
            st["samples"], st["seed"] = _f32(samples, "samples", (bn, spp, 3), dev), None
        else:
            st["samples"], st["seed"] = None, int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        direction, points, wi_mask = _SampleFn.apply(rough, st)
        radiance = [model.get_incident_radiance(p_, d_, intersect_func)
                    for p_, d_ in zip(torch.split(points, self.split_n_pixels, dim=0), torch.split(direction, self.split_n_pixels, dim=0))]
        radiance = torch.cat(radiance, dim=0) if radiance else points.new_zeros(0, 3)
        if tuple(radiance.shape) != (bn * spp, 3) or radiance.device != dev:
            raise ValueError(f"model.get_incident_radiance returned {tuple(radiance.shape)} on {radiance.device} in all, expected {(bn * spp, 3)} on {dev}")
        colorDiffuse, colorSpec = _ReduceFn.apply(Kd, Ks, rough, radiance.to(torch.float32), radiance_scale, st)
        return colorDiffuse, colorSpec, wi_mask


def get_rendering_parameters(albedo_raw, rough_raw, use_metallic):
    """The two material parametrisations of the reference (model/rendering/brdf.py): -> Kd, Ks, rough.
    use_metallic: albedo_raw (bn, 3) base colour, rough_raw (bn, 2) = [roughness, metalness]: Ks = lerp(0.04, base, metal), Kd = base (1 - metal).
    otherwise:    albedo_raw (bn, 6) = [Kd | Ks], rough_raw (bn, 1): Ks floored at 0.04.  rough is floored at 0.01 in both."""
    width = (int(albedo_raw.shape[-1]), int(rough_raw.shape[-1]))
    if width != ((3, 2) if use_metallic else (6, 1)):
        raise ValueError(f"get_rendering_parameters(use_metallic={bool(use_metallic)}): albedo_raw / rough_raw have {width} channels, "
                         f"expected {(3, 2) if use_metallic else (6, 1)}")
    rough = rough_raw[:, :1].clamp_min(0.01)
    if use_metallic:
        metal = rough_raw[:, 1:]
        return albedo_raw * (1 - metal), torch.lerp(torch.full_like(albedo_raw, 0.04), albedo_raw, metal), rough
    return albedo_raw[:, :3], albedo_raw[:, 3:].clamp_min(0.04), rough
