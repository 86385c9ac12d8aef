"""Sphere tracing of the learned surface: the argument checks of RenderEngine.trace_rays (usable without a device) and the
`intersect_func` object that I2SDFNetwork.get_incident_radiance accepts.  The marching rule is defined in include/i2sdf.h
("Sphere tracing"); tests/trace_ref.py restates it."""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import lib as L

TraceResult = namedtuple("TraceResult", ["t", "status", "steps"])
TraceResultF = namedtuple("TraceResultF", ["t", "status", "steps", "f_trace"])

HIT, MISS, UNRESOLVED, INSIDE = L.TRACE_HIT, L.TRACE_MISS, L.TRACE_UNRESOLVED, L.TRACE_INSIDE


def check_trace_cfg(eps=1e-4, max_steps=64, step_scale=1.0, route="auto") -> L.TraceCfg:
    """The limits of i2sdf_trace_cfg (include/i2sdf.h), refused here with the reason before anything reaches the library."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"trace_rays: eps = {eps!r} must be a positive finite number")
    if isinstance(step_scale, bool) or not isinstance(step_scale, (int, float)) or not (0 < step_scale <= 1):
        raise ValueError(f"trace_rays: step_scale = {step_scale!r} is outside (0, 1]")
    if isinstance(max_steps, bool) or not isinstance(max_steps, int) or not (1 <= max_steps <= L.TRACE_MAX_STEPS):
        raise ValueError(f"trace_rays: max_steps = {max_steps!r} must be an integer in 1..{L.TRACE_MAX_STEPS}")
    if route not in L.TRACE_ROUTES:
        raise ValueError(f"trace_rays: route = {route!r} is none of {sorted(L.TRACE_ROUTES)}")
    return L.TraceCfg(eps=float(eps), step_scale=float(step_scale), max_steps=int(max_steps), route=L.TRACE_ROUTES[route])


def check_trace_rays(cam_loc, dirs, t_min, t_max):
    """cam_loc, dirs (N, 3) floating point on one device; t_min / t_max a number or an (N,) tensor on that device.
    -> (cam_loc, dirs, t_min, t_max) as contiguous fp32 tensors, the bounds expanded to (N,)."""
    for name, t in (("cam_loc", cam_loc), ("dirs", dirs)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"trace_rays: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"trace_rays: {name} {tuple(t.shape)} must be (N, 3)")
        if not t.dtype.is_floating_point:
            raise ValueError(f"trace_rays: {name} is {t.dtype}, expected a floating-point tensor")
    if dirs.shape != cam_loc.shape:
        raise ValueError(f"trace_rays: cam_loc {tuple(cam_loc.shape)} and dirs {tuple(dirs.shape)} differ")
    if dirs.device != cam_loc.device:
        raise ValueError(f"trace_rays: cam_loc is on {cam_loc.device}, dirs on {dirs.device}")
    N, dev = cam_loc.shape[0], cam_loc.device
    bounds = []
    for name, b in (("t_min", t_min), ("t_max", t_max)):
        if isinstance(b, torch.Tensor):
            if tuple(b.shape) != (N,):
                raise ValueError(f"trace_rays: {name} {tuple(b.shape)} must be a number or ({N},)")
            if b.device != dev:
                raise ValueError(f"trace_rays: {name} is on {b.device}, the rays on {dev}")
            if not b.dtype.is_floating_point:
                raise ValueError(f"trace_rays: {name} is {b.dtype}, expected a floating-point tensor")
            bounds.append(b.detach().to(torch.float32).contiguous())
        elif isinstance(b, (int, float)) and not isinstance(b, bool):
            bounds.append(torch.full((N,), float(b), dtype=torch.float32, device=dev))
        else:
            raise TypeError(f"trace_rays: {name} must be a number or an ({N},) tensor, got {type(b).__name__}")
    c = lambda t: t.detach().to(torch.float32).contiguous()
    return c(cam_loc), c(dirs), bounds[0], bounds[1]


class SphereTracer:
    """The `intersect_func` of I2SDFNetwork.get_incident_radiance and RenderingLayer: bound to ONE module, it makes that module answer a
    secondary ray with the radiance at its first surface hit (render_surface) instead of a volume render.  Made by `net.sphere_tracer(**kw)`;
    kw are the keywords of RenderEngine.trace_rays (eps, max_steps, step_scale, route, t_min, t_max), checked when the tracer is made.
    Called directly, tracer(pts, dirs) returns net.trace_surface of those rays."""

    def __init__(self, net, **kw):
        unknown = set(kw) - {"eps", "max_steps", "step_scale", "route", "t_min", "t_max"}
        if unknown:
            raise TypeError(f"sphere_tracer: unknown keyword(s) {sorted(unknown)}")
        check_trace_cfg(**{k: v for k, v in kw.items() if k in ("eps", "max_steps", "step_scale", "route")})
        self.net, self.kw = net, dict(kw)

    def __call__(self, pts, dirs):
        return self.net.trace_surface(_rays_input(pts, dirs, "sphere_tracer"), **self.kw)


def _rays_input(pts, dirs, who):
    if not isinstance(pts, torch.Tensor) or not isinstance(dirs, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3 or dirs.shape != pts.shape:
        raise ValueError(f"{who}: pts {tuple(getattr(pts, 'shape', ()))} and dirs {tuple(getattr(dirs, 'shape', ()))} must both be (n, 3)")
    pts, dirs = pts.detach().to(torch.float32).contiguous(), dirs.detach().to(torch.float32).contiguous()
    return {"uv": pts, "rays": {"cam_loc": pts, "dirs": dirs, "dnorm": torch.ones(pts.shape[0], dtype=torch.float32, device=pts.device)}}


class MeshTracer:
    """An `intersect_func` that finds the hit on a triangle MESH (i2sdf_amd.ray_mesh_intersect: a BVH trace, no network pass) instead of
    marching the network: bound to ONE module, it makes that module answer a ray with the radiance net at the mesh hit -- one SDF +
    radiance pass at fma(t, d, o), the tail sphere tracing ends with.  Made by `net.mesh_tracer(mesh_or_bvh, t_min=0.0, t_max=None,
    cull="none")`; a bare mesh gets its tree built once, here.  t_max None: unbounded.  Called directly, tracer(pts, dirs) returns
    net.trace_surface of those rays.  The mesh is a snapshot: it does not follow the network's weights."""

    def __init__(self, net, mesh_or_bvh, t_min=0.0, t_max=None, cull="none"):
        from . import mesh as M
        if cull not in L.RAYCAST_CULL:
            raise ValueError(f"mesh_tracer: cull = {cull!r} is none of {sorted(L.RAYCAST_CULL)}")
        for name, b in (("t_min", t_min), ("t_max", t_max)):
            if b is None and name == "t_max":
                continue
            if isinstance(b, bool) or not isinstance(b, (int, float, torch.Tensor)):
                raise TypeError(f"mesh_tracer: {name} must be a number or a per-ray tensor, got {type(b).__name__}")
        self.net = net
        self.bvh = M.build_bvh(mesh_or_bvh)
        self.t_min, self.t_max, self.cull = t_min, (math.inf if t_max is None else t_max), cull

    def intersect(self, cam, dirs, lo=None, hi=None):
        """RayHits of rays lo..hi of (cam, dirs); per-ray bounds are cut to the same rows"""
        from . import mesh as M
        N = cam.shape[0]
        cut = lambda b: b[lo:hi] if isinstance(b, torch.Tensor) and b.dim() == 1 and b.shape[0] == N and lo is not None else b
        c, d = (cam, dirs) if lo is None else (cam[lo:hi], dirs[lo:hi])
        return M.ray_mesh_intersect(self.bvh, c, d, cut(self.t_min), cut(self.t_max), self.cull, False, "bvh")

    def __call__(self, pts, dirs):
        return self.net.trace_surface(_rays_input(pts, dirs, "mesh_tracer"), intersect_func=self)
