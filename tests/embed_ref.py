"""Plain-torch restatement of the reference's two other view embedders -- spherical harmonics and Fourier features
(model/network/embedder.py:41-135, `rendering_network.embed_type`) -- and of the radiance net, the forward and the training step with them,
in 'nerf' and 'idr' mode.  dtype-generic (fp32 / fp64), gradients by autograd.  Everything the embedder does not change -- the radiance
layers, the SDF net, sampler, density, compositing, loss -- is hdr_ref's / idr_ref's / the oracle's (whose radiance nets are positional-only
and stay so).

An embedder is described by `Embed(kind, n, B)`: kind 'spherical_harmonics' with n = degree (1..5), or 'fourier' with n = channels and the
matrix B (3, n) -- a persistent buffer of the reference's module, state_dict key `rendering_network.embedview_fn.B`."""
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn.functional as F

import hdr_ref
from oracle import i2sdf_oracle as orc

Tensor = torch.Tensor
B_KEY = "rendering_network.embedview_fn.B"
KINDS = {"sh": "spherical_harmonics", "ff": "fourier"}

# SHEncoder's constants (embedder.py:54-82)
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]
C4 = [2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
      0.47308734787878004, -1.7701307697799304, 0.6258357354491761]


@dataclass
class Embed:
    kind: str                       # 'spherical_harmonics' | 'fourier'
    n: int                          # degree | channels
    B: Optional[Tensor] = None      # fourier: (3, n)

    @property
    def dim(self) -> int:
        return self.n ** 2 if self.kind == "spherical_harmonics" else 2 * self.n + 3


def parse(tag: str) -> Embed:
    """'sh4' -> spherical harmonics of degree 4, 'ff12' -> Fourier features with 12 channels (B to be filled in)"""
    return Embed(KINDS[tag[:2]], int(tag[2:]))


def spherical_harmonics(v: Tensor, degree: int) -> Tensor:
    """SHEncoder.forward (embedder.py:84-122), term by term in the reference's own polynomial forms and order of operations"""
    assert 1 <= degree <= 5
    x, y, z = v.unbind(-1)
    r = [torch.full_like(x, C0)]
    if degree > 1:
        r += [-C1 * y, C1 * z, -C1 * x]
    if degree > 2:
        xx, yy, zz = x * x, y * y, z * z
        xy, yz, xz = x * y, y * z, x * z
        r += [C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if degree > 3:
        r += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
              C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    if degree > 4:
        r += [C4[0] * xy * (xx - yy), C4[1] * yz * (3 * xx - yy), C4[2] * xy * (7 * zz - 1), C4[3] * yz * (7 * zz - 3),
              C4[4] * (zz * (35 * zz - 30) + 3), C4[5] * xz * (7 * zz - 3), C4[6] * (xx - yy) * (7 * zz - 1), C4[7] * xz * (xx - 3 * yy),
              C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(r, dim=-1)


def fourier(v: Tensor, B: Tensor) -> Tensor:
    """FourierFeature.forward (embedder.py:133-135) with include_input: [v | sin(2 pi v B) | cos(2 pi v B)]"""
    xp = torch.matmul(2 * math.pi * v, B.to(v.dtype))
    return torch.cat([v, torch.sin(xp), torch.cos(xp)], dim=-1)


def embed(v: Tensor, emb: Embed) -> Tensor:
    return spherical_harmonics(v, emb.n) if emb.kind == "spherical_harmonics" else fourier(v, emb.B)


def embed_of(sd, kind: str, n: int) -> Embed:
    """the embedder of a state_dict: B is read from its buffer key"""
    return Embed(kind, n, sd[B_KEY] if kind == "fourier" else None)


def embed_conf(conf: dict, emb: Embed, mode: str = "nerf", sigma: float = 1.0) -> dict:
    """a `model:` node with that view embedder in 'nerf' or 'idr' mode: `multires` leaves the node (the reference raises on it there)"""
    conf = hdr_ref.hdr_conf(conf, None, mode)
    r = conf["rendering_network"]
    r.pop("multires", None)
    r["embed_type"] = emb.kind
    if emb.kind == "spherical_harmonics":
        r["degree"] = emb.n
    else:
        r.update({"channels": emb.n, "sigma": sigma})
    return conf


def init_params(cfg: orc.NetCfg, emb: Embed, mode: str, seed: int = 0, dtype=torch.float32, sigma: float = 1.0) -> Dict[str, Tensor]:
    """orc.init_params with the radiance net's first layer as wide as the embedder makes it (nn.Linear default init, as the reference's) and,
    for Fourier features, B ~ N(0, sigma^2) in front of the radiance layers, where the reference's state_dict has it"""
    sd = orc.init_params(cfg, seed=seed, dtype=dtype)
    gen = torch.Generator().manual_seed(seed + 104729)
    out, inn = cfg.rgb.dims[0], emb.dim + (6 if mode == "idr" else 0) + cfg.rgb.feature_size
    bound = 1.0 / math.sqrt(inn)
    Bm = (torch.randn(3, emb.n, generator=gen, dtype=torch.float64) * sigma).to(dtype) if emb.kind == "fourier" else None
    W = (torch.rand(out, inn, generator=gen, dtype=torch.float64) * 2 - 1) * bound
    sd["rendering_network.lin0.bias"] = ((torch.rand(out, generator=gen, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
    sd["rendering_network.lin0.weight_g"] = W.norm(dim=1, keepdim=True).to(dtype)
    sd["rendering_network.lin0.weight_v"] = W.to(dtype)
    if Bm is None:
        return sd
    ordered = {}
    for k, v in sd.items():          # the buffer's key stands in front of rendering_network.lin0.* (mlp.py:179-203)
        if k == "rendering_network.lin0.bias":
            ordered[B_KEY] = Bm
        ordered[k] = v
    return ordered


def perturb_params(sd: Dict[str, Tensor], scale: float = 0.05, seed: int = 1) -> Dict[str, Tensor]:
    """orc.perturb_params on the parameters; the buffer B stays what it is"""
    out = orc.perturb_params({k: v for k, v in sd.items() if k != B_KEY}, scale, seed=seed)
    return {k: (sd[k] if k == B_KEY else out[k]) for k in sd}


def rgb_forward(sd, cfg: orc.RgbCfg, emb: Embed, view_dirs: Tensor, feat: Tensor, points: Optional[Tensor] = None,
                normals: Optional[Tensor] = None, prefix: str = "rendering_network", act: str = "sigmoid") -> Tensor:
    """mlp.py:208-229 with `embedview_fn` = the embedder.  'idr' mode when points and normals are given: cat[points, E(view), normals,
    feature]; else 'nerf': cat[E(view), feature].  Hidden ReLUs honour orc.relu_hook.  E has no gradient path: it is a function of the view
    direction and the constant B alone."""
    ev = embed(view_dirs, emb)
    h = torch.cat([ev, feat] if points is None else [points, ev, normals, feat], dim=-1)
    for l in range(cfg.n_lin):
        h = F.linear(h, orc.effective_weight(sd, f"{prefix}.lin{l}"), sd[f"{prefix}.lin{l}.bias"])
        if l < cfg.n_lin - 1:
            h = torch.relu(h) if orc._RELU_HOOK is None else orc._RELU_HOOK(h, l)
    return torch.sigmoid(h) if act == "sigmoid" else (torch.relu(h) if act == "relu" else F.softplus(h))


def first_activation(sd, cfg: orc.RgbCfg, emb: Embed, view_dirs, feat, points=None, normals=None, prefix="rendering_network") -> Tensor:
    """r_1 = relu(W_0 [side row | feature] + b_0): what the forward saves first"""
    ev = embed(view_dirs, emb)
    h = torch.cat([ev, feat] if points is None else [points, ev, normals, feat], dim=-1)
    return torch.relu(F.linear(h, orc.effective_weight(sd, f"{prefix}.lin0"), sd[f"{prefix}.lin0.bias"]))


def side_row(emb: Embed, view_dirs, points=None, normals=None) -> Tensor:
    """the per-point row in front of the features: E(view) or [x | E(view) | normal]"""
    ev = embed(view_dirs, emb)
    return ev if points is None else torch.cat([points, ev, normals], dim=-1)


def rgb_grads(sd, cfg: orc.RgbCfg, emb: Embed, view_dirs, feat, rgb_bar, points=None, normals=None):
    """autograd through rgb_forward for the upstream gradient rgb_bar: -> (rgb, fbar, nbar_rgb or None, {radiance parameter: gradient})"""
    names = [k for k in sd if k.startswith("rendering_network.") and k != B_KEY]
    p = {k: v.detach().clone().requires_grad_(k in names) for k, v in sd.items()}
    f = feat.detach().clone().requires_grad_(True)
    n = normals.detach().clone().requires_grad_(True) if normals is not None else None
    rgb = rgb_forward(p, cfg, emb, view_dirs, f, points, n)
    g = torch.autograd.grad(rgb, [f] + ([n] if n is not None else []) + [p[k] for k in names], rgb_bar)
    k0 = 2 if n is not None else 1
    return rgb.detach(), g[0], (g[1] if n is not None else None), dict(zip(names, g[k0:]))


def network_forward(sd, cfg: orc.NetCfg, emb: Embed, mode: str, inputs: Dict[str, Tensor], training: bool, draws: Optional[orc.Draws] = None,
                    predict_only: bool = False, z_override=None) -> Dict[str, Tensor]:
    """hdr_ref.network_forward (model/network/__init__.py:99-221) with the radiance net above"""
    cam, dirs, dnorm = orc.prepare_rays(inputs["uv"], inputs["pose"], inputs["intrinsics"])
    draws = draws or orc.Draws()
    z_all, z_eik = orc.sample_z_vals(sd, cfg, dirs, cam, training, draws) if z_override is None else z_override
    z_max, z_vals = z_all[:, -1], z_all[:, :-1]
    n = z_vals.shape[1]
    pts = (cam.unsqueeze(1) + z_vals.unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
    dirs_flat = dirs.unsqueeze(1).repeat(1, n, 1).reshape(-1, 3)
    idr = mode == "idr"
    if cfg.use_normal or (not training) or idr:                      # network/__init__.py:109
        sdf, feat, grads = orc.sdf_outputs(sd, cfg.sdf, pts, create_graph=training)
    else:
        o = orc.sdf_forward(sd, cfg.sdf, pts)
        sdf, feat, grads = o[:, :1], o[:, 1:], None
    rgb = rgb_forward(sd, cfg.rgb, emb, dirs_flat, feat, pts if idr else None, grads if idr else None).reshape(-1, n, 3)
    w, _ = orc.volume_weights(z_vals, z_max, sdf, orc.get_beta(sd, cfg))
    out = {"rgb_values": torch.sum(w.unsqueeze(-1) * rgb, 1), "depth_values": torch.sum(w * z_vals, 1) / torch.clamp(dnorm, min=1e-6),
           "weight_sum": torch.sum(w, -1, keepdim=True)}
    if cfg.light is not None:
        lm = orc.light_forward(sd, cfg.light, feat).reshape(-1, n, 1)
        out["light_mask"] = torch.sum(w.unsqueeze(-1).detach() * lm, 1)
    out["_z_vals"], out["_sdf"], out["_grad"] = z_all, sdf, grads
    if predict_only:
        return out
    if training:
        near_pts = (cam.unsqueeze(1) + z_eik.unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
        eik = torch.cat([draws.eik_pts, near_pts, near_pts + draws.nbr_off], 0)
        g = orc.sdf_gradient(sd, cfg.sdf, eik, create_graph=True)
        nb = near_pts.shape[0]
        out["grad_theta"] = g[: 2 * nb]
        nrm = F.normalize(g[nb:], dim=1, eps=1e-6)
        out["diff_norm"] = torch.norm(nrm[:nb] - nrm[nb:], dim=1)
        if cfg.use_normal:
            nm = F.normalize(grads, dim=-1).reshape(-1, n, 3)
            out["normal_values"] = F.normalize(torch.sum(w.unsqueeze(-1).detach() * nm, 1), dim=-1)
    else:
        nm = F.normalize(grads.detach(), dim=-1).reshape(-1, n, 3)
        out["normal_map"] = F.normalize(torch.sum(w.unsqueeze(-1) * nm, 1), dim=-1)
    return out


def training_step_grads(sd, cfg: orc.NetCfg, emb: Embed, mode: str, inputs, gt, lc: orc.LossCfg, draws: orc.Draws, step: int = 0, z_override=None):
    """forward + loss + backward by autograd: (outputs, loss dict, {parameter: gradient}); the buffer B is no parameter and gets none"""
    params = {k: (v.detach().clone().requires_grad_(True) if k != B_KEY else v.detach()) for k, v in sd.items()}
    out = network_forward(params, cfg, emb, mode, inputs, True, draws, z_override=z_override)
    losses = orc.i2sdf_loss(out, gt, lc, step)
    names = [k for k in params if k != B_KEY]
    grads = torch.autograd.grad(losses["loss"], [params[k] for k in names], allow_unused=True)
    return out, losses, {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(names, grads)}
