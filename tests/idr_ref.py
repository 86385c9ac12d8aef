"""Plain-torch restatement of the reference's radiance net in 'idr' mode (model/network/mlp.py:185-216) and of the forward / training
step around it (model/network/__init__.py:99-221 with `returns_grad = use_normal or not training or mode == 'idr'`, :109,115).
dtype-generic (fp32 / fp64), gradients by autograd.  Everything the mode does not change -- SDF net, sampler, density, compositing,
loss -- is the oracle's (oracle/i2sdf_oracle.py, which is 'nerf'-only and stays so)."""
import math
from typing import Dict, Optional

import torch

from oracle import i2sdf_oracle as orc

Tensor = torch.Tensor


def idr_conf(conf: dict, multires: int = 4) -> dict:
    """the two-line switch config/synthetic.yml:47-52 documents, applied to a `model:` node; multires 0: without the view encoding
    (embed_type: null, mlp.py:179-183)"""
    conf = {k: (dict(v) if isinstance(v, dict) else v) for k, v in conf.items()}
    conf["rendering_network"].update({"mode": "idr", "d_in": 9})
    if multires == 0:
        conf["rendering_network"].update({"embed_type": None, "multires": 0})
    return conf


def view0(cfg: orc.NetCfg) -> orc.NetCfg:
    """the oracle configuration with unencoded view directions"""
    cfg.rgb.multires_view = 0
    return cfg


def init_params(cfg: orc.NetCfg, seed: int = 0, dtype=torch.float32) -> Dict[str, Tensor]:
    """orc.init_params with the radiance net's first layer widened to d_in 9 (nn.Linear default init, as the reference's)"""
    sd = orc.init_params(cfg, seed=seed, dtype=dtype)
    gen = torch.Generator().manual_seed(seed + 7919)
    out, inn = cfg.rgb.dims[0], 9 + 6 * cfg.rgb.multires_view + cfg.rgb.feature_size
    bound = 1.0 / math.sqrt(inn)
    W = (torch.rand(out, inn, generator=gen, dtype=torch.float64) * 2 - 1) * bound
    sd["rendering_network.lin0.bias"] = ((torch.rand(out, generator=gen, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
    sd["rendering_network.lin0.weight_g"] = W.norm(dim=1, keepdim=True).to(dtype)
    sd["rendering_network.lin0.weight_v"] = W.to(dtype)
    return sd


def rgb_forward(sd, cfg: orc.RgbCfg, points: Tensor, normals: Tensor, view_dirs: Tensor, feat: Tensor,
                prefix: str = "rendering_network") -> Tensor:
    """mlp.py:208-229, mode 'idr': cat[points, PE(view_dirs), normals, feature] -> ReLU stack -> sigmoid (honours orc.relu_hook)"""
    h = torch.cat([points, orc.positional_encode(view_dirs, cfg.multires_view), normals, feat], dim=-1)
    for l in range(cfg.n_lin):
        h = torch.nn.functional.linear(h, orc.effective_weight(sd, f"{prefix}.lin{l}"), sd[f"{prefix}.lin{l}.bias"])
        if l < cfg.n_lin - 1:
            h = torch.relu(h) if orc._RELU_HOOK is None else orc._RELU_HOOK(h, l)
    return torch.sigmoid(h)


def rgb_grads(sd, cfg: orc.RgbCfg, points, normals, view_dirs, feat, rgb_bar):
    """autograd through rgb_forward for the upstream gradient rgb_bar: -> (rgb, fbar, nbar_rgb, {radiance parameter: gradient})"""
    names = [k for k in sd if k.startswith("rendering_network.")]
    p = {k: v.detach().clone().requires_grad_(k in names) for k, v in sd.items()}
    f, n = feat.detach().clone().requires_grad_(True), normals.detach().clone().requires_grad_(True)
    rgb = rgb_forward(p, cfg, points, n, view_dirs, f)
    g = torch.autograd.grad(rgb, [f, n] + [p[k] for k in names], rgb_bar)
    return rgb.detach(), g[0], g[1], dict(zip(names, g[2:]))


def network_forward(sd, cfg: orc.NetCfg, inputs: Dict[str, Tensor], training: bool, draws: Optional[orc.Draws] = None,
                    predict_only: bool = False, z_override=None, detach_rgb_normals: bool = False) -> Dict[str, Tensor]:
    """orc.network_forward with the 'idr' radiance net: d sdf/dx is always formed (with a graph in training) and, unnormalised, is an
    input of the radiance net together with the sample points.  detach_rgb_normals: the radiance net sees the normals as constants -- what
    an implementation that dropped d loss / d normal through the radiance net would differentiate (tests measure that part with it)."""
    cam, dirs, dnorm = orc.prepare_rays(inputs["uv"], inputs["pose"], inputs["intrinsics"])
    draws = draws or orc.Draws()
    z_all, z_eik = orc.sample_z_vals(sd, cfg, dirs, cam, training, draws) if z_override is None else z_override
    z_max, z_vals = z_all[:, -1], z_all[:, :-1]
    n = z_vals.shape[1]
    pts = (cam.unsqueeze(1) + z_vals.unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
    dirs_flat = dirs.unsqueeze(1).repeat(1, n, 1).reshape(-1, 3)
    sdf, feat, grads = orc.sdf_outputs(sd, cfg.sdf, pts, create_graph=training)
    rgb = rgb_forward(sd, cfg.rgb, pts, grads.detach() if detach_rgb_normals else grads, dirs_flat, feat).reshape(-1, n, 3)
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
        nrm = torch.nn.functional.normalize(g[nb:], dim=1, eps=1e-6)
        out["diff_norm"] = torch.norm(nrm[:nb] - nrm[nb:], dim=1)
        if cfg.use_normal:
            nm = torch.nn.functional.normalize(grads, dim=-1).reshape(-1, n, 3)
            out["normal_values"] = torch.nn.functional.normalize(torch.sum(w.unsqueeze(-1).detach() * nm, 1), dim=-1)
    else:
        nm = torch.nn.functional.normalize(grads.detach(), dim=-1).reshape(-1, n, 3)
        out["normal_map"] = torch.nn.functional.normalize(torch.sum(w.unsqueeze(-1) * nm, 1), dim=-1)
    return out


def training_step_grads(sd, cfg: orc.NetCfg, inputs, gt, lc: orc.LossCfg, draws: orc.Draws, step: int = 0, z_override=None,
                        detach_rgb_normals: bool = False):
    """forward + loss + backward by autograd: (outputs, loss dict, {parameter: gradient}) -- orc.training_step_grads for this mode"""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out = network_forward(params, cfg, inputs, True, draws, z_override=z_override, detach_rgb_normals=detach_rgb_normals)
    losses = orc.i2sdf_loss(out, gt, lc, step)
    names = list(params.keys())
    grads = torch.autograd.grad(losses["loss"], [params[k] for k in names], allow_unused=True)
    return out, losses, {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(names, grads)}
