"""Plain-torch restatement of the reference's radiance net with `rendering_network.output_activation` 'sigmoid', 'relu' or 'softplus'
(model/network/mlp.py:153-157, 206, 227) in 'nerf' and 'idr' mode, of the forward / training step around it, and of the tone map its
validation applies to HDR images (utils/rend_util.py:linear_to_srgb behind clamp(0, 1); model/trainer/recon.py:320-350).
dtype-generic (fp32 / fp64), gradients by autograd.  Everything the activation does not change -- SDF net, sampler, density, compositing,
loss -- is the oracle's (oracle/i2sdf_oracle.py, which ends its radiance net in a sigmoid and stays so)."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

import idr_ref
from oracle import i2sdf_oracle as orc

Tensor = torch.Tensor
ACTS = ("sigmoid", "relu", "softplus")


def hdr_conf(conf: dict, act: Optional[str], mode: str = "nerf") -> dict:
    """a `model:` node with `rendering_network.output_activation: act` (None: the key is left out), in 'nerf' or 'idr' mode"""
    conf = idr_ref.idr_conf(conf) if mode == "idr" else {k: (dict(v) if isinstance(v, dict) else v) for k, v in conf.items()}
    if act is not None:
        conf["rendering_network"]["output_activation"] = act
    return conf


def init_params(cfg: orc.NetCfg, mode: str, seed: int = 0, dtype=torch.float32) -> Dict[str, Tensor]:
    return idr_ref.init_params(cfg, seed=seed, dtype=dtype) if mode == "idr" else orc.init_params(cfg, seed=seed, dtype=dtype)


def rgb_forward(sd, cfg: orc.RgbCfg, act: str, view_dirs: Tensor, feat: Tensor, points: Optional[Tensor] = None,
                normals: Optional[Tensor] = None, prefix: str = "rendering_network", return_pre: bool = False) -> Tensor:
    """mlp.py:208-229.  'idr' mode when points and normals are given: cat[points, PE(view_dirs), normals, feature]; else 'nerf':
    cat[PE(view_dirs), feature].  Hidden ReLUs honour orc.relu_hook; so does an output relu, as layer n_lin - 1 (a backward-mask flip of an
    output unit at zero within rounding is the same kind of event as one of a hidden unit)."""
    assert act in ACTS, act
    pe = orc.positional_encode(view_dirs, cfg.multires_view)
    h = torch.cat([pe, feat] if points is None else [points, pe, normals, feat], dim=-1)
    for l in range(cfg.n_lin):
        h = F.linear(h, orc.effective_weight(sd, f"{prefix}.lin{l}"), sd[f"{prefix}.lin{l}.bias"])
        if l < cfg.n_lin - 1:
            h = torch.relu(h) if orc._RELU_HOOK is None else orc._RELU_HOOK(h, l)
    if return_pre:
        return h
    if act == "relu":
        return torch.relu(h) if orc._RELU_HOOK is None else orc._RELU_HOOK(h, cfg.n_lin - 1)
    return torch.sigmoid(h) if act == "sigmoid" else F.softplus(h)


def network_forward(sd, cfg: orc.NetCfg, act: str, mode: str, inputs: Dict[str, Tensor], training: bool, draws: Optional[orc.Draws] = None,
                    predict_only: bool = False, z_override=None) -> Dict[str, Tensor]:
    """orc.network_forward / idr_ref.network_forward with the radiance net above (model/network/__init__.py:99-221)"""
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
    rgb = rgb_forward(sd, cfg.rgb, act, dirs_flat, feat, pts if idr else None, grads if idr else None).reshape(-1, n, 3)
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


def training_step_grads(sd, cfg: orc.NetCfg, act: str, mode: str, inputs, gt, lc: orc.LossCfg, draws: orc.Draws, step: int = 0, z_override=None):
    """forward + loss + backward by autograd: (outputs, loss dict, {parameter: gradient}) -- orc.training_step_grads with the activation"""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out = network_forward(params, cfg, act, mode, inputs, True, draws, z_override=z_override)
    losses = orc.i2sdf_loss(out, gt, lc, step)
    names = list(params.keys())
    grads = torch.autograd.grad(losses["loss"], [params[k] for k in names], allow_unused=True)
    return out, losses, {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(names, grads)}


def linear_to_srgb(x: Tensor, clamp: bool = True) -> Tensor:
    """utils/rend_util.py:9-10, behind `.clamp(0, 1)` as the validation applies it (model/trainer/recon.py: get_plot_data)"""
    x = x.clamp(0, 1) if clamp else x
    return torch.where(x <= 0.0031308, x * 12.92, 1.055 * (x.clamp_min(0) ** (1 / 2.4)) - 0.055)
