"""Configuration of the render core: reads the same yaml keys the reference's I2SDFNetwork ctor reads
(model/network/__init__.py:20-47) and derives the layer shapes (model/network/mlp.py:31-53,176-198)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple


def _get(node, key, default=None):
    if node is None:
        return default
    if isinstance(node, dict):
        return node.get(key, default)
    return getattr(node, key, default)


def _has(node, key):
    if isinstance(node, dict):
        return key in node
    return hasattr(node, key)


MAX_HIDDEN_LAYERS = 11      # include/i2sdf.h: I2SDF_MAX_LAYERS (12) linear layers per net, the output layer among them


def _check_depth(key, dims):
    if not 1 <= len(dims) <= MAX_HIDDEN_LAYERS:
        raise NotImplementedError(f"{key} has {len(dims)} hidden layers: the plan's descriptor and the kernels' layer loops hold 1..{MAX_HIDDEN_LAYERS} "
                                  f"hidden layers per net (include/i2sdf.h: I2SDF_MAX_LAYERS = {MAX_HIDDEN_LAYERS + 1} linear layers)")


@dataclass
class MlpShape:
    """One weight-normed nn.Linear stack."""
    name: str                       # state_dict prefix: implicit_network / rendering_network / light_network
    dims: List[Tuple[int, int]]     # (out, in) per layer
    hidden: int
    d_in: int
    multires: int
    skip_layer: int = -1
    # rendering_network.embed_type (embedder.py:138-160): 'positional' (multires above; 0 = none), or 'spherical_harmonics' / 'fourier' with
    # their parameter -- the degree (1..5) or the channel count (1..12); multires is then 0
    embed: str = "positional"
    embed_n: int = 0

    @property
    def embed_dim(self):
        """width of the embedded view direction of a radiance net with an SH / Fourier embedder"""
        return self.embed_n ** 2 if self.embed == "spherical_harmonics" else 2 * self.embed_n + 3

    @property
    def n_lin(self):
        return len(self.dims)

    @property
    def pe_dim(self):
        """width of the encoded input in front of the hidden / feature columns of layer 0 (csrc/plan.h: side_dim); a radiance net in 'idr'
        mode (d_in 9) encodes only the view direction: [x | PE(view) | normal]"""
        raw = 3 if self.d_in == 9 else self.d_in
        if self.embed != "positional":
            return self.embed_dim + (self.d_in - raw)
        return (raw + 2 * raw * self.multires if self.multires > 0 else raw) + (self.d_in - raw)


@dataclass
class SamplerConfig:
    """model/network/ray_sampler.py:47-61"""
    near: float = 0.0
    N_samples: int = 64
    N_samples_eval: int = 128
    N_samples_extra: int = 32
    eps: float = 0.1
    beta_iters: int = 10
    max_total_iters: int = 5
    add_tiny: float = 0.0


@dataclass
class NetConfig:
    feature_size: int
    sdf: MlpShape
    rgb: MlpShape
    light: Optional[MlpShape]
    sampler: SamplerConfig
    scene_bounding_sphere: float = 1.0
    beta_init: float = 0.1
    beta_min: float = 1e-4
    sdf_bias: float = 1.0
    use_normal: bool = False
    detach_light_feature: bool = True
    rgb_mode: str = "nerf"
    # rendering_network.output_activation (mlp.py:153-157, 206, 227): 'sigmoid', or 'relu' / 'softplus' for radiance above 1 (HDR targets)
    rgb_act: str = "sigmoid"
    # rendering_network.sigma of a Fourier view embedder: the scale of its random matrix B ~ N(0, sigma^2) (embedder.py:128)
    rgb_embed_sigma: float = 1.0
    # arithmetic of the MFMA kernels that have a bf16x3 twin (csrc/x3.h): fp32 operands split into three bf16 terms, six
    # partial products accumulated in fp32 -- fp32-level accuracy (same parity bar) on the 16x faster bf16 matrix pipe.
    # `bf16x3: false` in the model conf selects the plain fp32-MFMA kernels everywhere.
    bf16x3: bool = True
    # The weight-gradient GEMMs (256x256 blocks) with TWO bf16 terms per operand and three products instead of three and six
    # (include/i2sdf.h: I2SDF_OPT_WGRAD_BF16X2).  Weight gradients are terminal sums over ~1e5 points -- their rounding errors average out
    # and propagate nowhere; measured 3e-6 of the fp64 oracle on every parameter gradient (bar 1e-4), above the reference's own
    # float32_matmul_precision('medium') (main_recon.py:61).  Forward and backward ACTIVATIONS always keep the fp32-equivalent bf16x3
    # form.  `wgrad_bf16x2: false` in the model conf (or I2SDF_WGRAD_BF16X2=0) selects the fp32-equivalent form here too.
    wgrad_bf16x2: bool = True
    # The sampler's sdf-only passes with TWO bf16 terms per operand (include/i2sdf.h: I2SDF_OPT_SAMPLER_BF16X2).  These passes run under
    # no_grad and only CHOOSE the depths (ray_sampler.py:83-95); every returned value is computed at the chosen depths by the fp32-equivalent
    # kernels.  Round 6 ran the WHOLE GPU suite with the option on before making it the default (profiles/r6_sampler_x2.txt: 198 passed --
    # G7's iteration counts exact, the depth bars of tests/test_gpu_sampler.py, G8/G9/G14/G15 end-to-end at 1e-4): sampler entry point
    # 1.09 -> 0.67 ms, step 5.42 -> 4.97 ms, a 640x480 eval render 1.18 -> 0.86 s.  `sampler_bf16x2: false` (or I2SDF_SAMPLER_BF16X2=0)
    # selects the three-plane form here too.
    sampler_bf16x2: bool = True
    # abars, G(hbar), G(a) of the SDF net -- the saved tensors whose consumers keep 16 significant bits of them anyway (the two-plane
    # weight-gradient GEMMs) or use them in the second-order injection only -- stored with 16 significant bits in 3 bytes per value
    # (include/i2sdf.h: I2SDF_OPT_SAVES24; csrc/x3.h P24).  Effective only together with `wgrad_bf16x2` and the point ranges; with
    # `wgrad_bf16x2: false` (the fp32-equivalent mode) these tensors keep fp32 storage.  `saves24: false` (or I2SDF_SAVES24=0) keeps fp32 storage here too.
    saves24: bool = True

    @staticmethod
    def from_conf(conf) -> "NetConfig":
        fvs = int(_get(conf, "feature_vector_size"))
        inet, rnet = _get(conf, "implicit_network"), _get(conf, "rendering_network")
        if _has(conf, "bg_network"):
            raise NotImplementedError("bg_network (inverse-sphere background) is outside the accelerated hot path")
        # --- ImplicitNetwork (mlp.py:31-53)
        d_in, d_out = int(_get(inet, "d_in")), int(_get(inet, "d_out"))
        if _get(inet, "embed_type", None) not in ("positional",):
            raise NotImplementedError("only embed_type='positional' is accelerated (the shipped configs)")
        if not _get(inet, "weight_norm", True) or not _get(rnet, "weight_norm", True):
            raise NotImplementedError("weight_norm=False is not supported")
        multires = int(_get(inet, "multires"))
        hid = list(_get(inet, "dims"))
        skip_in = tuple(_get(inet, "skip_in", ()))
        if len(skip_in) > 1:
            raise NotImplementedError("at most one skip connection")
        _check_depth("implicit_network.dims", hid)
        _check_depth("rendering_network.dims", list(_get(rnet, "dims")))
        if skip_in and not 1 <= int(skip_in[0]) < len(hid):
            raise NotImplementedError(
                f"implicit_network.skip_in {list(skip_in)} with {len(hid)} hidden layers: the SDF kernels concatenate PE(x) in front of a hidden "
                f"layer behind the first one -- {f'entries 1..{len(hid) - 1}' if len(hid) > 1 else 'no entry'} here (layer 0 reads PE(x) "
                f"already; entry {len(hid)} would be the output layer, which the kernels evaluate as row vectors over the hidden width)")
        pe = d_in + 2 * d_in * multires
        full = [pe] + hid + [d_out + fvs]
        dims = []
        for l in range(len(full) - 1):
            out = full[l + 1] - full[0] if (l + 1) in skip_in else full[l + 1]
            dims.append((out, full[l]))
        if len(set(hid)) != 1:
            raise NotImplementedError("hidden widths must be uniform")
        sdf = MlpShape("implicit_network", dims, hid[0], d_in, multires, skip_in[0] if skip_in else -1)
        # --- RenderingNetwork (mlp.py:176-198)
        if _get(inet, "output_activation", None) is not None:
            raise NotImplementedError("implicit_network.output_activation: the reference applies it to the whole [sdf | feature] output "
                                      "(model/network/mlp.py:102-103); no kernel here does, and no shipped config sets it")
        act = _get(rnet, "output_activation", None)
        act = "sigmoid" if act is None else act          # (mlp.py:170: the default)
        if act not in ("sigmoid", "relu", "softplus"):
            raise NotImplementedError(f"rendering_network.output_activation must be one of 'sigmoid', 'relu', 'softplus' (the reference's "
                                      f"`activations` table, model/network/mlp.py:153-157, has no other entry); got {act!r}")
        mode = _get(rnet, "mode")
        if mode not in ("nerf", "idr"):
            raise NotImplementedError("rendering_network.mode must be 'nerf' (the shipped configs) or 'idr' (their documented two-line switch)")
        if mode == "idr" and _get(rnet, "embed_point", None) is not None:
            raise NotImplementedError("rendering_network.embed_point: the reference builds that embedder and widens lin0 for it, but never "
                                      "applies it in forward() (model/network/mlp.py:185-190, 208-216: the raw points are concatenated), so the "
                                      "option cannot run there either")
        # the view embedder (mlp.py:179-183 -> embedder.py:138-160): every other key of the node reaches the embedder's constructor
        etype = _get(rnet, "embed_type", None)
        embed, embed_n, sigma = "positional", 0, 1.0
        if etype in ("spherical_harmonics", "fourier"):
            if _has(rnet, "multires"):
                raise NotImplementedError(f"rendering_network.multires beside embed_type {etype!r}: the reference hands it to that embedder's constructor, "
                                          "which has no such argument (a TypeError there, mlp.py:181); remove the key")
            if etype == "spherical_harmonics":
                embed_n = int(_get(rnet, "degree", 4))         # (SHEncoder's default)
                if not 1 <= embed_n <= 5:
                    raise NotImplementedError(f"rendering_network.degree must be 1..5 (the reference's SHEncoder asserts it, embedder.py:50); got {embed_n}")
            else:
                if not _has(rnet, "channels"):
                    raise NotImplementedError("rendering_network.embed_type 'fourier' needs `channels` (FourierFeature has no default, embedder.py:126)")
                embed_n = int(_get(rnet, "channels"))
                if not 1 <= embed_n <= 12:
                    raise NotImplementedError(f"rendering_network.channels must be 1..12: the embedding [v | sin | cos] is 2 c + 3 wide and the radiance "
                                              f"net's side row has 27 view columns; got {embed_n}")
                if not _get(rnet, "include_input", True):
                    raise NotImplementedError("rendering_network.include_input: false (a Fourier embedding without the raw direction) is not supported")
                sigma = float(_get(rnet, "sigma", 1.0))
            embed = etype
        elif etype not in (None, False, "", "positional"):
            raise NotImplementedError(f"rendering_network.embed_type must be 'positional', 'spherical_harmonics' or 'fourier' (the reference's "
                                      f"get_embedder, model/network/embedder.py:138-160, has no other entry); got {etype!r}")
        mr_v = int(_get(rnet, "multires", 0)) if etype and embed == "positional" else 0
        rhid = list(_get(rnet, "dims"))
        r_d_in = int(_get(rnet, "d_in"))
        if mode == "idr" and r_d_in != 9:
            raise NotImplementedError(f"rendering_network.d_in must be 9 (points, view directions, normals) in 'idr' mode; got {r_d_in}")
        r_in = r_d_in + fvs + (6 * mr_v if mr_v else 0)
        if embed != "positional":
            r_in = r_d_in + fvs + (embed_n ** 2 if embed == "spherical_harmonics" else 2 * embed_n + 3) - 3
        rfull = [r_in] + rhid + [int(_get(rnet, "d_out"))]
        rgb = MlpShape("rendering_network", [(rfull[l + 1], rfull[l]) for l in range(len(rfull) - 1)], rhid[0], 9 if mode == "idr" else 3, mr_v,
                       embed=embed, embed_n=embed_n)
        light = None
        if _has(conf, "light_network"):
            lhid = list(_get(_get(conf, "light_network"), "dims"))
            if lhid not in ([128], [32]) or (fvs, lhid[0]) not in ((256, 128), (64, 32)):
                raise NotImplementedError(
                    f"light_network.dims {lhid} at feature_vector_size {fvs}: the light head's kernels are instantiated for one hidden layer of 128 "
                    "at feature size 256 (synthetic_light_mask.yml) and of 32 at feature size 64 (plumbing size) only; add an instantiation in "
                    "csrc/mlp_train.hip (light_fwd_kernel, light_bwd_kernel) for another head")
            lfull = [fvs] + lhid + [1]
            light = MlpShape("light_network", [(lfull[l + 1], lfull[l]) for l in range(len(lfull) - 1)], lhid[0], fvs, 0)
        rs = _get(conf, "ray_sampler")
        sam = SamplerConfig(near=float(_get(rs, "near")), N_samples=int(_get(rs, "N_samples")),
                            N_samples_eval=int(_get(rs, "N_samples_eval")), N_samples_extra=int(_get(rs, "N_samples_extra")),
                            eps=float(_get(rs, "eps")), beta_iters=int(_get(rs, "beta_iters")),
                            max_total_iters=int(_get(rs, "max_total_iters")), add_tiny=float(_get(rs, "add_tiny", 0.0)))
        # --- what the kernels are instantiated for (csrc): anything else is refused HERE, with the reason, not at the first launch
        if not ((hid[0] == 256 and fvs == 256 and rhid[0] == 256) or (hid[0] == 64 and fvs == 64 and rhid[0] == 64)):
            raise NotImplementedError(
                f"hidden width {hid[0]} / feature size {fvs} / radiance width {rhid[0]}: the MLP kernels are instantiated for 256/256/256 "
                "(synthetic.yml, synthetic_light_mask.yml: bf16x3 and fp32 MFMA) and 64/64/64 (plumbing size, fp32 MFMA) only -- one wave holds "
                "a whole layer's accumulators in registers (2 x width/32 x 16 of 512), which 512-wide layers do not fit; add an "
                "instantiation in csrc/mlp_*.hip and csrc/plan.cpp for another width")
        if len(set(rhid)) != 1:
            raise NotImplementedError("radiance hidden widths must be uniform")
        if multires != 6 or (embed == "positional" and mr_v not in (0, 4)):
            raise NotImplementedError(f"positional encodings are instantiated for multires 6 (SDF net) and 4 (view directions); got {multires} / {mr_v}")
        if sam.N_samples_eval > 128 or sam.N_samples > 128 or sam.N_samples_eval * sam.max_total_iters > 640 or sam.max_total_iters > 12 \
                or sam.N_samples + sam.N_samples_extra + 2 > 256:
            raise NotImplementedError(
                f"ray_sampler N_samples_eval={sam.N_samples_eval}, N_samples={sam.N_samples}, N_samples_extra={sam.N_samples_extra}, "
                f"max_total_iters={sam.max_total_iters}: the sampler kernels hold a ray's row in the registers of one wave, compiled for at most "
                "128 new samples per iteration, rows of N_samples_eval * max_total_iters <= 640 depths and N_samples + N_samples_extra + 2 <= 256 "
                "output depths (csrc/sampler.hip: NNEW, NMAX; the shipped configs use 128 / 64 / 32 / 5)")
        dens = _get(conf, "density")
        return NetConfig(feature_size=fvs, sdf=sdf, rgb=rgb, light=light, sampler=sam,
                         scene_bounding_sphere=float(_get(conf, "scene_bounding_sphere", 1.0)),
                         beta_init=float(_get(_get(dens, "params_init"), "beta")), beta_min=float(_get(dens, "beta_min", 1e-4)),
                         sdf_bias=float(_get(inet, "bias", 1.0)), use_normal=bool(_get(conf, "use_normal", False)),
                         detach_light_feature=bool(_get(conf, "detach_light_feature", True)), rgb_mode=mode, rgb_act=act, rgb_embed_sigma=sigma,
                         bf16x3=bool(_get(conf, "bf16x3", True)), wgrad_bf16x2=bool(_get(conf, "wgrad_bf16x2", True)),
                         sampler_bf16x2=bool(_get(conf, "sampler_bf16x2", True)), saves24=bool(_get(conf, "saves24", True)))


def synthetic_conf(light: bool = False) -> dict:
    """The `model:` node of config/synthetic.yml (synthetic_light_mask.yml when light=True) as a plain dict."""
    n_sdf, n_rgb, skip = (6, 3, 3) if light else (8, 4, 4)
    conf = {
        "feature_vector_size": 256, "scene_bounding_sphere": 3.0,
        "implicit_network": {"d_in": 3, "d_out": 1, "dims": [256] * n_sdf, "geometric_init": True, "bias": 0.6, "skip_in": [skip],
                             "weight_norm": True, "embed_type": "positional", "multires": 6},
        "rendering_network": {"mode": "nerf", "d_in": 3, "d_out": 3, "dims": [256] * n_rgb, "weight_norm": True,
                              "embed_type": "positional", "multires": 4},
        "density": {"params_init": {"beta": 0.1}, "beta_min": 0.0001},
        "ray_sampler": {"near": 0.0, "N_samples": 64, "N_samples_eval": 128, "N_samples_extra": 32, "eps": 0.1, "beta_iters": 10,
                        "max_total_iters": 5, "N_samples_inverse_sphere": 32, "add_tiny": 1.0e-6},
    }
    if light:
        conf["light_network"] = {"dims": [128], "weight_norm": True}
    return conf


def plumbing_conf(skip: bool = False, light: bool = False) -> dict:
    """BASELINE.json configs[0]: 2-layer x 64 SDF MLP, 16 samples/ray."""
    conf = synthetic_conf(light)
    conf["feature_vector_size"] = 64
    conf["implicit_network"]["dims"] = [64, 64, 64] if skip else [64, 64]
    conf["implicit_network"]["skip_in"] = [2] if skip else []
    conf["rendering_network"]["dims"] = [64, 64]
    conf["ray_sampler"].update({"N_samples": 16, "N_samples_eval": 32, "N_samples_extra": 8})
    if light:
        conf["light_network"] = {"dims": [32], "weight_norm": True}
    return conf
