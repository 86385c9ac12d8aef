"""The network shapes at the edges of what `NetConfig.from_conf` accepts, shared by tests/test_shape_frontier.py (CPU) and
tests/test_gpu_shapes.py (GPU): the case table, the conf of a case, its inputs and the oracle's evaluation of them.

Depth and skip position select kernels, they are not only loop bounds (csrc/mlp_common.h: sdf_x3_path; csrc/plan.cpp: build_rgb):
a 256-wide SDF net runs the bf16x3 kernels (blocked saves, 24-bit records) only with n_lin >= 4 and the skip not at the last hidden
layer, a 256-wide radiance net only with at least two hidden layers, and each net decides for itself -- so one training step can mix
both layouts.  Every case keeps the sampler sizes of `plumbing_conf` (the sampler has its own stage tests)."""
from collections import namedtuple

import torch

from oracle import i2sdf_oracle as orc

Case = namedtuple("Case", "id width sdf_hidden skip_in rgb_hidden light")

CASES = [
    Case("c01_w256_s1_r1", 256, 1, [], 1, None),           # fewest layers: fp32 path for both nets; the reverse chain is only W0^T
    Case("c02_w256_s2k1_r2_l128", 256, 2, [1], 2, [128]),  # n_lin 3: fp32 SDF path; smallest bf16x3 radiance net; bf16x3 light head
    Case("c03_w256_s3k2_r3", 256, 3, [2], 3, None),        # n_lin 4, kept off the bf16x3 path only by skip = n_lin - 2
    Case("c04_w256_s3_r1", 256, 3, [], 1, None),           # smallest bf16x3 SDF net, no skip; fp32 radiance (point-major) beside blocked SDF saves
    Case("c05_w256_s3k1_r4", 256, 3, [1], 4, None),        # skip at the first layer that can have one
    Case("c06_w256_s8_r4_l128", 256, 8, [], 4, [128]),     # shipped depth without a skip
    Case("c07_w256_s8k6_r4", 256, 8, [6], 4, None),        # last skip position that stays on the bf16x3 path
    Case("c08_w256_s11k5_r11", 256, 11, [5], 11, None),    # I2SDF_MAX_LAYERS in both nets
    Case("c09_w64_s1_r1", 64, 1, [], 1, None),
    Case("c10_w64_s3k1_r3_l32", 64, 3, [1], 3, [32]),
    Case("c11_w64_s11k10_r11", 64, 11, [10], 11, None),    # maximum depth; skip at the last hidden layer
    Case("c12_w64_s5_r2_l32", 64, 5, [], 2, [32]),
]
BY_ID = {c.id: c for c in CASES}
LIGHT_CASES = [c.id for c in CASES if c.light]

# weights: orc.perturb_params(orc.init_params(cfg, SEEDS[0]), 0.05, SEEDS[1]).  11 / 12 are the seeds of tests/test_gpu_backward.py; a case
# takes the first of the pairs (11, 12), (21, 22), (31, 32), ... that meets both conditions of
# tests/test_shape_frontier.py::test_oracle_fp32_is_well_inside_the_bars -- conditions on the oracle alone.  What the earlier pairs miss:
#   case 11 with (11, 12): the fp32 and the fp64 oracle disagree by 1.6e-2 on rendering_network.lin3.weight_v, a flipped ReLU mask;
#   case 7 with (11, 12): point 39, unit 128 of rendering_network.lin0 has the pre-activation 5.4e-9 at a layer scale of 0.8 -- the fp32
#     oracle happens to agree with fp64 on its sign, the library (measured on an MI355X) does not: 6.6e-2 on that layer's three gradients in
#     both weight-gradient modes, every other tensor inside 1.2e-5;
#   cases 3, 5, 6, 8: a radiance pre-activation within 2^-20 of its layer's scale (2e-8 .. 4e-7 at scales 0.1 .. 0.8).
SEEDS = {c.id: (11, 12) for c in CASES}
SEEDS.update({"c03_w256_s3k2_r3": (41, 42), "c05_w256_s3k1_r4": (31, 32), "c06_w256_s8_r4_l128": (31, 32), "c07_w256_s8k6_r4": (21, 22),
              "c08_w256_s11k5_r11": (41, 42), "c11_w64_s11k10_r11": (21, 22)})
# the points are uniform in [-X_SCALE, X_SCALE]^3.  Softplus(beta = 100) makes d sdf / d a_l of a deep net as sensitive to the rounding of
# a_l as 100 |a_l|: with the points in [-1.5, 1.5]^3 the oracle's own fp32 and fp64 runs differ by 6e-6 .. 1e-5 on abar of the last hidden
# layer of the 6-, 9- and 12-layer nets whatever the seeds (half of the 2e-5 bar); in [-0.5, 0.5]^3 by at most 3e-6.
# tests/test_shape_frontier.py::test_oracle_fp32_is_well_inside_the_bars holds seeds and points to a quarter of the bars.
X_SCALE = 0.5
M, B, N_PER_RAY, M_TAIL = 333, 37, 9, 37          # three 128-point workgroups, the last one ragged; the last 37 points carry no feature gradient
TOL_OUT, TOL_GRAD = 2e-5, 1e-4                    # tests/test_gpu_train_forward.py: TOL; tests/test_gpu_backward.py


def base_conf(width):
    from i2sdf_amd.config import synthetic_conf, plumbing_conf
    conf = synthetic_conf() if width == 256 else plumbing_conf()
    conf["ray_sampler"].update(plumbing_conf()["ray_sampler"])
    return conf


def make_conf(width, sdf_hidden, skip_in, rgb_hidden, light):
    conf = base_conf(width)
    conf["implicit_network"]["dims"] = [width] * sdf_hidden
    conf["implicit_network"]["skip_in"] = list(skip_in)
    conf["rendering_network"]["dims"] = [width] * rgb_hidden
    conf.pop("light_network", None)
    if light is not None:
        conf["light_network"] = {"dims": list(light), "weight_norm": True}
    return conf


def case_conf(case):
    return make_conf(case.width, case.sdf_hidden, case.skip_in, case.rgb_hidden, case.light)


def unchecked_cfg(conf):
    """the NetConfig of a conf whose depth, skip or light head `from_conf` refuses, built behind its back: what a C caller can describe
    to i2sdf_plan_create"""
    import copy
    from i2sdf_amd import config as C
    conf = copy.deepcopy(conf)
    light = conf.pop("light_network", None)
    skip = conf["implicit_network"]["skip_in"]
    conf["implicit_network"]["skip_in"] = []
    saved = C._check_depth
    try:
        C._check_depth = lambda key, dims: None
        cfg = C.NetConfig.from_conf(conf)
    finally:
        C._check_depth = saved
    if skip:
        full = [cfg.sdf.pe_dim] + list(conf["implicit_network"]["dims"]) + [1 + cfg.feature_size]
        cfg.sdf.dims = [(full[l + 1] - full[0] if (l + 1) in skip else full[l + 1], full[l]) for l in range(len(full) - 1)]
        cfg.sdf.skip_layer = skip[0]
    if light is not None:
        lfull = [cfg.feature_size] + list(light["dims"]) + [1]
        cfg.light = C.MlpShape("light_network", [(lfull[l + 1], lfull[l]) for l in range(len(lfull) - 1)], lfull[1], cfg.feature_size, 0)
    return cfg


def case_weights(case):
    ocfg = orc.NetCfg.from_conf(case_conf(case))
    s0, s1 = SEEDS[case.id]
    return ocfg, orc.perturb_params(orc.init_params(ocfg, s0), 0.05, s1)


def case_inputs(case):
    """points, view directions and the weights of the probe loss  sum(sdf sw) + sum(feat fw) + sum((|grad| - 1)^2) + sum(rgb cw) [+ sum(lm lw)]"""
    g = torch.Generator().manual_seed(5)
    F = case.width
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * X_SCALE
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
    sw, fw = torch.randn(M, 1, generator=g), torch.randn(M, F, generator=g) * 0.1
    cw, lw = torch.randn(M, 3, generator=g), torch.randn(M, 1, generator=g)
    m_f = M - M_TAIL
    fw[m_f:] = 0
    cw[m_f:] = 0
    lw[m_f:] = 0
    return {"x": x, "dirs": dirs, "sw": sw, "fw": fw, "cw": cw, "lw": lw, "m_f": m_f}


def oracle_run(case, dtype):
    """Every quantity the GPU tests compare, from the oracle in `dtype`: {"sdf", "feat", "grad", "h_<l>", "abar_<l>", "rgb", ["lm"],
    "grad.<parameter>"}"""
    ocfg, sd = case_weights(case)
    inp = case_inputs(case)
    c = lambda v: v.to(dtype)
    x, m_f = c(inp["x"]), inp["m_f"]
    dirs_pt = c(inp["dirs"]).unsqueeze(1).repeat(1, N_PER_RAY, 1).reshape(-1, 3)
    out = {}
    fwd = orc.sdf_analytic_forward({k: c(v) for k, v in sd.items()}, ocfg.sdf, x)
    for l in range(ocfg.sdf.n_lin - 1):
        out[f"h_{l + 1}"], out[f"abar_{l}"] = orc.softplus100(fwd["a"][l]), fwd["abar"][l]
    params = {k: c(v).requires_grad_(True) for k, v in sd.items() if k != "density.beta"}
    sdf, feat, grad = orc.sdf_outputs(params, ocfg.sdf, x, create_graph=True)
    rgb = orc.rgb_forward(params, ocfg.rgb, dirs_pt, feat)
    loss = (sdf * c(inp["sw"])).sum() + (feat * c(inp["fw"])).sum() + ((grad.norm(2, dim=1) - 1) ** 2).sum() + (rgb * c(inp["cw"])).sum()
    if case.light:
        lm = orc.light_forward(params, ocfg.light, feat[:m_f])
        loss = loss + (lm * c(inp["lw"])[:m_f]).sum()
        out["lm"] = lm.detach().reshape(-1)
    names = list(params)
    grads = torch.autograd.grad(loss, [params[k] for k in names], allow_unused=True)
    out.update({"sdf": sdf.detach(), "feat": feat.detach(), "grad": grad.detach(), "rgb": rgb.detach()})
    out.update({"grad." + k: (g if g is not None else torch.zeros_like(params[k])).detach() for k, g in zip(names, grads)})
    return out


RELU_MARGIN = 2.0 ** -20


def relu_margin(case):
    """the smallest |pre-activation| of a ReLU of the radiance net on the points that carry a colour gradient, relative to its layer's
    largest, in the fp64 oracle.  A unit whose pre-activation is zero within fp32 rounding has its backward mask decided by that rounding:
    one point's contribution to a bias gradient appears or disappears, in the reference's own fp32 run as in any other (helpers.py:
    relu_flip_analysis).  RELU_MARGIN = 2^-20 is sixteen units of fp32 rounding at the layer's scale -- sqrt(K) u for the K = 256 .. 283
    terms of a pre-activation -- so no correct fp32-equivalent evaluation flips a mask on inputs that keep this margin."""
    ocfg, sd = case_weights(case)
    inp = case_inputs(case)
    D = torch.float64
    sd = {k: v.to(D) for k, v in sd.items()}
    rec = {}

    def record(a, l):
        rec[l] = a.detach()
        return torch.relu(a)

    with torch.no_grad(), orc.relu_hook(record):
        feat = orc.sdf_forward(sd, ocfg.sdf, inp["x"].to(D))[:, 1:]
        orc.rgb_forward(sd, ocfg.rgb, inp["dirs"].to(D).unsqueeze(1).repeat(1, N_PER_RAY, 1).reshape(-1, 3), feat)
    return min(float(a[:inp["m_f"]].abs().min() / a[:inp["m_f"]].abs().max()) for a in rec.values())


def bar(name):
    return TOL_GRAD if name.startswith("grad.") else TOL_OUT


def reference(case):
    """the fp64 oracle's run of a case: computed once per session, shared and never written to"""
    from helpers import memo
    return memo(("shape frontier fp64", case.id), lambda: oracle_run(case, torch.float64))


# ---- which weight streams a shape's kernels walk (the selection rule of the launch sites, restated) ---------------------------------
FP32_SPANS = ["sdf.fwd_hidden", "sdf.fwd_sdf", "sdf.fwd_all", "sdf.rev_sweep2", "sdf.rev_chain", "rgb.fwd", "rgb.rev"]


def span_rule(width, sdf_n_lin, skip, rgb_n_lin, light_width):
    """-> (used, absent): the spans the shape's kernels take at a launch site (each must be a whole number of stages) and the spans whose
    being EMPTY is how the library knows that the shape has no such kernel (i2sdf_plan_set_option, sdf_fwd_kind, the light head's launch).
    skip: the skip layer or -1; light_width: the head's hidden width or None.  A span in neither set is a stream the plan emits for the
    shape and no kernel of it walks: the 32-point-wave bf16x3 streams of a 64-wide net beyond its sdf-only forward, and of a 256-wide
    SDF net on the fp32 path (the recorded layouts of tests/golden/plan_layout pin the former)."""
    used, absent = list(FP32_SPANS), []
    if light_width is not None:
        used += ["light.fwd", "light.rev"]
    sdf3h, rgb3h = ["sdf.fwd3h_sdf", "sdf.fwd3h_all", "sdf.fwd2h"], ["rgb.fwd3h", "rgb.rev3h"]
    if width == 256:
        used += sdf3h                                          # sdf-only forward, sampler passes: every depth
        if sdf_n_lin >= 4 and skip != sdf_n_lin - 2:           # training forward, d sdf/dx chain, backward sweeps
            used += ["sdf.fwd3_hidden", "sdf.rev3_sweep2", "sdf.rev3_chain"]
        if rgb_n_lin >= 3:
            used += rgb3h
        else:
            absent += rgb3h
        if light_width is not None:
            (used if light_width == 128 and rgb_n_lin >= 3 else absent if light_width != 128 else []).append("light.fwd3h")
    else:
        used += ["sdf.fwd3_all"]                               # sdf-only forward on 32-point waves
        absent += sdf3h + rgb3h + (["light.fwd3h"] if light_width is not None else [])
    return used, absent
