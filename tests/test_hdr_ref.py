"""CPU: the radiance net's output activations (rendering_network.output_activation: sigmoid / relu / softplus) and the HDR tone map.
tests/hdr_ref.py, the plain-torch restatement the GPU tests compare with, against the live reference where it can be imported and against
the numbers the reference recorded (tests/golden/g21_hdr_*.npz, tests/golden/gen_golden_hdr.py) everywhere, at the bars of
tests/test_idr_ref.py; and the host side: the configuration is parsed, the descriptor carries the activation, the plan refuses an unknown
one, the tone-map entry point is declared, exported and bound."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import hdr_ref
from oracle import i2sdf_oracle as orc
from helpers import assert_close, sd_from_npz, t as tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(m, a) for m in ("nerf", "idr") for a in ("relu", "softplus")]


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def _grads(sd, rcfg, act, mode, view, feat, pts, nrm, w):
    names = [k for k in sd if k.startswith("rendering_network.")]
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    f = feat.detach().clone().requires_grad_(True)
    n = nrm.detach().clone().requires_grad_(True) if mode == "idr" else None
    rgb = hdr_ref.rgb_forward(p, rcfg, act, view, f, pts if mode == "idr" else None, n)
    g = torch.autograd.grad(rgb, [f] + ([n] if n is not None else []) + [p[k] for k in names], w)
    k0 = 2 if n is not None else 1
    return rgb.detach(), g[0], (g[1] if n is not None else None), dict(zip(names, g[k0:]))


# ---- hdr_ref against the reference's recorded numbers ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,act", CASES)
def test_radiance_net_matches_the_recorded_reference(mode, act):
    z = _load(f"g21_hdr_{mode}_{act}")
    assert os.path.getsize(os.path.join(GOLDEN, f"g21_hdr_{mode}_{act}.npz")) < os.path.getsize(os.path.join(GOLDEN, "g17_idr_train_full.npz"))
    sd = sd_from_npz(z)
    assert tuple(sd["rendering_network.lin0.weight_v"].shape) == (64, 97 if mode == "idr" else 91)
    idr = mode == "idr"
    rgb, fbar, nbar, grads = _grads(sd, orc.plumbing_cfg().rgb, act, mode, tensor(z["view_dirs"]), tensor(z["feat"]),
                                    tensor(z["points"]) if idr else None, tensor(z["normals"]) if idr else None, tensor(z["rgb_bar"]))
    ref_rgb = tensor(z["rgb"])
    # the fixture exercises what the activation adds: radiance above 1, softplus's linear branch, relu's zero branch
    assert float(ref_rgb.max()) > 20.0 and float((ref_rgb > 1).float().mean()) > 0.02
    if act == "relu":
        assert float((ref_rgb == 0).float().mean()) > 0.1
    else:
        assert float(ref_rgb.min()) > 0.0
    assert_close(rgb, ref_rgb, 1e-4, "rgb")
    assert_close(fbar, tensor(z["fbar"]), 1e-3, "d/d feature")
    if idr:
        assert_close(nbar, tensor(z["nbar"]), 1e-3, "d/d normals")
    ref = {k[len("grad."):]: tensor(z[k]) for k in z.files if k.startswith("grad.")}
    assert set(ref) == set(grads)
    for k, v in ref.items():
        assert_close(grads[k], v, 1e-3, k)
    # the sigmoid restatement is the oracle's, bit for bit
    if not idr:
        assert torch.equal(hdr_ref.rgb_forward(sd, orc.plumbing_cfg().rgb, "sigmoid", tensor(z["view_dirs"]), tensor(z["feat"])),
                           orc.rgb_forward(sd, orc.plumbing_cfg().rgb, tensor(z["view_dirs"]), tensor(z["feat"])))


def test_tone_map_matches_the_recorded_reference():
    z = _load("g21_hdr_tonemap")
    x = tensor(z["x"])
    ns, no = int(z["n_special"]), int(z["n_outside"])
    thr = np.float32(0.0031308)
    for v in (0.0, float(thr), float(np.nextafter(thr, np.float32(0))), float(np.nextafter(thr, np.float32(1))), 1.0):
        assert bool((x[:ns] == v).any()), v
    assert bool((x[ns:ns + no] < 0).any()) and bool((x[ns:ns + no] > 1).any())
    for key, clamp, dt in (("srgb", False, torch.float32), ("srgb_clamped", True, torch.float32), ("srgb64", False, torch.float64),
                           ("srgb64_clamped", True, torch.float64)):
        got = hdr_ref.linear_to_srgb(x.to(dt), clamp)
        assert got.dtype == dt
        assert torch.equal(got, tensor(z[key])), key          # the same elementwise torch expression: the same bits
    c = hdr_ref.linear_to_srgb(x.double(), True)
    assert float(c.min()) == 0.0 and abs(float(c.max()) - 1.0) < 1e-15 and bool((c[x >= 1] == c[x == 1][0]).all())


# ---- hdr_ref against the live reference ----------------------------------------------------------------------------------------------
def _live_reference():
    sys.path.insert(0, GOLDEN)
    import ref_import
    if not ref_import.available():
        pytest.skip("the reference is not on this machine")
    return ref_import, ref_import.import_reference()[0]


@pytest.mark.parametrize("mode", ["nerf", "idr"])
@pytest.mark.parametrize("act", ["sigmoid", "relu", "softplus"])
def test_radiance_net_matches_the_live_reference(mode, act):
    _live_reference()
    from model.network.mlp import RenderingNetwork
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(3)
    rnet = RenderingNetwork(64, mode=mode, d_in=9 if mode == "idr" else 3, d_out=3, dims=[64, 64], weight_norm=True, embed_type="positional",
                            multires=4, output_activation=act)
    with torch.no_grad():
        rnet.lin2.weight_g.mul_(300.0)
    sd = {"rendering_network." + k: v.detach().clone() for k, v in rnet.state_dict().items()}
    M = 100
    pts, nrm = torch.randn(M, 3, generator=g), torch.randn(M, 3, generator=g)
    view = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    feat, w = torch.randn(M, 64, generator=g), torch.randn(M, 3, generator=g)
    f_, n_ = feat.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
    rgb_ref = rnet(pts, n_, view, f_)
    (rgb_ref * w).sum().backward()
    rgb, fbar, nbar, grads = _grads(sd, orc.plumbing_cfg().rgb, act, mode, view, feat, pts, nrm, w)
    if act != "sigmoid":
        assert float(rgb_ref.max()) > 20.0
    assert_close(rgb, rgb_ref, 1e-4, "rgb")
    assert_close(fbar, f_.grad, 1e-3, "d/d feature")
    if mode == "idr":
        assert_close(nbar, n_.grad, 1e-3, "d/d normals")
    for n, p in rnet.named_parameters():
        assert_close(grads["rendering_network." + n], p.grad, 1e-3, n)


def test_tone_map_matches_the_live_reference():
    _live_reference()
    rend_util = importlib.import_module("utils.rend_util")
    x = torch.rand(4096, generator=torch.Generator().manual_seed(1)) * 9.5 - 0.5
    assert torch.equal(hdr_ref.linear_to_srgb(x, True), rend_util.linear_to_srgb(x.clamp(0, 1)))
    assert torch.equal(hdr_ref.linear_to_srgb(x.double(), False), rend_util.linear_to_srgb(x.double()))


@pytest.mark.parametrize("mode,act", CASES)
def test_network_forward_and_step_reduce_to_the_oracles_with_a_sigmoid(mode, act):
    """hdr_ref.network_forward / training_step_grads are the oracle's ('nerf') and idr_ref's ('idr') around another last line: with
    'sigmoid' they give the same bits, with `act` another render."""
    import idr_ref
    from helpers import camera_inputs, make_draws, make_gt
    cfg = orc.plumbing_cfg(False)
    cfg.use_normal = True
    sd = orc.perturb_params(hdr_ref.init_params(cfg, mode, seed=3), 0.03, seed=4)
    B = 8
    inp, gt, dr = camera_inputs(B, (0.0, 0.0, -2.0), seed=5), make_gt(B), make_draws(cfg, B, n_row=cfg.sampler.N_samples_eval, seed=2)
    lc = orc.LossCfg()
    cam, dirs, _ = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
    zo = orc.sample_z_vals(sd, cfg, dirs, cam, training=True, draws=dr, force_iters=1)
    base = (idr_ref.training_step_grads(sd, cfg, inp, gt, lc, dr, 0, z_override=zo) if mode == "idr"
            else orc.training_step_grads(sd, cfg, inp, gt, lc, dr, 0, z_override=zo))
    same = hdr_ref.training_step_grads(sd, cfg, "sigmoid", mode, inp, gt, lc, dr, 0, z_override=zo)
    assert torch.equal(same[1]["loss"], base[1]["loss"]) and all(torch.equal(same[2][k], base[2][k]) for k in base[2])
    other = hdr_ref.training_step_grads(sd, cfg, act, mode, inp, gt, lc, dr, 0, z_override=zo)
    assert not torch.equal(other[0]["rgb_values"], base[0]["rgb_values"])
    assert torch.equal(other[0]["depth_values"], base[0]["depth_values"])


# ---- the host side -------------------------------------------------------------------------------------------------------------------
def test_config_reads_the_output_activation():
    from i2sdf_amd import I2SDFNetwork
    from i2sdf_amd.config import NetConfig, plumbing_conf, synthetic_conf
    from i2sdf_amd.params import ParamLayout
    from i2sdf_amd import lib as L
    for base in (synthetic_conf(), plumbing_conf(True, True)):
        for mode in ("nerf", "idr"):
            assert NetConfig.from_conf(hdr_ref.hdr_conf(base, None, mode)).rgb_act == "sigmoid"          # absent
            conf = hdr_ref.hdr_conf(base, None, mode)
            conf["rendering_network"]["output_activation"] = None
            assert NetConfig.from_conf(conf).rgb_act == "sigmoid"                                        # None
            n0 = ParamLayout(NetConfig.from_conf(hdr_ref.hdr_conf(base, None, mode))).n_params
            for code, act in enumerate(("sigmoid", "relu", "softplus")):
                cfg = NetConfig.from_conf(hdr_ref.hdr_conf(base, act, mode))
                assert cfg.rgb_act == act and cfg.rgb_mode == mode
                lay = ParamLayout(cfg)
                desc = lay.net_desc()
                assert desc.rgb.reserved == (1 if mode == "idr" else 0) | code << 8 and L.RGB_ACTS[act] == code
                assert lay.n_params == n0 and desc.sdf.reserved == 0
    conf = hdr_ref.hdr_conf(synthetic_conf(), "tanh")
    with pytest.raises((NotImplementedError, ValueError), match="output_activation must be one of 'sigmoid', 'relu', 'softplus'"):
        NetConfig.from_conf(conf)
    conf = synthetic_conf()
    conf["implicit_network"]["output_activation"] = "sigmoid"
    with pytest.raises((NotImplementedError, ValueError), match=r"implicit_network.output_activation.*\[sdf \| feature\]"):
        NetConfig.from_conf(conf)
    conf["implicit_network"]["output_activation"] = None
    assert NetConfig.from_conf(conf).rgb_act == "sigmoid"
    # the module: the activation is an attribute, the state_dict's keys and shapes do not change
    a, b = I2SDFNetwork(plumbing_conf()), I2SDFNetwork(hdr_ref.hdr_conf(plumbing_conf(), "relu"))
    assert a.rendering_network.output_activation == "sigmoid" and b.rendering_network.output_activation == "relu"
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)
    b.load_state_dict(sa)


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_tone_map_entry_point_is_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    assert re.search(r"int\s+i2sdf_linear_to_srgb\(const float\* src, float\* dst, int64_t n, int32_t clamp01, void\* stream\);", header)
    for name, val in (("SIGMOID", 0), ("RELU", 1), ("SOFTPLUS", 2)):
        assert re.search(rf"#define I2SDF_RGB_ACT_{name} {val}\b", header)
    assert "i2sdf_linear_to_srgb" in lib.SIGNATURES
    raw = C.CDLL(lib.LIB_PATH)
    assert getattr(raw, "i2sdf_linear_to_srgb") is not None
    h = lib.load()
    P = C.c_void_p(4096)
    # host-side validation, nothing launched: empty input, negative length, missing pointers
    assert h.i2sdf_linear_to_srgb(None, None, 0, 1, None) == 0
    assert h.i2sdf_linear_to_srgb(P, P, -1, 1, None) == -1
    assert h.i2sdf_linear_to_srgb(None, P, 8, 1, None) == -1 and h.i2sdf_linear_to_srgb(P, None, 8, 0, None) == -1
    import i2sdf_amd
    from i2sdf_amd import views
    assert i2sdf_amd.linear_to_srgb is views.linear_to_srgb
    with pytest.raises(ValueError, match="no CPU path"):
        views.linear_to_srgb(torch.zeros(4))
    for fn in (views.image_metrics, views.psnr, views.ssim):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(torch.zeros(121, 3), torch.zeros(121, 3), (11, 11), hdr=True)
    with pytest.raises(ValueError, match="no CPU path"):
        views.to_frames(rgb=torch.zeros(121, 3), img_res=(11, 11), hdr=True)


def test_plan_create_refuses_an_unknown_activation(lib):
    from i2sdf_amd.config import NetConfig, plumbing_conf, synthetic_conf
    from i2sdf_amd.params import ParamLayout
    h = lib.load()
    for base in (plumbing_conf(), synthetic_conf()):
        for mode in ("nerf", "idr"):
            floats = None
            for act in ("sigmoid", "relu", "softplus"):
                desc = ParamLayout(NetConfig.from_conf(hdr_ref.hdr_conf(base, act, mode))).net_desc()
                plan = C.c_void_p()
                assert h.i2sdf_plan_create(C.byref(desc), C.byref(plan)) == 0, (mode, act)
                # the streams and the weight-gradient blocks do not depend on the activation
                sizes = (h.i2sdf_plan_pack_floats(plan), h.i2sdf_plan_wgrad_floats(plan))
                floats = floats or sizes
                assert sizes == floats
                h.i2sdf_plan_destroy(plan)
            desc = ParamLayout(NetConfig.from_conf(hdr_ref.hdr_conf(base, "relu", mode))).net_desc()
            mode_bits = desc.rgb.reserved & 0xff
            for bad in (mode_bits | 3 << 8, mode_bits | 255 << 8, mode_bits | 1 << 16, mode_bits | 1 << 8 | 1 << 20):
                desc.rgb.reserved = bad
                plan = C.c_void_p()
                assert h.i2sdf_plan_create(C.byref(desc), C.byref(plan)) == -1, bad
                msg = h.i2sdf_last_hip_error().decode()
                assert "output activation" in msg and "I2SDF_RGB_ACT_SOFTPLUS" in msg, msg
            desc.rgb.reserved = 2                      # an unknown MODE stays refused (bits 0..7)
            plan = C.c_void_p()
            assert h.i2sdf_plan_create(C.byref(desc), C.byref(plan)) == -1


def test_softplus_derivative_from_the_saved_output():
    """The backward kernels recover d softplus / d o from the saved y = softplus(o): -expm1(-y) = sigmoid(o) exactly; for o > 20
    (nn.Softplus's threshold) y = o and the derivative is 1.  fp64 closed forms over o in [-80, 20], then the fp32 evaluation the kernels
    use, whose error must stay relative (1 - exp(-y) would lose every digit where y is tiny)."""
    o = torch.cat([torch.linspace(-80.0, 20.0, 20001, dtype=torch.float64), torch.tensor([-1e-3, 0.0, 1e-3, 19.999, 20.0], dtype=torch.float64)])
    y = torch.nn.functional.softplus(o)
    sig = torch.sigmoid(o)
    d = -torch.expm1(-y)
    assert float(((d - sig).abs() / sig).max()) < 1e-14
    # autograd's own derivative of nn.Softplus on both sides of the threshold
    oo = torch.tensor([-30.0, -1.0, 0.0, 5.0, 19.5, 20.0, 20.5, 25.0, 60.0], dtype=torch.float64, requires_grad=True)
    yy = torch.nn.Softplus()(oo)
    g, = torch.autograd.grad(yy.sum(), oo)
    rule = torch.where(yy.detach() > 20, torch.ones_like(yy), -torch.expm1(-yy.detach()))
    assert bool((yy.detach()[oo.detach() > 20] == oo.detach()[oo > 20]).all()) and bool((rule[oo.detach() > 20] == 1).all())
    assert float(((rule - g).abs() / g).max()) < 1e-8          # (at o in (20, ~37) torch's own derivative is 1 where sigmoid(o) is 1 - 2e-9)
    # fp32: y <= 20 whenever o <= 20, and the rule from the fp32 y keeps a relative accuracy of a few ulps down to o = -80
    o32 = o.float()
    y32 = torch.where(o32 > 20, o32, torch.log1p(torch.exp(o32)))
    assert bool((y32[o32 <= 20] <= 20).all())
    d32 = torch.where(y32 > 20, torch.ones_like(y32), -torch.expm1(-y32))
    rel = ((d32.double() - torch.sigmoid(o32.double())).abs() / torch.sigmoid(o32.double())).max()
    assert float(rel) < 1e-6, float(rel)
    naive = 1.0 - torch.exp(-y32)
    assert float(((naive.double() - torch.sigmoid(o32.double())).abs() / torch.sigmoid(o32.double())).max()) > 0.5
