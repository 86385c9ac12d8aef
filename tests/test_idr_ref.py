"""CPU: the radiance net's 'idr' mode (rendering_network.mode: idr, d_in: 9 -- points and normals as inputs).
tests/idr_ref.py, the plain-torch restatement the GPU tests compare with, against the live reference where it can be imported and against
the numbers the reference recorded (tests/golden/g17_idr_*.npz, tests/golden/gen_golden_idr.py) everywhere, at the bars of
tests/test_oracle_vs_reference.py; and the host side of the mode: the configuration is accepted, the plan builds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import idr_ref
from oracle import i2sdf_oracle as orc
from helpers import assert_close, assert_grad_digest, sd_from_npz, t as tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOSS = orc.LossCfg(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05)


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def _group(z, prefix):
    return {k[len(prefix):]: tensor(z[k]) for k in z.files if k.startswith(prefix)}


def _plumbing_cfg():
    cfg = orc.plumbing_cfg(skip=True)
    cfg.use_normal = True
    return cfg


# ---- idr_ref against the reference's recorded numbers ----------------------------------------------------------------------------
def test_radiance_net_matches_the_recorded_reference():
    z = _load("g17_idr_rgb")
    sd = sd_from_npz(z)
    assert tuple(sd["rendering_network.lin0.weight_v"].shape) == (64, 97)
    rgb, fbar, nbar, grads = idr_ref.rgb_grads(sd, orc.plumbing_cfg().rgb, tensor(z["points"]), tensor(z["normals"]), tensor(z["view_dirs"]),
                                               tensor(z["feat"]), tensor(z["rgb_bar"]))
    assert_close(rgb, tensor(z["rgb"]), 1e-4, "rgb")
    assert_close(fbar, tensor(z["fbar"]), 1e-3, "d/d feature")
    assert_close(nbar, tensor(z["nbar"]), 1e-3, "d/d normals")
    ref = _group(z, "grad.")
    assert set(ref) == set(grads)
    for k, v in ref.items():
        assert_close(grads[k], v, 1e-3, k)
    # the six columns the mode adds carry gradient of their own: a restatement that dropped them would still pass on the other 91
    g0 = ref["rendering_network.lin0.weight_v"]
    assert float(g0[:, :3].abs().max()) > 0 and float(g0[:, 30:33].abs().max()) > 0


def test_eval_forward_matches_the_recorded_reference():
    z = _load("g17_idr_eval")
    out = idr_ref.network_forward(sd_from_npz(z), _plumbing_cfg(), _group(z, "in."), training=False,
                                  z_override=(tensor(z["ref.z_vals"]), tensor(z["ref.z_eik"])))
    ref = _group(z, "out.")
    assert {"rgb_values", "depth_values", "normal_map"} <= set(ref)
    for k, v in ref.items():
        assert_close(out[k], v, 2e-3 if k == "normal_map" else 1e-4, k)
    # and with the oracle's own sampler in front (the depths are not given)
    out = idr_ref.network_forward(sd_from_npz(z), _plumbing_cfg(), _group(z, "in."), training=False)
    assert_close(out["rgb_values"], ref["rgb_values"], 1e-4, "rgb_values, own sampler")


def test_train_step_matches_the_recorded_reference():
    z = _load("g17_idr_train")
    dr = orc.Draws(**_group(z, "draw."))
    out, losses, grads = idr_ref.training_step_grads(sd_from_npz(z), _plumbing_cfg(), _group(z, "in."), _group(z, "gt."), LOSS, dr, step=10)
    for k, v in _group(z, "out.").items():
        assert_close(out[k], v, 2e-3 if k in ("normal_values", "diff_norm") else 1e-4, k)
    assert_close(losses["loss"], tensor(z["loss.loss"]), 1e-5, "loss")
    ref = _group(z, "grad.")
    assert set(ref) == set(grads) and "density.beta" in ref
    for k, v in ref.items():
        assert_close(grads[k], v, 1e-3, k)


def test_train_step_full_size_matches_the_recorded_reference():
    z = _load("g17_idr_train_full")
    cfg = orc.synthetic_cfg(False)
    sd = orc.perturb_params(idr_ref.init_params(cfg, seed=int(z["init_seed"])), float(z["perturb_scale"]), seed=int(z["perturb_seed"]))
    chk = torch.stack([v.double().sum() for v in sd.values()])
    assert torch.allclose(chk[:-1], tensor(z["sd_checksum"])[:-1], rtol=0, atol=1e-9), "rebuilt weights differ from the fixture's"
    sd["density.beta"] = torch.tensor(0.05)
    assert tuple(sd["rendering_network.lin0.weight_v"].shape) == (256, 289)
    dr = orc.Draws(**_group(z, "draw."))
    out, losses, grads = idr_ref.training_step_grads(sd, cfg, _group(z, "in."), _group(z, "gt."), LOSS, dr, step=10,
                                                     z_override=(tensor(z["ref.z_vals"]), tensor(z["ref.z_eik"])))
    for k, v in _group(z, "out.").items():
        assert_close(out[k], v, 2e-3 if k in ("normal_values", "diff_norm") else 1e-4, k)
    assert_close(losses["loss"], tensor(z["loss.loss"]), 1e-5, "loss")
    assert_grad_digest(z, grads, 1e-3)


# ---- idr_ref against the live reference --------------------------------------------------------------------------------------------
def _live_reference():
    sys.path.insert(0, GOLDEN)
    import ref_import
    if not ref_import.available():
        pytest.skip("the reference is not on this machine")
    return ref_import, ref_import.import_reference()[0]


@pytest.mark.parametrize("multires", [4, 0])
def test_radiance_net_matches_the_live_reference(multires):
    _live_reference()
    from model.network.mlp import RenderingNetwork
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(3)
    rnet = RenderingNetwork(64, mode="idr", d_in=9, d_out=3, dims=[64, 64], weight_norm=True, embed_type="positional" if multires else None,
                            multires=multires)
    assert rnet.lin0.weight_v.shape[1] == 9 + 6 * multires + 64
    rcfg = orc.plumbing_cfg().rgb
    rcfg.multires_view = multires
    sd = {"rendering_network." + k: v.detach().clone() for k, v in rnet.state_dict().items()}
    M = 100
    pts, nrm = torch.randn(M, 3, generator=g), torch.randn(M, 3, generator=g)
    view = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    feat, w = torch.randn(M, 64, generator=g), torch.randn(M, 3, generator=g)
    f_, n_ = feat.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
    rgb_ref = rnet(pts, n_, view, f_)
    (rgb_ref * w).sum().backward()
    rgb, fbar, nbar, grads = idr_ref.rgb_grads(sd, rcfg, pts, nrm, view, feat, w)
    assert_close(rgb, rgb_ref, 1e-4, "rgb")
    assert_close(fbar, f_.grad, 1e-3, "d/d feature")
    assert_close(nbar, n_.grad, 1e-3, "d/d normals")
    for n, p in rnet.named_parameters():
        assert_close(grads["rendering_network." + n], p.grad, 1e-3, n)


@pytest.mark.parametrize("multires", [4, 0])
def test_eval_forward_matches_the_live_reference(multires):
    """the whole eval forward, each side with its own sampler (fp32 on both sides: the same arithmetic), on a view from inside the scene"""
    ref_import, ref_model = _live_reference()
    sys.path.insert(0, GOLDEN)
    import gen_golden as G
    cfg = G.small_conf(skip=True)
    cfg.rendering_network.mode, cfg.rendering_network.d_in = "idr", 9
    if multires == 0:
        cfg.rendering_network.embed_type, cfg.rendering_network.multires = "", 0          # (falsy: mlp.py:180; the config node takes no None)
    torch.manual_seed(0)
    full = ref_model.I2SDFNetwork(cfg)
    G.perturb_(full)
    full.eval()
    inp = G.camera_batch(128, (0.1, -0.2, 0.3), train_layout=False)
    ref = full(inp)
    ocfg = _plumbing_cfg()
    ocfg.rgb.multires_view = multires
    out = idr_ref.network_forward({k: v.detach().clone() for k, v in full.state_dict().items()}, ocfg, inp, training=False)
    for k in ("rgb_values", "depth_values", "weight_sum"):
        assert_close(out[k], ref[k], 1e-4, k)
    assert_close(out["normal_map"], ref["normal_map"], 2e-3, "normal_map")


# ---- the host side of the mode -------------------------------------------------------------------------------------------------------
def test_config_accepts_the_idr_switch_and_still_refuses_embed_point():
    from i2sdf_amd.config import NetConfig, plumbing_conf, synthetic_conf
    for conf, in0 in ((synthetic_conf(), 289), (synthetic_conf(True), 289), (plumbing_conf(), 97), (plumbing_conf(True, True), 97)):
        cfg = NetConfig.from_conf(idr_ref.idr_conf(conf))
        assert cfg.rgb_mode == "idr" and cfg.rgb.dims[0][1] == in0 and cfg.rgb.d_in == 9
        assert NetConfig.from_conf(conf).rgb_mode == "nerf" and NetConfig.from_conf(conf).rgb.dims[0][1] == in0 - 6
    for conf, in0 in ((synthetic_conf(), 265), (plumbing_conf(True, True), 73)):          # without the view encoding: 9 in 16
        cfg = NetConfig.from_conf(idr_ref.idr_conf(conf, 0))
        assert cfg.rgb_mode == "idr" and cfg.rgb.dims[0][1] == in0 and cfg.rgb.multires == 0 and cfg.rgb.pe_dim == 9
    assert NetConfig.from_conf(idr_ref.idr_conf(synthetic_conf())).rgb.pe_dim == 33 and NetConfig.from_conf(synthetic_conf()).rgb.pe_dim == 27
    conf = idr_ref.idr_conf(synthetic_conf())
    conf["rendering_network"]["embed_point"] = {"embed_type": "positional", "multires": 6}
    with pytest.raises(NotImplementedError, match="never applies it"):
        NetConfig.from_conf(conf)
    conf = idr_ref.idr_conf(synthetic_conf())
    conf["rendering_network"]["d_in"] = 3
    with pytest.raises(NotImplementedError, match="d_in must be 9"):
        NetConfig.from_conf(conf)
    conf = idr_ref.idr_conf(synthetic_conf())
    conf["rendering_network"]["mode"] = "no_such_mode"
    with pytest.raises(NotImplementedError):
        NetConfig.from_conf(conf)


def test_state_dict_keys_and_shapes_are_the_references():
    from i2sdf_amd import I2SDFNetwork, synthetic_conf
    z = _load("g17_idr_train_full")
    net = I2SDFNetwork(idr_ref.idr_conf(synthetic_conf()))
    sd = net.state_dict()
    assert tuple(sd["rendering_network.lin0.weight_v"].shape) == (256, 289) and net.rendering_network.mode == "idr"
    ref_sd = idr_ref.init_params(orc.synthetic_cfg(False), seed=int(z["init_seed"]))
    assert set(sd) == set(ref_sd) and all(tuple(sd[k].shape) == tuple(ref_sd[k].shape) for k in sd)
    net.load_state_dict(ref_sd)               # a checkpoint of that shape loads


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def _plan(lib, conf):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.params import ParamLayout
    lay = ParamLayout(NetConfig.from_conf(conf))
    desc = lay.net_desc()
    plan = C.c_void_p()
    return lib.load().i2sdf_plan_create(C.byref(desc), C.byref(plan)), plan, lay, desc


def test_plan_builds_for_the_idr_description(lib):
    from i2sdf_amd.config import plumbing_conf, synthetic_conf
    h = lib.load()
    P = C.c_void_p(4096)
    for conf in (synthetic_conf(), synthetic_conf(True), plumbing_conf(), plumbing_conf(True, True)):
        rc0, plan0, lay0, _ = _plan(lib, conf)
        rc, plan, lay, desc = _plan(lib, idr_ref.idr_conf(conf))
        assert rc0 == 0 and rc == 0
        assert desc.rgb.reserved == lib.RGB_MODE_IDR and desc.rgb.d_in == 9 and desc.rgb.in0 == lay0.cfg.rgb.dims[0][1] + 6
        H = lay.cfg.rgb.hidden
        assert lay.n_params == lay0.n_params + 6 * H
        # the streams grew by the wider side block, the weight-gradient block of layer 0 by its 8 padded columns
        assert h.i2sdf_plan_pack_floats(plan) > h.i2sdf_plan_pack_floats(plan0)
        assert h.i2sdf_plan_wgrad_floats(plan) == h.i2sdf_plan_wgrad_floats(plan0) + 8 * H
        # each mode's entry points refuse the other mode's plan (before anything is launched)
        assert h.i2sdf_rgb_forward(plan, P, P, 4, P, 128, 128, P, None, None, None) == -1
        assert h.i2sdf_rgb_backward(plan, P, P, P, P, 128, 128, P, P, P, None) == -1
        assert h.i2sdf_rgb_forward_idr(plan0, P, P, None, P, None, 0, 4, P, P, 128, 128, P, None, None, None) == -1
        assert h.i2sdf_rgb_backward_idr(plan0, P, P, P, P, 128, 128, P, P, P, P, 1, None) == -1
        # argument validation of the new entry points: empty batch, padded rows, neither points nor rays, no nbar
        assert h.i2sdf_rgb_forward_idr(plan, P, P, None, P, None, 0, 4, P, P, 0, 0, P, None, None, None) == 0
        assert h.i2sdf_rgb_forward_idr(plan, P, P, None, P, None, 0, 4, P, P, 100, 100, P, None, None, None) == -1
        assert h.i2sdf_rgb_forward_idr(plan, P, None, None, P, None, 0, 4, P, P, 128, 128, P, None, None, None) == -1
        assert h.i2sdf_rgb_backward_idr(plan, P, P, P, P, 128, 128, P, P, P, None, 1, None) == -1
        h.i2sdf_plan_destroy(plan)
        h.i2sdf_plan_destroy(plan0)
    # without the view encoding: the side block is 9 of 16 columns, 16 fewer padded weight-gradient columns than 'nerf' mode's 32
    for conf in (synthetic_conf(), plumbing_conf(True, True)):
        rc0, plan0, lay0, _ = _plan(lib, conf)
        rc, plan, lay, desc = _plan(lib, idr_ref.idr_conf(conf, 0))
        assert rc0 == 0 and rc == 0 and desc.rgb.multires == 0 and desc.rgb.in0 == 9 + lay.cfg.feature_size
        assert h.i2sdf_plan_wgrad_floats(plan) == h.i2sdf_plan_wgrad_floats(plan0) - 16 * lay.cfg.rgb.hidden
        assert h.i2sdf_rgb_forward_idr(plan, P, P, None, P, None, 0, 4, P, P, 0, 0, P, None, None, None) == 0
        assert h.i2sdf_rgb_forward_idr(plan, P, None, None, P, None, 0, 4, P, P, 128, 128, P, None, None, None) == -1
        h.i2sdf_plan_destroy(plan)
        h.i2sdf_plan_destroy(plan0)
    # a description whose d_in does not agree with the mode is refused
    rc, plan, lay, desc = _plan(lib, idr_ref.idr_conf(plumbing_conf()))
    h.i2sdf_plan_destroy(plan)
    desc.rgb.d_in = 3
    p2 = C.c_void_p()
    assert h.i2sdf_plan_create(C.byref(desc), C.byref(p2)) == -1
    desc.rgb.d_in, desc.rgb.reserved = 9, 2
    assert h.i2sdf_plan_create(C.byref(desc), C.byref(p2)) == -1
