"""CPU: the oracle against the reference at the full synthetic.yml / synthetic_light_mask.yml network shapes, through the
reference's own recorded numbers (tests/golden/g17_*, written by tests/golden/gen_golden.py vsref): its two configs, the
structure of its initialisation, an eval forward and a training step with the random draws it made.  The weights of the
forward / training cases are rebuilt from oracle.init_params(seed) and checked against the fixture's checksums (as G14)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import i2sdf_oracle as orc
from helpers import assert_close, camera_inputs, gaussian_projections, t as tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g17():
    return np.load(os.path.join(GOLDEN, "g17_full_size.npz"), allow_pickle=False)


def _model_conf(cfg_name):
    with open(os.path.join(GOLDEN, "g17_configs.json")) as f:
        conf = json.load(f)[cfg_name]["model"]
    conf["use_normal"] = True
    return conf


def _weights(z, tag, cfg, beta):
    sd = orc.init_params(cfg, seed=int(z[tag + "init_seed"]))
    chk = torch.stack([v.double().sum() for k, v in sd.items() if k != "density.beta"])
    assert torch.allclose(chk, tensor(z[tag + "sd_checksum"]), rtol=0, atol=1e-9), "rebuilt weights differ from the fixture's"
    sd["density.beta"] = torch.tensor(beta)
    return sd


def _group(z, prefix):
    return {k[len(prefix):]: tensor(z[k]) for k in z.files if k.startswith(prefix)}


def test_netcfg_from_conf_matches_literals():
    for name, light in (("synthetic.yml", False), ("synthetic_light_mask.yml", True)):
        assert orc.NetCfg.from_conf(_model_conf(name)) == orc.synthetic_cfg(light)


def test_init_params_same_shapes_and_structure(g17):
    shapes_ref = {k[len("plain.init_shape."):]: tuple(int(d) for d in g17[k]) for k in g17.files if k.startswith("plain.init_shape.")}
    sd = orc.init_params(orc.synthetic_cfg())
    assert set(sd) == set(shapes_ref)
    for k in sd:
        assert tuple(sd[k].shape) == shapes_ref[k], k
    # geometric-init structure (mlp.py:55-69): zero columns and the last-layer mean
    assert torch.count_nonzero(sd["implicit_network.lin0.weight_v"][:, 3:]) == 0
    assert torch.count_nonzero(sd["implicit_network.lin4.weight_v"][:, -36:]) == 0
    assert abs(sd["implicit_network.lin8.weight_v"].mean().item() - float(g17["plain.init.lin8_weight_v_mean"])) < 1e-4
    assert torch.equal(sd["implicit_network.lin8.bias"], tensor(g17["plain.init.lin8_bias"]))


@pytest.mark.parametrize("cfg_name,light,t,beta", [("synthetic.yml", False, (0.1, -0.2, 0.3), 0.1),
                                                   ("synthetic_light_mask.yml", True, (0.0, 0.0, -2.0), 0.02)])
def test_eval_forward_full_size(g17, cfg_name, light, t, beta):
    tag = "eval_" + ("light." if light else "plain.")
    assert float(g17[tag + "beta"]) == np.float32(beta)
    cfg = orc.NetCfg.from_conf(_model_conf(cfg_name))
    sd = _weights(g17, tag, cfg, beta)
    inp = camera_inputs(24, t, train_layout=False)
    rec = _group(g17, tag + "in.")
    assert set(inp) == set(rec) and all(torch.equal(inp[k], rec[k]) for k in inp), "the fixture's rays are not this camera's"
    ref = _group(g17, tag + "out.")
    out = orc.network_forward(sd, cfg, inp, training=False)
    for k, v in ref.items():
        assert_close(out[k], v, 2e-3 if k == "normal_map" else 1e-4, k)


def test_train_step_full_size_with_captured_draws(g17):
    conf = _model_conf("synthetic.yml")
    cfg = orc.NetCfg.from_conf(conf)
    sd = _weights(g17, "train.", cfg, 0.05)
    inp, gt, ref = _group(g17, "train.in."), _group(g17, "train.gt."), _group(g17, "train.out.")
    dr = orc.Draws(**_group(g17, "train.draw."))
    lc = orc.LossCfg(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, depth_weight=0.1, normal_weight=0.05, bubble_weight=0.5)
    out, losses, grads = orc.training_step_grads(sd, cfg, inp, gt, lc, dr, step=10)
    for k, v in ref.items():
        assert_close(out[k], v, 2e-3 if k in ("normal_values", "diff_norm") else 1e-4, k)
    assert_close(losses["loss"], tensor(g17["train.loss.loss"]), 1e-5, "loss")
    # gradients, max-norm relative error <= 1e-3 per tensor.  Tensors of <= 1024 elements are stored whole.  Of a larger one the
    # fixture holds max |g_ref| and N_PROJ seeded Gaussian projections R g_ref: with e = g - g_ref, mean((R e)^2) estimates |e|_2^2,
    # and the test requires that estimate to be <= (0.7 * 1e-3 * max |g_ref|)^2.  |e|_inf <= |e|_2, so a pass implies the 1e-3
    # max-norm bound unless the projections underestimate |e|_2^2 by more than 1 / 0.49 (chi-square, 256 degrees of freedom: < 1e-9
    # for any fixed e) -- and |e|_2 <= bound is itself the stricter condition.
    tol = 1e-3
    names = {k.split(".", 2)[2] for k in g17.files if k.startswith(("train.grad.", "train.gproj."))}
    assert names and names <= set(grads)
    for n in sorted(names):
        g = torch.as_tensor(grads[n]).detach()
        if "train.grad." + n in g17.files:
            assert_close(g, tensor(g17["train.grad." + n]), tol, n)
            continue
        assert tuple(g.shape) == tuple(int(d) for d in g17["train.gshape." + n]) and torch.isfinite(g).all(), n
        gmax = float(g17["train.gmax." + n])
        d = gaussian_projections(g, n) - g17["train.gproj." + n]
        l2 = float(np.sqrt(np.mean(d ** 2)))
        assert l2 <= 0.7 * tol * gmax, f"{n}: 2-norm of the difference ~{l2 / gmax:.3e} of max |g_ref| > {0.7 * tol:.1e}"
