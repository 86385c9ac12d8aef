"""GPU: the radiance net's output activations (rendering_network.output_activation: relu, softplus; sigmoid stays the default) in both
kernel families, both modes, forward and backward, against tests/hdr_ref.py in fp64 (itself held to the reference by
tests/test_hdr_ref.py); and the HDR half of the validation views (views.linear_to_srgb, the `hdr` arguments).  Both weight-gradient modes
(I2SDF_WGRAD_BF16X2, set here: tests/conftest.py lists the dual-mode modules by name).  Sizes are those of tests/test_gpu_idr.py."""
import math
import os

import numpy as np
import pytest
import torch

import hdr_ref
import idr_ref
import views_ref as VR
from oracle import i2sdf_oracle as orc
from helpers import assert_close, camera_inputs, make_draws, make_gt, memo, rel_max, sd_from_npz, t

pytestmark = pytest.mark.gpu
TOL = 2e-5                   # the bar of the existing forward tests (tests/test_gpu_train_forward.py, tests/test_gpu_idr.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WGRAD_MODES = ["wgrad-bf16x2", "wgrad-bf16x3"]
ACTS = ["relu", "softplus"]
MODES = ["nerf", "idr"]
CASES = {"plumbing": (lambda: orc.plumbing_cfg(False), {}), "synthetic": (lambda: orc.synthetic_cfg(False), {}),
         "synthetic_fp32": (lambda: orc.synthetic_cfg(False), {"bf16x3": False})}
# ("plumbing", 30, 10): 64 wide, fp32 MFMA, one partial workgroup behind two full ones; ("synthetic", 300, 7): 256 wide, 16-point waves, sixteen
# full workgroups and a partial one; parts = 4: the point ranges of I2SDF_OPT_PARTS; ("synthetic", 4750, 7, parts 0), 'nerf' only: more than one
# round of 256 workgroups with a partial last one, which the split-K tail kernels take
SIZES = [("plumbing", 30, 10, None), ("synthetic", 300, 7, None), ("synthetic", 300, 7, 4), ("synthetic_fp32", 300, 7, None)]
TAIL = ("synthetic", 4750, 7, 0)


def _conf(which, act, mode, **extra):
    from i2sdf_amd.config import plumbing_conf, synthetic_conf
    conf = hdr_ref.hdr_conf(plumbing_conf(False) if which.startswith("plumbing") else synthetic_conf(False), act, mode)
    conf.update(CASES[which][1])
    conf.update(extra)
    return conf


def _engine(conf, sd, parts=None):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.engine import RenderEngine
    eng = RenderEngine(NetConfig.from_conf(conf))
    if parts is not None:
        eng.set_parts(parts)
        assert eng.parts == (parts if parts >= 2 else 0) and eng.blocked_saves
    eng.pack(eng.layout.flat_from_state_dict(sd).cuda())
    return eng


def _weights(ocfg, mode, seed, out_gain=1.0, scale=0.05):
    """out_gain: the last layer's weight_g times this -- freshly initialised, the net's outputs stay within +-0.1 of zero, where nothing of
    an HDR activation shows (and where an output relu sits on its kink); with a gain of 20 they reach past 1"""
    sd = orc.perturb_params(hdr_ref.init_params(ocfg, mode, seed=seed), scale, seed=seed + 1)
    last = f"rendering_network.lin{ocfg.rgb.n_lin - 1}.weight_g"
    sd[last] = sd[last] * out_gain
    return sd


def dbl(sd):
    return {k: v.double() for k, v in sd.items()}


def _assert_tail_cut(eng, M, Mp):
    """the split-K tail kernels ran: the blocked prefix of the saved radiance tensors (the points of the full workgroups) ends at a whole
    number of rounds of 256 workgroups, in front of the batch's end"""
    bulk = eng.blocked_points(1, M, Mp)
    assert 0 < bulk < M and bulk % (256 * 128) == 0 and M - bulk < 256 * 128, (bulk, M, Mp)
    return bulk


@pytest.fixture
def wgrad(request, monkeypatch):
    monkeypatch.setenv("I2SDF_WGRAD_BF16X2", "1" if request.param == "wgrad-bf16x2" else "0")
    return request.param


# ---- 1. radiance forward ---------------------------------------------------------------------------------------------------------------
def _fwd_case(which, B, n, act, mode):
    """inputs and the fp64 reference, computed once per (size, activation, mode).  The features are scaled (by the smallest power of 4 that
    does it, decided on the reference's pre-activations alone) until outputs exceed 1 and one pre-activation exceeds 20, softplus's threshold."""
    def make():
        ocfg = CASES[which][0]()
        sd = _weights(ocfg, mode, 51)
        g = torch.Generator().manual_seed(2)
        M, F = B * n, ocfg.rgb.feature_size
        cam = torch.randn(B, 3, generator=g) * 0.3
        dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
        z = torch.cat([torch.sort(torch.rand(B, n, generator=g) * 3.0, -1)[0], torch.full((B, 1), 4.0)], 1)
        pts = (cam.unsqueeze(1) + z[:, :n].unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
        nrm = torch.randn(M, 3, generator=g) * 0.8
        feat0 = torch.randn(M, F, generator=g) * 0.5
        dflat = dirs.unsqueeze(1).repeat(1, n, 1).reshape(-1, 3)
        idr = mode == "idr"
        for s in (1.0, 4.0, 16.0, 64.0, 256.0, 1024.0, 4096.0, 16384.0):
            feat = feat0 * s
            pre = hdr_ref.rgb_forward(dbl(sd), ocfg.rgb, act, dflat.double(), feat.double(), pts.double() if idr else None,
                                      nrm.double() if idr else None, return_pre=True)
            if float(pre.max()) > 20.5 and float((pre > 1).double().mean()) > 0.02:
                break
        ref = hdr_ref.rgb_forward(dbl(sd), ocfg.rgb, act, dflat.double(), feat.double(), pts.double() if idr else None, nrm.double() if idr else None)
        return ocfg, sd, cam, dirs, z, pts, nrm, feat, pre, ref
    return memo(("hdr fwd", which, B, n, act, mode), make)


# (the tail size in 'nerf' mode only: 'idr' mode has no split-K tail, tests/test_gpu_idr.py runs that size through full workgroups)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("which,B,n,parts,mode", [s + (m,) for s in SIZES for m in MODES] + [TAIL + ("nerf",)])
def test_rgb_forward(which, B, n, parts, mode, act):
    ocfg, sd, cam, dirs, z, pts, nrm, feat, pre, ref = _fwd_case(which, B, n, act, mode)
    M, F = B * n, ocfg.rgb.feature_size
    # radiance above 1 is there, and so is softplus's linear branch (o > 20) / relu's zero branch
    assert float(ref.max()) > 1.0 and float((ref > 1).double().mean()) > 0.02 and float(pre.max()) > 20.0
    assert float((pre < 0).double().mean()) > 0.02
    eng = _engine(_conf(which, act, mode), sd, parts)
    assert eng.rgb_act == act and eng.idr == (mode == "idr")
    Mp = eng.pad_rows(M)
    featp = torch.zeros(Mp, F)
    featp[:M] = feat
    if mode == "idr":
        rgb, rs, pev = eng.rgb_forward(dirs.cuda(), n, featp.cuda(), M, points=pts.cuda(), normals=nrm.cuda())
    else:
        rgb, rs, pev = eng.rgb_forward(dirs.cuda(), n, featp.cuda(), M)
    err = assert_close(rgb.cpu(), ref, TOL, f"rgb ({act}, {mode})")
    print(f"{which} {B}x{n} parts={parts} {act} {mode}: rgb max {float(ref.max()):.1f}, max-norm relative error {err:.2e}")
    if act == "relu":
        # where the reference's pre-activation is negative beyond rounding the output is exactly 0
        assert bool((rgb.cpu()[pre < -1e-4 * float(pre.abs().max())] == 0).all())
    else:
        big = pre > 20.5
        assert bool(big.any()) and float((rgb.cpu().double()[big] - pre[big]).abs().max()) <= TOL * float(ref.max())
        assert float(rgb.min()) > 0.0
    if (which, B, n, parts) == TAIL:
        bulk = _assert_tail_cut(eng, M, Mp)
        assert_close(rgb.cpu()[bulk:], ref[bulk:], TOL, "rgb of the split-K tail")
        assert float(pre[bulk:].max()) > 1.0 and float(pre[bulk:].min()) < 0.0


# ---- 2. radiance backward ----------------------------------------------------------------------------------------------------------------
KINK = 1e-4                  # |o| below this in the fp64 reference: the output relu's derivative is decided by rounding, the point is given no weight


def _bwd_case(which, B, n, act, mode, idx=None):
    """probe loss sum(rgb * cw) with the SDF net in front, fp64; `idx`: the points the loss weights (all of them when None).  For relu, cw is
    zeroed where the reference's |o| < KINK -- decided here, from the reference alone, before anything is launched."""
    def make():
        ocfg = CASES[which][0]()
        sd = _weights(ocfg, mode, 13, out_gain=20.0)
        g = torch.Generator().manual_seed(6)
        M = B * n
        x = (torch.rand(M, 3, generator=g) * 2 - 1)
        dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
        cw = torch.randn(M, 3, generator=g)
        sel = torch.arange(M) if idx is None else idx
        keep = torch.zeros(M, 1)
        keep[sel] = 1
        cw = cw * keep
        idr = mode == "idr"
        params = {k: v.double().requires_grad_(True) for k, v in sd.items() if not k.startswith("light") and k != "density.beta"}
        dflat = dirs.double()[sel // n]
        if idr:
            sdf, feat, grad = orc.sdf_outputs(params, ocfg.sdf, x.double()[sel], create_graph=True)
        else:
            feat, grad = orc.sdf_forward(params, ocfg.sdf, x.double()[sel])[:, 1:], None
        pre = hdr_ref.rgb_forward(params, ocfg.rgb, act, dflat, feat, x.double()[sel] if idr else None, grad, return_pre=True)
        rgb = torch.relu(pre) if act == "relu" else torch.nn.functional.softplus(pre)
        zeroed = 0.0
        if act == "relu":
            kink = pre.detach().abs() < KINK
            zeroed = float(kink.double().mean())
            cw[sel] = cw[sel] * (~kink).float()
        loss = (rgb * cw.double()[sel]).sum()
        names = list(params)
        gr = torch.autograd.grad(loss, [feat] + ([grad] if idr else []) + [params[k] for k in names], allow_unused=True)
        k0 = 2 if idr else 1
        ref = {k: (v if v is not None else torch.zeros_like(params[k])) for k, v in zip(names, gr[k0:])}
        return ocfg, sd, x, dirs, cw, rgb.detach(), pre.detach(), gr[0], (gr[1] if idr else None), ref, zeroed
    return memo(("hdr bwd", which, B, n, act, mode, None if idx is None else int(idx.sum())), make)


def _run_backward(eng, flat, x, dirs, n, cw, M, idr):
    fwd = eng.sdf_forward_grad(points=x.cuda())
    if idr:
        rgb_h, rs, pev = eng.rgb_forward(dirs.cuda(), n, fwd["feat"], M, points=x.cuda(), normals=fwd["grad"])
        nbar = torch.full((M, 3), float("nan"), device="cuda")                      # written, not added to
        gar, ga_last, fbar = eng.rgb_backward(rgb_h, cw.cuda(), rs, M, nbar=nbar, accumulate=False)
    else:
        rgb_h, rs, pev = eng.rgb_forward(dirs.cuda(), n, fwd["feat"], M)
        nbar = None
        gar, ga_last, fbar = eng.rgb_backward(rgb_h, cw.cuda(), rs, M)
    bw = eng.sdf_backward(fwd, sbar=None, fbar=fbar, m_fbar=M, nbar=nbar)
    gflat = torch.zeros_like(flat)
    eng.weight_grads(flat, gflat, fwd, bw, M_main=M, fbar=fbar, rgb_fw={"pev": pev, "rs": rs}, rgb_bw={"gar": gar, "ga_last": ga_last})
    return rgb_h, fbar, nbar, ga_last, eng.layout.state_dict_from_flat(gflat.cpu())


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("which,B,n,parts", SIZES)
def test_rgb_backward_param_feature_and_normal_grads(which, B, n, parts, act, mode, wgrad):
    """probe loss = sum(rgb * cw) with the SDF net in front, as tests/test_gpu_idr.py has it: fbar, nbar ('idr') and every parameter gradient
    at 1e-4.  relu: the derivative is undefined at the kink; cw is zero where the fp64 reference has |o| < 1e-4 (at most 0.5 % of the outputs)."""
    ocfg, sd, x, dirs, cw, rgb_ref, pre, fbar_ref, nbar_ref, ref, zeroed = _bwd_case(which, B, n, act, mode)
    print(f"{which} {act} {mode}: {zeroed * 100:.3f} % of the outputs lie within {KINK} of the kink and carry no weight")
    assert zeroed <= 0.005
    M = B * n
    eng = _engine(_conf(which, act, mode), sd, parts)
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    rgb_h, fbar, nbar, ga_last, got = _run_backward(eng, flat, x, dirs, n, cw, M, mode == "idr")
    assert_close(rgb_h.cpu(), rgb_ref, TOL, "rgb")
    # G(a_last) = cw * dy/do, by the rule the header states, from the reference's o
    d = (pre > 0).double() if act == "relu" else torch.sigmoid(pre)
    assert_close(ga_last[:M, :3].cpu(), cw.double() * d, 1e-4, "G(a_last)")
    assert float(ga_last[:M, 3].abs().max()) == 0.0
    assert_close(fbar[:M].cpu(), fbar_ref, 1e-4, "fbar")
    if mode == "idr":
        assert_close(nbar.cpu(), nbar_ref, 1e-4, "nbar_rgb")
    for k in ref:
        assert_close(got[k], ref[k], 1e-4, k)
    assert float(ref["rendering_network.lin0.weight_v"].abs().max()) > 0 and float(ref["implicit_network.lin0.weight_v"].abs().max()) > 0


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("act", ACTS)
def test_rgb_backward_split_k_tail(act, wgrad):
    """('synthetic', 4750, 7, parts 0), 'nerf': 256 full workgroups and a tail of 482 points that rgb_bwd_split_kernel takes.  The probe loss
    weights the tail and a few bulk points, so the oracle differentiates just those (tests/test_gpu_backward.py: test_backward_split_k_tail)."""
    which, B, n, parts = TAIL
    M = B * n
    idx = torch.cat([torch.arange(0, 150), torch.arange(256 * 128 - 90, M)])
    ocfg, sd, x, dirs, cw, rgb_ref, pre, fbar_ref, _, ref, zeroed = _bwd_case(which, B, n, act, "nerf", idx)
    assert zeroed <= 0.005
    eng = _engine(_conf(which, act, "nerf"), sd, parts)
    bulk = _assert_tail_cut(eng, M, eng.pad_rows(M))
    assert bulk == 256 * 128 and int((idx >= bulk).sum()) == M - bulk and float(cw[bulk:].abs().max()) > 0
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    rgb_h, fbar, _, ga_last, got = _run_backward(eng, flat, x, dirs, n, cw, M, False)
    assert_close(rgb_h.cpu()[idx], rgb_ref, TOL, "rgb")
    d = (pre > 0).double() if act == "relu" else torch.sigmoid(pre)
    assert_close(ga_last[:M, :3].cpu()[idx], cw.double()[idx] * d, 1e-4, "G(a_last)")
    assert_close(fbar[:M].cpu()[idx], fbar_ref, 1e-4, "fbar")
    assert_close(fbar[bulk:M].cpu(), fbar_ref[idx >= bulk], 1e-4, "fbar of the split-K tail")
    for k in ref:
        assert_close(got[k], ref[k], 1e-4, k)


# ---- 3. train-step parity, 4. reproducibility ------------------------------------------------------------------------------------------------
def _train_case(which, act, mode):
    ocfg = CASES[which][0]()
    ocfg.use_normal = True
    sd = _weights(ocfg, mode, 41, out_gain=20.0, scale=0.03)
    sd["density.beta"] = torch.tensor(0.05)
    B = 64
    inp = camera_inputs(B, (0.0, 0.0, -2.0), seed=5)
    gt = make_gt(B)
    gt["rgb"] = torch.rand(B, 3, generator=torch.Generator().manual_seed(77)) * 8.0          # HDR targets: radiance in [0, 8]
    dr = make_draws(ocfg, B, n_row=ocfg.sampler.N_samples_eval, seed=2)
    lkw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05, angular_weight=0.05)

    def oracle():
        cam, dirs, _ = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
        z_all, z_eik = orc.sample_z_vals(sd, ocfg, dirs, cam, training=True, draws=dr, force_iters=1)
        D, dev = torch.float64, "cuda"            # the fp64 restatement as eager ops on the GPU (tests/test_gpu_network.py: _oracle_fp64_on_gpu)
        c = lambda v: (v.to(D) if v.dtype.is_floating_point else v).to(dev)
        d64 = orc.Draws(eik_pts=c(dr.eik_pts), nbr_off=c(dr.nbr_off))
        out, losses, grads = hdr_ref.training_step_grads({k: c(v) for k, v in sd.items()}, ocfg, act, mode, {k: c(v) for k, v in inp.items()},
                                                         {k: c(v) for k, v in gt.items()}, orc.LossCfg(**lkw), d64, step=10,
                                                         z_override=(c(z_all), c(z_eik)))
        cpu = lambda x_: {k: v.detach().cpu() for k, v in x_.items() if torch.is_tensor(v)}
        return z_all, z_eik, cpu(out), cpu(losses), cpu(grads)

    return sd, inp, gt, dr, lkw, memo(("hdr train", which, act, mode), oracle)


def _step(which, act, mode, sd, inp, gt, dr, lkw, z_all, z_eik):
    from i2sdf_amd import I2SDFLoss, I2SDFNetwork
    net = I2SDFNetwork(_conf(which, act, mode, use_normal=True))
    net.load_state_dict(sd)
    net = net.cuda().train()
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    eng = net._engine_for("cuda:0")
    c, d, nn = eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
    out = net.render(cu(inp), c, d, nn, z_all.cuda(), z_eik.cuda(), draws={"eik_pts": dr.eik_pts.cuda(), "nbr_off": dr.nbr_off.cuda()})
    losses = I2SDFLoss(**lkw)(out, cu(gt), 10)
    net.zero_grad()
    losses["loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for k, p in net.named_parameters()}
    node = out["rgb_values"].grad_fn              # the render core's autograd node keeps the saved radiance activations and outputs it used
    M_main, H = node.M_main, eng.cfg.rgb.hidden

    def masks():
        """relu(a) > 0 of the hidden layers as the library saved them, and behind them -- as layer n_lin - 1, where hdr_ref.rgb_forward puts
        an output relu -- the saved output rgb > 0 in the first three columns"""
        rs = eng.saved_to_point_major(node.rs, eng.blocked_points(1, M_main, node.rs.shape[1]))[:, :M_main]
        last = torch.zeros(1, M_main, H, device=rs.device, dtype=rs.dtype)
        last[0, :, :3] = node.rgb[:M_main]
        return torch.cat([rs, last], 0)

    return {k: v.detach() for k, v in out.items()}, losses["loss"].detach(), grads, masks


def _assert_grads_modulo_relu_flips(which, act, mode, route, grads, ref_g, masks, sd, inp, gt, dr, lkw, z_all, z_eik):
    """tests/test_gpu_idr.py: _assert_grads_modulo_relu_flips, word for word the same bars -- the difference must be a 0/1 combination of at most
    4 backward-mask flips of ReLU units whose pre-activation is zero within rounding (|pre-activation| < 1e-6) plus a residual inside 1e-4,
    the library's masks may differ from the restatement's only at such units, and every flip used must be one the library really has.  An
    output unit of a relu net is such a unit too (hdr_ref.rgb_forward hooks it as layer n_lin - 1) and counts as one of the 4."""
    from helpers import explain_by_relu_flips, hip_mask_flips, relu_flip_analysis
    ocfg = CASES[which][0]()
    ocfg.use_normal = True
    c = lambda v: (v.to(torch.float64) if v.dtype.is_floating_point else v).cuda()
    d64 = orc.Draws(eik_pts=c(dr.eik_pts), nbr_off=c(dr.nbr_off))
    run = lambda: hdr_ref.training_step_grads({k: c(v) for k, v in sd.items()}, ocfg, act, mode, {k: c(v) for k, v in inp.items()},
                                              {k: c(v) for k, v in gt.items()}, orc.LossCfg(**lkw), d64, step=10, z_override=(c(z_all), c(z_eik)))[2]
    _, cands, deltas = relu_flip_analysis(run, tau=1e-6)
    pre = relu_flip_analysis.pre
    scale = {k: float(ref_g[k].abs().max()) for k in ref_g}
    err = {k: grads[k].cpu().double().reshape(-1) - ref_g[k].double().reshape(-1) for k in ref_g}
    chosen, res = explain_by_relu_flips(err, [{k: d[k].detach().cpu().reshape(-1) for k in d} for d in deltas], scale)
    print(f"{which} {act} {mode} {route}: {len(cands)} ReLU units with |pre-activation| < 1e-6; flips that explain the difference:",
          [(cands[i][0], cands[i][1], cands[i][2], "%.1e" % cands[i][3]) for i in chosen], "residual %.2e" % max(res.values()))
    assert len(chosen) <= 4 and max(res.values()) <= 1e-4, (chosen, {k: v for k, v in res.items() if v > 1e-4})
    flips, worst = hip_mask_flips(masks().cpu(), pre)
    print(f"masks that differ between the library and the restatement: {sorted(flips)} (largest |pre-activation| among them {worst:.1e})")
    assert worst < 1e-6, f"a backward mask differs at a unit whose pre-activation is {worst:.2e}: not a rounding-level flip"
    for i in chosen:
        assert (cands[i][0], cands[i][1], cands[i][2]) in flips, f"flip {cands[i]} explains the difference but the library's mask of that unit equals the restatement's"


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("which", ["plumbing", "synthetic"])
def test_train_step_parity(which, act, mode, wgrad, monkeypatch):
    """64 rays end to end against hdr_ref.training_step_grads in fp64, ground-truth rgb in [0, 8], depths and draws given, through the fused
    loss route and the separate one, at the bars of test_train_step_parity in tests/test_gpu_idr.py."""
    sd, inp, gt, dr, lkw, (z_all, z_eik, ref_out, ref_loss, ref_g) = _train_case(which, act, mode)
    # the step is a real one for this activation: the render is not zero, and the radiance net's last layer gets a gradient
    assert float(ref_out["rgb_values"].abs().max()) > 1e-2 and float(ref_g["rendering_network.lin0.weight_v"].abs().max()) > 0
    routes = {}
    for route, env in (("fused", "1"), ("separate", "0")):
        monkeypatch.setenv("I2SDF_FUSED_RENDER_LOSS", env)
        out, loss, grads, masks = _step(which, act, mode, sd, inp, gt, dr, lkw, z_all, z_eik)
        for k in ("rgb_values", "depth_values", "weight_sum", "grad_theta"):
            assert_close(out[k].cpu(), ref_out[k], 1e-4, f"{k} ({route})")
        hit = ref_out["weight_sum"].reshape(-1) > 1e-2
        assert_close(out["normal_values"].cpu()[hit], ref_out["normal_values"][hit], 1e-4, f"normal_values ({route}, weight_sum > 0.01)")
        assert_close(loss.cpu(), ref_loss["loss"], 1e-5, f"loss ({route})")
        worst = max(rel_max(grads[k].cpu(), ref_g[k]) for k in grads)
        print(f"{which} {act} {mode} {route}: worst relative parameter-gradient error {worst:.2e}")
        if worst > 1e-4:
            _assert_grads_modulo_relu_flips(which, act, mode, route, grads, ref_g, masks, sd, inp, gt, dr, lkw, z_all, z_eik)
        for k in grads:
            assert grads[k].shape == ref_g[k].shape and bool(torch.isfinite(grads[k]).all()), k
        routes[route] = (loss, grads)
    assert_close(routes["separate"][0].cpu(), routes["fused"][0].cpu(), 1e-6, "loss, separate vs fused route")
    for k in routes["fused"][1]:
        assert_close(routes["separate"][1][k].cpu(), routes["fused"][1][k].cpu(), 1e-6, f"grad {k}, separate vs fused route")


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("which,mode", [("plumbing", "nerf"), ("synthetic", "nerf"), ("synthetic", "idr")])
def test_relu_train_step_is_bitwise_reproducible(which, mode, wgrad):
    sd, inp, gt, dr, lkw, (z_all, z_eik, *_) = _train_case(which, "relu", mode)
    a = _step(which, "relu", mode, sd, inp, gt, dr, lkw, z_all, z_eik)
    b = _step(which, "relu", mode, sd, inp, gt, dr, lkw, z_all, z_eik)
    assert torch.equal(a[1], b[1])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), f"grad {k}: {int((a[2][k] != b[2][k]).sum())} entries differ"


# ---- 5. the default is unchanged ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("which,mode", [("plumbing", "nerf"), ("synthetic", "nerf"), ("synthetic", "idr")])
def test_sigmoid_none_and_absent_are_one_network_and_relu_is_another(which, mode, wgrad):
    """`output_activation: 'sigmoid'`, `None` and no key at all: torch.equal outputs and gradients.  'relu' must NOT equal them -- where the
    activation is ignored it does."""
    sd, inp, gt, dr, lkw, (z_all, z_eik, *_) = _train_case(which, "relu", mode)
    from i2sdf_amd import I2SDFLoss, I2SDFNetwork

    def run(conf):
        net = I2SDFNetwork(conf)
        net.load_state_dict(sd)
        net = net.cuda().train()
        cu = lambda d: {k: v.cuda() for k, v in d.items()}
        eng = net._engine_for("cuda:0")
        c, d, nn = eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
        out = net.render(cu(inp), c, d, nn, z_all.cuda(), z_eik.cuda(), draws={"eik_pts": dr.eik_pts.cuda(), "nbr_off": dr.nbr_off.cuda()})
        loss = I2SDFLoss(**lkw)(out, cu(gt), 10)["loss"]
        net.zero_grad()
        loss.backward()
        return {k: v.detach() for k, v in out.items()}, {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    absent = _conf(which, None, mode, use_normal=True)
    assert "output_activation" not in absent["rendering_network"]
    none = _conf(which, None, mode, use_normal=True)
    none["rendering_network"]["output_activation"] = None
    o0, g0 = run(absent)
    for conf in (none, _conf(which, "sigmoid", mode, use_normal=True)):
        o, g = run(conf)
        assert all(torch.equal(o[k], o0[k]) for k in o0) and set(g) == set(g0) and all(torch.equal(g[k], g0[k]) for k in g0)
    o, g = run(_conf(which, "relu", mode, use_normal=True))
    assert not torch.equal(o["rgb_values"], o0["rgb_values"])
    assert not torch.equal(g["rendering_network.lin0.weight_v"], g0["rendering_network.lin0.weight_v"])
    assert torch.equal(o["depth_values"], o0["depth_values"])          # the activation touches nothing in front of the radiance net's last line


# ---- 6. checkpoint ---------------------------------------------------------------------------------------------------------------------------
def _eval_fixture():
    """the recorded 'idr' checkpoint and 32 x 32 view of tests/golden/g17_idr_eval.npz (a view on which the reference's arithmetic is well
    conditioned with the sampler in the loop, tests/golden/gen_golden_idr.py), rendered with a relu output: the last layer's bias is raised so
    that the radiance is positive on most samples and above 1 on some"""
    z = np.load(os.path.join(GOLDEN, "g17_idr_eval.npz"), allow_pickle=False)
    sd = sd_from_npz(z)
    sd["rendering_network.lin2.weight_g"] = sd["rendering_network.lin2.weight_g"] * 10.0
    sd["rendering_network.lin2.bias"] = sd["rendering_network.lin2.bias"] + 1.0
    inp = {k[3:]: t(z[k]) for k in z.files if k.startswith("in.")}
    return z, sd, inp


def test_checkpoint_round_trip_eval_render_and_render_image(tmp_path):
    from i2sdf_amd import I2SDFNetwork, plumbing_conf
    z, sd, inp = _eval_fixture()
    conf = hdr_ref.hdr_conf(plumbing_conf(skip=True), "relu", "idr")
    conf["use_normal"] = True
    first = I2SDFNetwork(conf)
    first.load_state_dict(sd)
    path = os.path.join(str(tmp_path), "relu.pth")
    torch.save(first.state_dict(), path)
    saved = torch.load(path)
    assert list(saved) == list(first.state_dict()) and not any("activation" in k for k in saved)
    net = I2SDFNetwork(conf)                      # a fresh module
    net.load_state_dict(saved)
    net = net.cuda().eval()
    assert net.rendering_network.output_activation == "relu"
    ocfg = orc.plumbing_cfg(skip=True)
    ocfg.use_normal = True
    zo = (t(z["ref.z_vals"]), t(z["ref.z_eik"]))
    ref = memo("hdr eval", lambda: {k: v.detach() for k, v in hdr_ref.network_forward(dbl(sd), ocfg, "relu", "idr", {k: v.double() for k, v in inp.items()}, False,
                                                                                   z_override=(zo[0].double(), zo[1].double())).items() if torch.is_tensor(v)})
    sig = idr_ref.network_forward(dbl(sd), ocfg, {k: v.double() for k, v in inp.items()}, False, z_override=(zo[0].double(), zo[1].double()))
    assert float(ref["rgb_values"].max()) > 1.0 and rel_max(sig["rgb_values"], ref["rgb_values"]) > 0.05      # HDR, and not the sigmoid's render
    cinp = {k: v.cuda() for k, v in inp.items()}
    eng = net._engine_for("cuda:0")
    c, d, n = eng.ray_setup(cinp["uv"], cinp["pose"], cinp["intrinsics"])
    with torch.no_grad():
        out = net.render(cinp, c, d, n, zo[0].cuda(), zo[1].cuda())
        img = net.render_image(cinp, split_n_pixels=1024)
    hit = ref["weight_sum"].reshape(-1) > 1e-2
    for name, o in (("render", out), ("render_image", img)):
        for k in ("rgb_values", "depth_values", "weight_sum"):
            assert_close(o[k].cpu().reshape(ref[k].shape), ref[k], 1e-4, f"{k} ({name})")
        assert_close(o["normal_map"].cpu()[hit], ref["normal_map"][hit], 1e-4, f"normal_map ({name}, weight_sum > 0.01)")


# ---- 7. views ---------------------------------------------------------------------------------------------------------------------------------
SRGB_TOL = 1e-6              # absolute: a powf, a subtraction, a product and a sum at magnitude <= 1.06, each within a few fp32 roundings of 6e-8, tenfold margin


def test_linear_to_srgb():
    from i2sdf_amd import views as V
    z = np.load(os.path.join(GOLDEN, "g21_hdr_tonemap.npz"), allow_pickle=False)
    grid = t(z["x"])
    rnd = torch.rand(100000, generator=torch.Generator().manual_seed(9)) * 9.5 - 0.5           # [-0.5, 9]
    for name, x in (("fixture grid", grid), ("random", rnd)):
        for clamp in (True, False):
            got = V.linear_to_srgb(x.cuda(), clamp=clamp).cpu()
            want = hdr_ref.linear_to_srgb(x.double(), clamp)
            # clamped (the default, what the validation uses): absolute.  Unclamped the values leave [0, 1.06] on both sides (12.92 x below 0,
            # x^(1/2.4) above 1) and the same few roundings are relative to the magnitude: the error is taken over max(1, |value|)
            err = float(((got.double() - want).abs() / (1.0 if clamp else want.abs().clamp_min(1.0))).max())
            xs = x
            print(f"linear_to_srgb, {name}, clamp={clamp}: max {'abs' if clamp else 'scaled'} error {err:.2e}")
            assert got.dtype == torch.float32 and err <= SRGB_TOL
            assert bool((got[xs == 0] == 0).all())
            if clamp:
                assert bool((got[xs >= 1] == 1.0).all()) and bool((got[xs <= 0] == 0.0).all()) and int((xs >= 1).sum()) > 0
    assert_close(V.linear_to_srgb(grid.cuda(), clamp=True).cpu(), t(z["srgb64_clamped"]), SRGB_TOL, "recorded reference (fp64)", floor=1.0)
    # in place, any shape, empty
    x = rnd.reshape(100, 250, 4).cuda()
    want = V.linear_to_srgb(x)
    y = x.clone()
    assert V.linear_to_srgb(y, out=y) is y and torch.equal(y, want) and want.shape == x.shape
    assert V.linear_to_srgb(torch.empty(0, 3, device="cuda")).shape == (0, 3)
    with pytest.raises(ValueError, match="float32"):
        V.linear_to_srgb(x.double())


def _hdr_views(H, W):
    """3 HDR view pairs: the seeded views of tests/views_ref.py stretched to [-0.4, 2] -- values below 0, between, and above 1 (clamped)"""
    def make():
        pairs = [VR.view_pair(H, W, seed=2000 * H + 10 * W + v, noise=0.05) for v in range(3)]
        pred = (np.stack([p for p, _ in pairs]) * 2.4 - 0.4).astype(np.float32)
        gt = (np.stack([g for _, g in pairs]) * 2.4 - 0.4).astype(np.float32)
        tone = lambda a: hdr_ref.linear_to_srgb(torch.from_numpy(a).double(), True).numpy()
        return pred, gt, tone(pred), tone(gt)
    return memo(("hdr views", H, W), make)


@pytest.mark.parametrize("H,W", [(11, 11), (26, 42), (33, 70)])
def test_image_metrics_hdr(H, W):
    """hdr=True is the explicit tone map followed by the plain call, bit for bit; the result agrees with tests/views_ref.py
    (a) on the library's own tone-mapped images at the bars of tests/test_gpu_views.py (SSE 1e-12 relative, PSNR 1e-10 dB, SSIM map 2 E32,
        mean 1e-12 of its own map), and
    (b) on the fp64 tone-mapped images at those bars widened by what an input error of delta = SRGB_TOL + 2^-24 (the tone map's own bar
        and the rounding of the fp64 image to fp32) can do: with N values and e = sqrt(SSE / N),  |d SSE| <= 4 delta sqrt(N SSE) + 4 N delta^2,
        so |d PSNR| <= (10 / ln 10) (4 delta / e + 4 delta^2 / e^2);  SSIM = A B with |A|, |B| <= 1 on these images,
        A = (2 mp mt + c1) / (mp^2 + mt^2 + c1), B = (2 spt + c2) / (sp + st + c2), values in [0, 1]:  numerator and denominator of A
        move by at most 4 delta + 2 delta^2, those of B by at most 8 delta + 4 delta^2, hence to first order
        |d SSIM| <= 2 (4 delta) / min den A + 2 (8 delta) / min den B, the minima taken over the fp64 reference's own maps."""
    from i2sdf_amd import views as V
    pred, gt, tp64, tg64 = _hdr_views(H, W)
    assert pred.min() < 0 and pred.max() > 1 and gt.min() < 0 and gt.max() > 1
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    tp, tg = V.linear_to_srgb(p), V.linear_to_srgb(g)
    assert float((tp.cpu().double() - torch.from_numpy(tp64)).abs().max()) <= SRGB_TOL and float(tp.min()) == 0.0 and float(tp.max()) == 1.0
    m = V.image_metrics(p, g, (H, W), hdr=True)
    plain = V.image_metrics(tp, tg, (H, W))
    assert torch.equal(m["psnr"], plain["psnr"]) and torch.equal(m["ssim"], plain["ssim"])
    assert torch.equal(V.psnr(p, g, (H, W), hdr=True), m["psnr"]) and torch.equal(V.ssim(p, g, (H, W), hdr=True), m["ssim"])
    assert not torch.equal(V.image_metrics(p, g, (H, W))["psnr"], m["psnr"])
    assert torch.equal(p, torch.from_numpy(pred).cuda()) and torch.equal(g, torch.from_numpy(gt).cuda())      # the inputs are not touched
    mean, smap = V.ssim(p, g, (H, W), hdr=True, return_map=True)
    assert torch.equal(mean, m["ssim"])
    own_p, own_g = tp.cpu().numpy(), tg.cpu().numpy()
    delta = SRGB_TOL + 2.0 ** -24
    N = 3 * H * W
    for v in range(3):
        # (a) the library's own tone-mapped images
        want = VR.sse(own_p[v], own_g[v])
        sse = 10.0 ** (-float(m["psnr"][v]) / 10.0) * N
        assert abs(sse - want) <= 1e-11 * want                      # (the SSE recovered from the PSNR: the log costs a digit)
        assert abs(float(m["psnr"][v]) - VR.psnr(own_p[v], own_g[v])) <= 1e-10
        f64 = VR.ssim_map_f64(own_p[v].reshape(H, W, 3), own_g[v].reshape(H, W, 3), None)
        f32 = VR.ssim_map_f32_conv2d(own_p[v].reshape(H, W, 3), own_g[v].reshape(H, W, 3), None)
        e32 = float(np.abs(f32.astype(np.float64) - f64).max())
        got = smap[v].cpu().numpy().astype(np.float64)
        assert e32 > 0 and float(np.abs(got - f64).max()) <= 2 * e32
        assert abs(float(mean[v]) - got.mean()) <= 1e-12 * abs(got.mean())
        # (b) the fp64 tone-mapped images
        a32, b32 = tp64[v].astype(np.float32), tg64[v].astype(np.float32)
        e = math.sqrt(VR.sse(a32, b32) / N)
        d_psnr = (10.0 / math.log(10.0)) * (4 * delta / e + 4 * delta ** 2 / e ** 2)
        assert abs(float(m["psnr"][v]) - VR.psnr(a32, b32)) <= 1e-10 + d_psnr, (float(m["psnr"][v]), VR.psnr(a32, b32), d_psnr)
        a, b = a32.astype(np.float64).reshape(H, W, 3), b32.astype(np.float64).reshape(H, W, 3)
        R = VR.data_range_of(a32, b32)
        k2d = np.outer(VR.gaussian(), VR.gaussian())
        ma, mb, maa, mbb = (VR._valid_window_2d(x_, k2d) for x_ in (a, b, a * a, b * b))
        den_a = ma * ma + mb * mb + (0.01 * R) ** 2
        den_b = (maa - ma * ma) + (mbb - mb * mb) + (0.03 * R) ** 2
        d_ssim = 2 * (4 * delta) / float(den_a.min()) + 2 * (8 * delta) / float(den_b.min())
        ref64 = VR.ssim_map_f64(a32.reshape(H, W, 3), b32.reshape(H, W, 3), None)
        print(f"{H}x{W} view {v}: psnr {float(m['psnr'][v]):.6f} (fp64 images {VR.psnr(a32, b32):.6f}, bound {d_psnr:.1e}); ssim {float(mean[v]):.8f} "
              f"(fp64 images {ref64.mean():.8f}, bound {2 * e32 + d_ssim:.1e})")
        assert float(np.abs(got - ref64).max()) <= 2 * e32 + d_ssim
        assert abs(float(mean[v]) - ref64.mean()) <= 2 * e32 + d_ssim


def test_to_frames_hdr():
    from i2sdf_amd import views as V
    H, W = 26, 42
    pred, _, _, _ = _hdr_views(H, W)
    p = torch.from_numpy(pred).cuda()
    a = V.to_frames(rgb=p, img_res=(H, W), hdr=True)["rgb8"]
    b = V.to_frames(rgb=V.linear_to_srgb(p), img_res=(H, W))["rgb8"]
    assert torch.equal(a, b) and a.dtype == torch.uint8 and int(a.max()) == 255 and int(a.min()) == 0
    assert not torch.equal(a, V.to_frames(rgb=p, img_res=(H, W))["rgb8"])
    assert np.array_equal(a.cpu().numpy().reshape(3, H * W, 3), VR.rgb8_f32(V.linear_to_srgb(p).cpu().numpy()))
    d = torch.rand(3, H * W, 1, device="cuda")
    both = V.to_frames(rgb=p, depth=d, img_res=(H, W), hdr=True)
    assert torch.equal(both["rgb8"], a) and torch.equal(both["depth8"], V.to_frames(depth=d, img_res=(H, W))["depth8"])


def test_evaluate_views_hdr():
    """2 views of 24 x 32 with a relu net: metrics and rgb8 from the tone-mapped images, rgb_values the raw render."""
    from i2sdf_amd import I2SDFNetwork, plumbing_conf
    from i2sdf_amd import views as V
    H, W = 24, 32
    conf = hdr_ref.hdr_conf(plumbing_conf(), "relu")
    conf["use_normal"] = True
    ocfg = orc.plumbing_cfg()
    sd = orc.perturb_params(orc.init_params(ocfg, seed=41), 0.05, seed=42)
    sd["density.beta"] = torch.tensor(0.05)
    sd["rendering_network.lin2.weight_g"] = sd["rendering_network.lin2.weight_g"] * 10.0          # (radiance above 1 on four pixels in ten)
    sd["rendering_network.lin2.bias"] = sd["rendering_network.lin2.bias"] + 1.0
    net = I2SDFNetwork(conf)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    K = torch.eye(4); K[0, 0] = K[1, 1] = 30.0; K[0, 2], K[1, 2] = W / 2, H / 2
    p0, p1 = VR.pose_pair(3, 25.0, t_scale=0.3)
    p0[:3, 3] += -1.8 * p0[:3, 2]; p1[:3, 3] += -1.8 * p1[:3, 2]
    poses = torch.from_numpy(np.stack([p0, p1])).float().cuda()
    gt = torch.from_numpy(np.stack([VR.view_pair(H, W, 50 + v, 0.0)[1] for v in range(2)])).cuda() * 3.0
    res = net.evaluate_views(poses, K.cuda(), (H, W), gt_rgb=gt, split_n_pixels=300, frames=True, hdr=True)
    raw = net.evaluate_views(poses, K.cuda(), (H, W), gt_rgb=gt, split_n_pixels=300, frames=True)
    assert torch.equal(res["rgb_values"], raw["rgb_values"]) and float(res["rgb_values"].max()) > 1.0        # the raw render (hdr_eval), HDR indeed
    m = V.image_metrics(V.linear_to_srgb(res["rgb_values"]), V.linear_to_srgb(gt), (H, W))
    assert torch.equal(res["psnr"], m["psnr"]) and torch.equal(res["ssim"], m["ssim"])
    assert not torch.equal(res["psnr"], raw["psnr"])
    assert torch.equal(res["rgb8"], V.to_frames(rgb=V.linear_to_srgb(res["rgb_values"]), img_res=(H, W))["rgb8"])
    assert not torch.equal(res["rgb8"], raw["rgb8"])
    for k in ("normal8", "depth8", "depth_values", "normal_map", "sampler_iters"):
        assert torch.equal(res[k], raw[k]), k
    lean = net.evaluate_views(poses, K.cuda(), (H, W), gt_rgb=gt, split_n_pixels=300, frames=True, keep_outputs=False, hdr=True)
    for k in ("psnr", "ssim", "rgb8"):
        assert torch.equal(lean[k], res[k]), k
