"""GPU: fused I2SDFLoss (value + gradients in HIP) vs the fp64 oracle loss and the reference's golden values."""
import pytest
import torch

from helpers import assert_close, t

pytestmark = pytest.mark.gpu


def _rand_case(B, n_pc, light, seed):
    g = torch.Generator().manual_seed(seed)
    out = {"rgb_values": torch.rand(B, 3, generator=g), "depth_values": torch.rand(B, generator=g) * 3, "weight_sum": torch.rand(B, 1, generator=g),
           "grad_theta": torch.randn(2 * B, 3, generator=g), "diff_norm": torch.rand(B, generator=g),
           "normal_values": torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1), "surface_sdf": torch.randn(n_pc, 1, generator=g) * 0.1}
    gt = {"rgb": torch.rand(B, 3, generator=g), "depth": torch.rand(B, generator=g) * 3, "depth_mask": torch.rand(B, generator=g) > 0.3,
          "normal": torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1), "normal_mask": torch.rand(B, generator=g) > 0.3,
          "mask": (torch.rand(B, 1, generator=g) > 0.5).float()}
    if light:
        out["light_mask"] = torch.rand(B, 1, generator=g)
        gt["light_mask"] = (torch.rand(B, 1, generator=g) > 0.5).float()
    return out, gt


@pytest.mark.parametrize("light,kw,step", [
    (False, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, depth_weight=0.1, normal_weight=0.05, bubble_weight=0.5,
                 min_bubble_iter=50000, max_bubble_iter=150000), 160000),
    (True, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05, light_mask_weight=0.5,
                mask_weight=0.3), 10),
    (False, dict(eikonal_weight=0.1, depth_weight=0.0, normal_weight=0.0, angular_weight=0.0), 10),
])
def test_fused_loss_matches_oracle(light, kw, step):
    """values and the gradient w.r.t. every network output vs the fp64 oracle loss (oracle.i2sdf_loss + torch.autograd on CPU)."""
    from i2sdf_amd import I2SDFLoss
    from oracle import i2sdf_oracle as orc
    out, gt = _rand_case(777, 41, light, seed=3)
    fused = I2SDFLoss(**kw)
    lc = orc.LossCfg(**{k: v for k, v in kw.items() if k in orc.LossCfg.__dataclass_fields__})
    lc.smooth_iter = fused.smooth_iter
    o1 = {k: v.cuda().requires_grad_(True) for k, v in out.items()}
    o2 = {k: v.double().requires_grad_(True) for k, v in out.items()}
    gtc = {k: v.cuda() for k, v in gt.items()}
    gt64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in gt.items()}
    l1, l2 = fused(o1, gtc, step), orc.i2sdf_loss(o2, gt64, lc, step)
    for k in l2:
        assert_close(l1[k].detach().cpu(), l2[k].detach(), 2e-6, k)
    (l1["loss"] * 1.7).backward()
    (l2["loss"] * 1.7).backward()
    for k in o1:
        g2 = o2[k].grad if o2[k].grad is not None else torch.zeros_like(o2[k])
        g1 = o1[k].grad if o1[k].grad is not None else torch.zeros_like(o1[k])
        if g2.abs().max() == 0:
            assert g1.abs().max() == 0, k
        else:
            assert_close(g1.cpu(), g2, 1e-5, "grad " + k)


def test_fused_loss_golden(golden):
    from i2sdf_amd import I2SDFLoss
    z = golden("g11_loss")
    out = {k[4:]: t(z[k]).cuda() for k in z.files if k.startswith("out.")}
    gt = {k[3:]: t(z[k]).cuda() for k in z.files if k.startswith("gt.")}
    kw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, depth_weight=0.1, normal_weight=0.05, bubble_weight=0.5,
              min_bubble_iter=50000, max_bubble_iter=150000)
    l1 = I2SDFLoss(**kw)(out, gt, 160000)
    l2 = I2SDFLoss(light_mask_weight=0.5, **kw)(out, gt, 60000)
    for k in l1:
        assert_close(l1[k].cpu(), z["synthetic." + k], 2e-6, "synthetic." + k)
        assert_close(l2[k].cpu(), z["light." + k], 2e-6, "light." + k)


def test_extra_points_and_backward_seeds_match_the_torch_glue_bitwise():
    """i2sdf_extra_points / i2sdf_backward_seeds replace a multiply, two adds, a concatenation / three fills and two copies of torch
    glue (model/network/__init__.py:175-186 and autograd's accumulation): same bits."""
    import torch
    from i2sdf_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    for B in (1, 77, 1024):
        cam, dirs = torch.randn(B, 3, generator=g).to(dev), torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(dev)
        z, eik, off = (torch.rand(B, 1, generator=g) * 5).to(dev), (torch.rand(B, 3, generator=g) * 6 - 3).to(dev), ((torch.rand(B, 3, generator=g) - 0.5) * 0.01).to(dev)
        out = torch.full((3 * B + 5, 3), 7.0, device=dev)
        L.check(lib.i2sdf_extra_points(L.ptr(cam), L.ptr(dirs), L.ptr(z), L.ptr(eik), L.ptr(off), B, L.ptr(out), L.stream_ptr()), "extra_points")
        near = cam + z * dirs
        assert torch.equal(out[:3 * B], torch.cat([eik, near, near + off], 0))
        assert torch.equal(out[3 * B:], torch.full((5, 3), 7.0, device=dev)), "rows beyond 3B must be left alone"
    for (Mm, n_eik, n_pc, tail, n_beta, zero_main, with_e, with_s) in ((0, 0, 0, 0, 1, 0, False, False), (640, 96, 0, 32, 3, 0, True, False),
                                                                         (640, 96, 17, 15, 1, 1, True, True), (99328, 3072, 0, 0, 1, 0, True, False),
                                                                         (256, 30, 9, 3, 2, 1, False, True)):
        Ms = Mm + n_eik + n_pc + tail
        beta = torch.full((n_beta + 2,), 5.0, device=dev)
        sbar, nbar = torch.full((max(Ms, 1),), 3.0, device=dev), torch.full((max(Ms, 1), 3), 4.0, device=dev)
        ge = torch.randn(n_eik, 3, generator=g).to(dev) if with_e else None
        gs = torch.randn(n_pc, generator=g).to(dev) if with_s else None
        L.check(lib.i2sdf_backward_seeds(L.ptr(beta), n_beta, L.ptr(sbar), L.ptr(nbar), Mm, Ms, L.ptr(ge), n_eik, L.ptr(gs), n_pc, zero_main,
                                         L.stream_ptr()), "backward_seeds")
        assert torch.equal(beta, torch.cat([torch.zeros(n_beta, device=dev), torch.full((2,), 5.0, device=dev)]))
        es, en = torch.full((max(Ms, 1),), 3.0, device=dev), torch.full((max(Ms, 1), 3), 4.0, device=dev)
        if Ms > 0:
            es[Mm:Ms] = 0.0
            en[Mm:Ms] = 0.0
            if zero_main:
                en[:Mm] = 0.0
            if with_e:
                en[Mm:Mm + n_eik] = ge
            if with_s:
                es[Mm + n_eik:Mm + n_eik + n_pc] = gs
        assert torch.equal(sbar, es) and torch.equal(nbar, en), (Mm, n_eik, n_pc)
    # argument checks
    assert lib.i2sdf_backward_seeds(None, 1, None, None, 0, 0, None, 0, None, 0, 0, L.stream_ptr()) != 0
    assert lib.i2sdf_backward_seeds(L.ptr(beta), 1, L.ptr(sbar), L.ptr(nbar), 10, 12, None, 3, None, 0, 0, L.stream_ptr()) != 0      # n_eik > extra rows


# ---- round 6: loss + render backward fused (i2sdf_render_loss_backward) against the separate path, same process, same draws -------------
def _step(net, loss_fn, inp, gt, draws, step, fused, scale=1.0, extra=None):
    """one forward + loss + backward; returns (loss dict, flat gradient copy).  fused=False forces the separate path."""
    import os
    os.environ["I2SDF_FUSED_RENDER_LOSS"] = "1" if fused else "0"
    try:
        for p in net.parameters():
            p.grad = None
        out = net(inp, draws=draws)
        res = loss_fn(out, gt, step)
        tot = res["loss"] * scale
        if extra is not None:
            tot = tot + extra(out)
        tot.backward()
        g = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
        return {k: v.detach().clone() for k, v in res.items()}, g, out
    finally:
        os.environ.pop("I2SDF_FUSED_RENDER_LOSS", None)


@pytest.mark.parametrize("light,n_pc,step,scale", [(False, 0, 10, 1.0), (True, 0, 10, 0.37), (False, 37, 60000, 1.0), (False, 0, 200000, 2.5)])
def test_fused_render_loss_equals_the_separate_path(light, n_pc, step, scale, wgrad_mode):
    """The module's default path -- I2SDFLoss recognises the outputs of a training render and runs loss + render backward as one fused library
    call -- against the separate entry points (I2SDF_FUSED_RENDER_LOSS=0): same reported values, same parameter gradients (the per-sample
    gradients are computed by the same device functions; sums are taken in a different but fixed order -> 1e-6), with a light head, with a
    bubble point cloud (step inside the bubble window), with the smoothness term active (step behind smooth_iter) and with an upstream
    gradient that is not 1."""
    from i2sdf_amd import I2SDFNetwork, I2SDFLoss, synthetic_conf
    from helpers import camera_inputs, make_gt
    conf = synthetic_conf(light)
    conf["use_normal"] = True
    torch.manual_seed(5)
    net = I2SDFNetwork(conf).cuda().train()
    with torch.no_grad():
        net.density.beta.fill_(0.05)
    B = 203
    inp = {k: v.cuda() for k, v in camera_inputs(B, (0.0, 0.0, -2.0), seed=11).items()}
    if n_pc:
        inp["pointcloud"] = (torch.rand(n_pc, 3, device="cuda") * 2 - 1) * 0.7
    gt = {k: v.cuda() for k, v in make_gt(B).items()}
    gt["depth_mask"][::3] = False
    gt["normal_mask"][1::4] = False
    if light:
        gt["light_mask"] = (torch.rand(B, 1, device="cuda") > 0.5).float()
    loss_fn = I2SDFLoss(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, depth_weight=0.1, normal_weight=0.05, bubble_weight=0.5 if n_pc else 0.0,
                        min_bubble_iter=50000, max_bubble_iter=150000, light_mask_weight=0.5 if light else 0.0)
    eng = net._engine_for(torch.device("cuda:0"))
    draws = {k: v for k, v in eng.training_draws(B, 1234, "cuda", net.scene_bounding_sphere).items() if v is not None}
    net.force_iters = 2
    r_sep, g_sep, _ = _step(net, loss_fn, inp, gt, draws, step, fused=False, scale=scale)
    r_fus, g_fus, out = _step(net, loss_fn, inp, gt, draws, step, fused=True, scale=scale)
    assert getattr(out["rgb_values"], "_i2sdf_render", None) is not None
    for k in r_sep:
        assert_close(r_fus[k], r_sep[k], 2e-6, f"loss term {k}", floor=1e-6)
    assert torch.isfinite(g_fus).all()
    assert_close(g_fus, g_sep, 2e-6, "parameter gradients, fused vs separate")


def test_fused_render_loss_with_other_consumers_of_the_outputs(wgrad_mode):
    """Another differentiable term on the same outputs: the loss's seeds reach _RenderFn.backward summed with foreign gradients -- the fused
    path must notice (its placeholders do not arrive untouched), correct for the upstream scale and give what the separate path gives."""
    from i2sdf_amd import I2SDFNetwork, I2SDFLoss, synthetic_conf
    from helpers import camera_inputs, make_gt
    conf = synthetic_conf(False)
    conf["use_normal"] = True
    torch.manual_seed(6)
    net = I2SDFNetwork(conf).cuda().train()
    B = 64
    inp = {k: v.cuda() for k, v in camera_inputs(B, (0.0, 0.0, -2.0), seed=12).items()}
    gt = {k: v.cuda() for k, v in make_gt(B).items()}
    loss_fn = I2SDFLoss(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05)
    eng = net._engine_for(torch.device("cuda:0"))
    draws = {k: v for k, v in eng.training_draws(B, 99, "cuda", net.scene_bounding_sphere).items() if v is not None}
    net.force_iters = 1
    for extra in (lambda o: 0.1 * o["rgb_values"].sum() + 0.05 * o["depth_values"].mean(),
                  lambda o: 0.02 * o["grad_theta"].pow(2).sum(),
                  lambda o: 0.3 * o["diff_norm"].sum() + 0.1 * o["normal_values"][:, 0].sum()):
        _, g_sep, _ = _step(net, loss_fn, inp, gt, draws, 10, fused=False, scale=0.7, extra=extra)
        _, g_fus, _ = _step(net, loss_fn, inp, gt, draws, 10, fused=True, scale=0.7, extra=extra)
        assert_close(g_fus, g_sep, 5e-6, "parameter gradients with a foreign term, fused vs separate")


def test_fused_render_loss_called_twice_on_the_same_outputs(wgrad_mode):
    """Two loss calls on one render's outputs (e.g. a logging call and the training call with other weights), backward through a weighted
    sum of both: the first call's prepared gradients are superseded by the second's -- its node must then give autograd real, scaled
    gradients -- and the result must equal the separate path's."""
    from i2sdf_amd import I2SDFNetwork, I2SDFLoss, synthetic_conf
    from helpers import camera_inputs, make_gt
    import os
    conf = synthetic_conf(False)
    conf["use_normal"] = True
    torch.manual_seed(8)
    net = I2SDFNetwork(conf).cuda().train()
    B = 48
    inp = {k: v.cuda() for k, v in camera_inputs(B, (0.0, 0.0, -2.0), seed=13).items()}
    gt = {k: v.cuda() for k, v in make_gt(B).items()}
    l1 = I2SDFLoss(eikonal_weight=0.1, depth_weight=0.1, normal_weight=0.05)
    l2 = I2SDFLoss(eikonal_weight=0.3, depth_weight=0.0, normal_weight=0.2, smooth_weight=0.05, smooth_iter=None)
    eng = net._engine_for(torch.device("cuda:0"))
    draws = {k: v for k, v in eng.training_draws(B, 5, "cuda", net.scene_bounding_sphere).items() if v is not None}
    net.force_iters = 1
    res = []
    for fused in (False, True):
        os.environ["I2SDF_FUSED_RENDER_LOSS"] = "1" if fused else "0"
        try:
            for p in net.parameters():
                p.grad = None
            out = net(inp, draws=draws)
            a, b = l1(out, gt, 10)["loss"], l2(out, gt, 10)["loss"]
            (0.6 * a + 1.7 * b).backward()
            res.append((torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone(), a.detach().clone(), b.detach().clone()))
        finally:
            os.environ.pop("I2SDF_FUSED_RENDER_LOSS", None)
    assert_close(res[1][1], res[0][1], 2e-6, "first loss value"); assert_close(res[1][2], res[0][2], 2e-6, "second loss value")
    assert_close(res[1][0], res[0][0], 5e-6, "parameter gradients of a weighted sum of two loss calls, fused vs separate")


# ---- the fused path (the default gradient path of every training step) against the fp64 oracle, term by term -----------------------------
from oracle import i2sdf_oracle as orc                    # noqa: E402
from helpers import camera_inputs, make_draws, make_gt, memo, rel_max      # noqa: E402

_LOSS_KEYS = ("loss", "rgb_loss", "eikonal_loss", "smooth_loss", "mask_loss", "depth_loss", "normal_loss", "angular_loss", "bubble_loss",
              "light_mask_loss")


def _given_depths_case(B, light, n_pc, masks, seed):
    """A synthetic.yml network (fixed weights, beta = 0.05), B rays, depths pinned by the oracle's sampler (force_iters=1), fixed draws."""
    ocfg = orc.synthetic_cfg(light)
    ocfg.use_normal = True
    sd = orc.perturb_params(orc.init_params(ocfg, seed=41), 0.03, seed=42)
    sd["density.beta"] = torch.tensor(0.05)
    inp = camera_inputs(B, (0.0, 0.0, -2.0), seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    if n_pc:
        inp["pointcloud"] = (torch.rand(n_pc, 3, generator=g) * 2 - 1) * 0.7
    gt = make_gt(B, seed=seed, light=light)
    for key, kind in zip(("depth_mask", "normal_mask"), masks):
        gt[key] = {"random": torch.rand(B, generator=g) > 0.4, "all": torch.ones(B, dtype=torch.bool),
                   "none": torch.zeros(B, dtype=torch.bool)}[kind]
    dr = make_draws(ocfg, B, n_row=128, seed=seed + 1)
    cam, dirs, _ = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
    z_all, z_eik = memo(("given-depths case", B, light, n_pc, seed), lambda: orc.sample_z_vals(sd, ocfg, dirs, cam, training=True, draws=dr, force_iters=1))
    # the object mask: the label a ray's weight_sum agrees with where weight_sum < 0.05 or > 0.95 (rays beyond the clip included), random
    # in between.  A ray labelled against a weight_sum of 1 - 1e-3 + tiny would weigh its seed by 1 / (1 - weight_sum): fp32 rounding of
    # weight_sum, not the kernels, would then decide the gradient (measured: 1.5e-4 on implicit_network.lin0.bias with random labels).
    w = memo(("given-depths weight_sum", B, light, n_pc, seed), lambda: orc.network_forward(
        {k: v.double().cuda() for k, v in sd.items()}, ocfg, {k: v.double().cuda() for k, v in inp.items()}, True, predict_only=True,
        z_override=(z_all.double().cuda(), z_eik.double().cuda()))["weight_sum"].detach().cpu())
    label = (torch.rand(B, 1, generator=g) > 0.5).double()
    gt["mask"] = torch.where((w - 0.5).abs() > 0.45, (w > 0.5).double(), label).float()
    return ocfg, sd, inp, gt, dr, z_all, z_eik


def _oracle_step(sd, ocfg, inp, gt, lc, dr, z_all, z_eik, step, scale, T=None, retain=()):
    """fp64 training step as eager torch on the GPU: network_forward -> T(outputs) -> i2sdf_loss -> (loss * scale).backward()
    (T = ("late", fn): fn(outputs) after the loss call instead).  T is the same transformation the HIP side applies (detach, hooks, in-place edits behave identically in plain torch).  Returns CPU tensors:
    outputs, loss terms, parameter gradients, .grad of the outputs in `retain`."""
    D = torch.float64
    c = lambda v: (v.to(D) if v.dtype.is_floating_point else v).cuda()
    params = {k: v.to(D).cuda().requires_grad_(True) for k, v in sd.items()}
    d64 = orc.Draws(eik_pts=c(dr.eik_pts), nbr_off=c(dr.nbr_off))
    out = orc.network_forward(params, ocfg, {k: c(v) for k, v in inp.items()}, True, d64, z_override=(c(z_all), c(z_eik)))
    out = {k: v for k, v in out.items() if not k.startswith("_")}
    early, late = (None, T[1]) if isinstance(T, tuple) else (T, None)
    if early is not None:
        early(out)
    for k in retain:
        out[k].retain_grad()
    losses = orc.i2sdf_loss(out, {k: c(v) for k, v in gt.items()}, lc, step)
    if late is not None:
        late(out)
    (losses["loss"] * scale).backward()
    cpu = lambda v: v.detach().cpu()
    return ({k: cpu(v) for k, v in out.items()}, {k: cpu(v) for k, v in losses.items()},
            {k: cpu(p.grad) if p.grad is not None else torch.zeros_like(p, device="cpu") for k, p in params.items()},
            {k: cpu(out[k].grad) for k in retain})


def _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, step, scale, fused, T=None, retain=()):
    """The same step through I2SDFNetwork.render + I2SDFLoss; fused=False forces the separate path (I2SDF_FUSED_RENDER_LOSS=0).  Returns
    (loss terms, {param: grad}, retained .grad, number of _RenderFn backwards that took the fast path)."""
    import os
    from test_gpu_network import cuda
    from i2sdf_amd import network as N
    fast = []
    orig = N._RenderFn._backward_from_seeds

    def counting(ctx, pre, gflat):
        fast.append(1)
        return orig(ctx, pre, gflat)
    os.environ["I2SDF_FUSED_RENDER_LOSS"] = "1" if fused else "0"
    N._RenderFn._backward_from_seeds = staticmethod(counting)
    try:
        eng = net._engine_for("cuda:0")
        c, d, n = eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
        out = net.render(cuda(inp), c, d, n, z_all.cuda(), z_eik.cuda(), draws={"eik_pts": dr.eik_pts.cuda(), "nbr_off": dr.nbr_off.cuda()})
        early, late = (None, T[1]) if isinstance(T, tuple) else (T, None)
        if early is not None:
            early(out)
        for k in retain:
            out[k].retain_grad()
        losses = loss_fn(out, cuda(gt), step)
        if late is not None:
            late(out)
        net.zero_grad()
        (losses["loss"] * scale).backward()
        grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu() for k, p in net.named_parameters()}
        return ({k: v.detach().cpu() for k, v in losses.items()}, grads, {k: out[k].grad.detach().cpu() for k in retain}, len(fast))
    finally:
        N._RenderFn._backward_from_seeds = orig
        os.environ.pop("I2SDF_FUSED_RENDER_LOSS", None)


def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads.values()])


def _assert_grads_match_oracle(grads, ref_g, what, tol=1e-4):
    worst = 0.0
    for k, r in ref_g.items():
        if float(r.abs().max()) == 0.0:
            assert float(grads[k].abs().max()) == 0.0, f"{what}: grad {k} must be exactly zero"
        else:
            worst = max(worst, assert_close(grads[k], r, tol, f"{what}: grad {k}"))
    return worst


def _assert_terms(l_hip, l_ref, tol, what, floor=0.0):
    """loss terms; a term the reference reports as NaN (an empty masked mean) must be NaN on the HIP side too.  Two terms are measured on
    their natural O(1) scale (assert_close's floor): smooth_loss, a mean of |n(x) - n(x + 5e-3)| over unit normals n, small differences of
    unit vectors; mask_loss, a BCE (log 2 for an undecided ray) whose value at a ray near the clip edge moves with fp32 rounding of
    weight_sum.  At 1 - 7 rays both came out at 1.2e-5 - 1.9e-5 relative to their own small values."""
    worst = 0.0
    for k in _LOSS_KEYS:
        a, b = l_hip[k].double(), l_ref[k].double()
        if torch.isnan(b):
            assert torch.isnan(a), f"{what}: {k} is NaN in the reference, {float(a)} here"
            continue
        f_ = max(floor, 1.0) if k in ("smooth_loss", "mask_loss") else floor
        worst = max(worst, assert_close(a, b, tol, f"{what}: {k}", floor=f_))
    return worst


# every term of oracle.i2sdf_loss is on in at least one case and off in at least one: (id, light, n_pc, B, loss kwargs, step, masks, scale)
_ORACLE_CASES = [
    ("mask-angular-B203", False, 0, 203, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, mask_weight=0.3, depth_weight=0.1,
                                              normal_weight=0.0, angular_weight=0.05), 10, ("random", "random"), 1.0),
    ("light-bubble-B5", True, 37, 5, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, bubble_weight=0.5, min_bubble_iter=50000,
                                          max_bubble_iter=150000, depth_weight=0.1, normal_weight=0.05, angular_weight=0.0,
                                          light_mask_weight=0.5), 60000, ("random", "random"), 0.37),
    ("all-on-B1", False, 0, 1, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, mask_weight=0.3, depth_weight=0.1,
                                    normal_weight=0.05, angular_weight=0.05), 10, ("all", "all"), 2.5),
    ("mask-only-B2", False, 0, 2, dict(eikonal_weight=0.0, smooth_weight=0.0, mask_weight=0.5, depth_weight=0.0, normal_weight=0.0,
                                       angular_weight=0.0), 10, ("random", "random"), 1.0),
    ("light-mask-B3", True, 0, 3, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, mask_weight=0.3, depth_weight=0.1,
                                       normal_weight=0.05, light_mask_weight=0.5), 10, ("all", "random"), 0.37),
    ("bubble-smooth-B203", False, 41, 203, dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=100, bubble_weight=0.5, min_bubble_iter=0,
                                                max_bubble_iter=150000, mask_weight=0.0, depth_weight=0.1, normal_weight=0.05,
                                                angular_weight=0.0), 160000, ("all", "random"), 1.0),
]


def _loss_pair(kw):
    from i2sdf_amd import I2SDFLoss
    fn = I2SDFLoss(**kw)
    lc = orc.LossCfg(**{k: v for k, v in kw.items() if k in orc.LossCfg.__dataclass_fields__})
    lc.smooth_iter = fn.smooth_iter
    return fn, lc


@pytest.mark.parametrize("case", _ORACLE_CASES, ids=[c[0] for c in _ORACLE_CASES])
def test_fused_render_loss_matches_oracle(case, wgrad_mode):
    """The default path (loss + render backward fused, i2sdf_render_loss_backward) against the fp64 oracle at identical depths and draws:
    loss terms to 1e-5, every parameter gradient to 1e-4, density.beta's gradient to 1e-4 on its own; and against the separate path
    (I2SDF_FUSED_RENDER_LOSS=0): terms to 2e-6, the flat gradient to 2e-6, beta to 1e-6.  Batches of 1, 2, 3 and 5 rays leave the last
    4-ray workgroup of render_loss_bwd_kernel partly empty (every workgroup counts the masks itself); the mask term's weight_sum seed is
    checked with rays on both sides of its clip(1e-3, 1 - 1e-3), where the seed is zero."""
    from i2sdf_amd import synthetic_conf
    from test_gpu_network import build
    name, light, n_pc, B, kw, step, masks, scale = case
    ocfg, sd, inp, gt, dr, z_all, z_eik = _given_depths_case(B, light, n_pc, masks, seed=5 + B)
    loss_fn, lc = _loss_pair(kw)
    ref_out, ref_l, ref_g, _ = memo(("fused-vs-oracle", name), lambda: _oracle_step(sd, ocfg, inp, gt, lc, dr, z_all, z_eik, step, scale))
    if name == "mask-angular-B203":
        w = ref_out["weight_sum"].reshape(-1)
        assert int(((w < 1e-3) | (w > 1 - 1e-3)).sum()) >= 5 and int(((w >= 1e-3) & (w <= 1 - 1e-3)).sum()) >= 5, "rays on both sides of the clip"
    net = build(synthetic_conf(light), sd, train=True)
    l_sep, g_sep, _, n_fast_sep = _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, step, scale, fused=False)
    l_fus, g_fus, _, n_fast = _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, step, scale, fused=True)
    assert n_fast == 1 and n_fast_sep == 0, "the plain step must take the fused fast path (and the separate one must not)"
    e_terms = _assert_terms(l_fus, ref_l, 1e-5, "fused vs fp64", floor=1e-6)
    e_grads = _assert_grads_match_oracle(g_fus, ref_g, "fused vs fp64")
    e_beta = assert_close(g_fus["density.beta"], ref_g["density.beta"], 1e-4, "grad density.beta, fused vs fp64")
    _assert_terms(l_fus, l_sep, 2e-6, "fused vs separate", floor=1e-6)
    e_sep = assert_close(_flat(g_fus), _flat(g_sep), 2e-6, "parameter gradients, fused vs separate")
    e_beta_sep = assert_close(g_fus["density.beta"], g_sep["density.beta"], 1e-6, "grad density.beta, fused vs separate")
    print(f"{name}: vs fp64 terms {e_terms:.2e} grads {e_grads:.2e} beta {e_beta:.2e}; vs separate grads {e_sep:.2e} beta {e_beta_sep:.2e}")


@pytest.mark.parametrize("empty", ["depth", "normal", "both"])
def test_fused_render_loss_with_empty_masks(empty, wgrad_mode):
    """An all-false depth / normal mask: the masked mean is 0/0.  The oracle (torch's boolean indexing) reports NaN for that term and for
    the total; both HIP paths must report NaN for the same terms.  The term's seeds are zero for every ray, so the parameter gradients are
    finite and equal the oracle's (1e-4) and each other's (2e-6)."""
    from i2sdf_amd import synthetic_conf
    from test_gpu_network import build
    masks = {"depth": ("none", "random"), "normal": ("random", "none"), "both": ("none", "none")}[empty]
    B = 7
    ocfg, sd, inp, gt, dr, z_all, z_eik = _given_depths_case(B, False, 0, masks, seed=31)
    kw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, mask_weight=0.3, depth_weight=0.1, normal_weight=0.05, angular_weight=0.05)
    loss_fn, lc = _loss_pair(kw)
    _, ref_l, ref_g, _ = memo(("empty masks", empty), lambda: _oracle_step(sd, ocfg, inp, gt, lc, dr, z_all, z_eik, 10, 0.37))
    assert torch.isnan(ref_l["loss"])
    net = build(synthetic_conf(False), sd, train=True)
    l_sep, g_sep, _, _ = _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, 10, 0.37, fused=False)
    l_fus, g_fus, _, _ = _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, 10, 0.37, fused=True)
    for k in _LOSS_KEYS:
        assert bool(torch.isnan(l_fus[k])) == bool(torch.isnan(ref_l[k])) == bool(torch.isnan(l_sep[k])), k
    assert torch.isnan(l_fus["depth_loss" if empty != "normal" else "normal_loss"])
    _assert_terms(l_fus, ref_l, 1e-5, "fused vs fp64", floor=1e-6)
    assert torch.isfinite(_flat(g_fus)).all() and torch.isfinite(_flat(g_sep)).all()
    _assert_grads_match_oracle(g_fus, ref_g, "fused vs fp64")
    assert_close(_flat(g_fus), _flat(g_sep), 2e-6, "parameter gradients, fused vs separate")


def test_fused_render_loss_large_batch(wgrad_mode):
    """B = 4096 rays (1024 workgroups of render_loss_bwd_kernel; each recounts both masks over all B rays, O(B^2) byte reads -- a known
    cost, not changed here).  Against the separate path only (the fp64 oracle at this size is slow): loss terms to 2e-6, the flat
    parameter gradient to 2e-6, beta to 1e-6, and the per-ray seeds d loss / d output of a fixed 32-ray subset to 1e-6."""
    import os
    from i2sdf_amd import I2SDFNetwork, I2SDFLoss, synthetic_conf
    from helpers import camera_inputs, make_gt
    conf = synthetic_conf(False)
    conf["use_normal"] = True
    torch.manual_seed(5)
    net = I2SDFNetwork(conf).cuda().train()
    with torch.no_grad():
        net.density.beta.fill_(0.05)
    B = 4096
    inp = {k: v.cuda() for k, v in camera_inputs(B, (0.0, 0.0, -2.0), seed=21).items()}
    gt = {k: v.cuda() for k, v in make_gt(B).items()}
    g = torch.Generator().manual_seed(4)
    gt["depth_mask"] = (torch.rand(B, generator=g) > 0.3).cuda()
    gt["normal_mask"] = (torch.rand(B, generator=g) > 0.6).cuda()
    gt["mask"] = (torch.rand(B, 1, generator=g) > 0.5).float().cuda()
    loss_fn = I2SDFLoss(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, mask_weight=0.3, depth_weight=0.1, normal_weight=0.05)
    eng = net._engine_for(torch.device("cuda:0"))
    draws = {k: v for k, v in eng.training_draws(B, 77, "cuda", net.scene_bounding_sphere).items() if v is not None}
    net.force_iters = 1
    rows = torch.randperm(B, generator=g)[:32].sort().values.cuda()
    names = ("rgb", "depth", "wsum", "normal", "grad_theta", "diff_norm", "surface", "lmask")
    res = {}
    for fused in (False, True):
        os.environ["I2SDF_FUSED_RENDER_LOSS"] = "1" if fused else "0"
        try:
            for p in net.parameters():
                p.grad = None
            out = net(inp, draws=draws)
            losses = loss_fn(out, gt, 10)
            # the seeds for an upstream gradient of 1: the fused path's placeholders / the separate loss's gradients, before backward
            seeds = out["rgb_values"]._i2sdf_render["pre"]["tok"] if fused else dict(zip(names, losses["loss"].grad_fn.grads))
            pick = {}
            for k in ("rgb", "depth", "wsum", "normal", "diff_norm"):
                pick[k] = seeds[k].reshape(B, -1)[rows].clone()
            pick["grad_theta"] = torch.cat([seeds["grad_theta"][rows], seeds["grad_theta"][B + rows]]).clone()
            losses["loss"].backward()
            res[fused] = ({k: v.detach().clone() for k, v in losses.items()}, torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone(),
                          net.density.beta.grad.clone(), pick)
        finally:
            os.environ.pop("I2SDF_FUSED_RENDER_LOSS", None)
    (l_sep, g_sep, b_sep, s_sep), (l_fus, g_fus, b_fus, s_fus) = res[False], res[True]
    for k in l_sep:
        assert_close(l_fus[k], l_sep[k], 2e-6, f"loss term {k}", floor=1e-6)
    e = assert_close(g_fus, g_sep, 2e-6, "parameter gradients, fused vs separate")
    eb = assert_close(b_fus, b_sep, 1e-6, "grad density.beta, fused vs separate")
    es = max(assert_close(s_fus[k], s_sep[k], 1e-6, f"seed d loss / d {k} (32 rays)", floor=1e-12) for k in s_sep)
    print(f"B={B}: fused vs separate grads {e:.2e}, beta {eb:.2e}, seeds {es:.2e}")


# ---- the autograd contract of the fused path: whatever happens to the outputs between the render and the loss, the result is plain torch's --
def _detach(k):
    return lambda o: o.__setitem__(k, o[k].detach())


def _hook(k, fn):
    return lambda o: o[k].register_hook(fn)


def _clamp_depth(o):
    o["depth_values"].clamp_(1.5, 2.5)


# Transformations that cut or remove the depth term's gradient leave implicit_network.lin6 gradients that fp32 evaluation reproduces
# to only 1.1e-4 - 1.9e-4 of fp64 (the same on the separate path, whose arithmetic does not involve the fused kernel); clamp_ of the depths
# is a step function of rays whose depth lies within rounding of a bound (1.5e-3).  Those cases are held to 2e-3 against fp64 -- a wrong
# path is off by 0.25 - 2.0 there -- and to 5e-6 against the separate path like every case.
_CONDITIONED = {"detach-depth_values", "detach-surface_sdf", "hook-clamp-depth_values", "late-hook-clamp-depth_values", "inplace-clamp-depth_values"}

_CONTRACT = [
    ("untouched", None, ()),
    ("detach-weight_sum", _detach("weight_sum"), ()),
    ("detach-depth_values", _detach("depth_values"), ()),
    ("detach-normal_values", _detach("normal_values"), ()),
    ("detach-grad_theta", _detach("grad_theta"), ()),
    ("detach-surface_sdf", _detach("surface_sdf"), ()),
    ("detach-light_mask", _detach("light_mask"), ()),
    ("hook-clamp-rgb_values", _hook("rgb_values", lambda g: g.clamp(-1e-3, 1e-3)), ()),
    ("hook-clamp-depth_values", _hook("depth_values", lambda g: g.clamp(-1e-3, 1e-3)), ()),
    ("hook-inplace-depth_values", _hook("depth_values", lambda g: g.mul_(0.5)), ()),
    ("inplace-clamp-depth_values", _clamp_depth, ()),
    ("retain_grad", None, ("rgb_values", "depth_values")),
    # registered after the loss call, before backward: the loss has already taken its fused path; its backward must notice
    ("late-hook-clamp-depth_values", ("late", _hook("depth_values", lambda g: g.clamp(-1e-3, 1e-3))), ()),
    ("late-hook-inplace-rgb_values", ("late", _hook("rgb_values", lambda g: g.mul_(0.5))), ()),
]


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("case", _CONTRACT, ids=[c[0] for c in _CONTRACT])
def test_fused_render_loss_autograd_contract(case, scale, wgrad_mode):
    """A transformation T of the outputs between net(...) and the loss -- a detached output, a gradient hook that clamps or edits in place,
    an in-place edit, retain_grad() -- with an upstream gradient of 1 and of 0.37.  The reference is the fp64 oracle with the same T (plain
    torch: detach / hooks / in-place ops mean the same there): parameter gradients to 1e-4, and the separate path to 5e-6.  The fused
    path hands autograd unscaled placeholder seeds only when nothing can observe or transform them (i2sdf_amd.loss.fast_path_refusal);
    `untouched` must still take that fast path, every other case must not.  Light head, bubble point cloud and a mask term are on, so
    that every detached output carries a seed."""
    from i2sdf_amd import synthetic_conf
    from test_gpu_network import build
    name, T, retain = case
    tol = 2e-3 if name in _CONDITIONED else 1e-4
    B, n_pc, step = 48, 17, 60000
    ocfg, sd, inp, gt, dr, z_all, z_eik = _given_depths_case(B, True, n_pc, ("random", "random"), seed=61)
    kw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, bubble_weight=0.5, min_bubble_iter=0, max_bubble_iter=None,
              mask_weight=0.3, depth_weight=0.1, normal_weight=0.05, angular_weight=0.05, light_mask_weight=0.5)
    loss_fn, lc = _loss_pair(kw)
    if name == "inplace-clamp-depth_values":
        d = memo(("contract", "untouched", 1.0), lambda: _oracle_step(sd, ocfg, inp, gt, lc, dr, z_all, z_eik, step, 1.0))[0]["depth_values"]
        assert bool((d < 1.5).any() or (d > 2.5).any()) and bool(((d > 1.5) & (d < 2.5)).any()), "the clamp must bind for some rays only"
    _, ref_l, ref_g, ref_r = memo(("contract", name, scale), lambda: _oracle_step(sd, ocfg, inp, gt, lc, dr, z_all, z_eik, step, scale, T, retain))
    net = build(synthetic_conf(True), sd, train=True)
    l_sep, g_sep, r_sep, _ = _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, step, scale, fused=False, T=T, retain=retain)
    l_fus, g_fus, r_fus, n_fast = _hip_step(net, inp, gt, dr, z_all, z_eik, loss_fn, step, scale, fused=True, T=T, retain=retain)
    es = assert_close(_flat(g_fus), _flat(g_sep), 5e-6, f"{name}, g={scale}: parameter gradients, fused vs separate")
    e = _assert_grads_match_oracle(g_fus, ref_g, f"{name}, g={scale}: fused vs fp64", tol)
    _assert_grads_match_oracle(g_sep, ref_g, f"{name}, g={scale}: separate vs fp64", tol)
    _assert_terms(l_fus, ref_l, 1e-5, f"{name}: fused vs fp64", floor=1e-6)
    for k in retain:
        assert_close(r_fus[k], r_sep[k], 1e-6, f"{k}.grad, fused vs separate")
        assert_close(r_fus[k], ref_r[k], 1e-5, f"{k}.grad, fused vs fp64")
    assert n_fast == (1 if name == "untouched" else 0), f"{name}: fast path taken {n_fast} times"
    print(f"{name}, g={scale}: fused vs fp64 grads {e:.2e}, vs separate {es:.2e}")


def test_fused_render_loss_leaves_no_reference_cycle(wgrad_mode):
    """With the cyclic garbage collector off, the fused path's prepared per-sample gradients (sbar, ...) are freed by loss.backward()
    itself: nothing of the render's state refers back to itself (eik_true captures neither `pre` nor the autograd context)."""
    import gc
    import weakref
    from i2sdf_amd import synthetic_conf
    from test_gpu_network import build, cuda
    B = 16
    ocfg, sd, inp, gt, dr, z_all, z_eik = _given_depths_case(B, False, 0, ("random", "random"), seed=71)
    loss_fn, _ = _loss_pair(dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05))
    net = build(synthetic_conf(False), sd, train=True)
    eng = net._engine_for("cuda:0")
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        c, d, n = eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
        out = net.render(cuda(inp), c, d, n, z_all.cuda(), z_eik.cuda(), draws={"eik_pts": dr.eik_pts.cuda(), "nbr_off": dr.nbr_off.cuda()})
        losses = loss_fn(out, cuda(gt), 10)
        pre = out["rgb_values"]._i2sdf_render["pre"]
        refs = {k: weakref.ref(pre[k]) for k in ("sbar", "nbar", "rgb_bar")}
        del pre
        losses["loss"].backward()
        alive = [k for k, r in refs.items() if r() is not None]
        assert not alive, f"still referenced after backward without a cyclic collection: {alive}"
    finally:
        if was:
            gc.enable()
