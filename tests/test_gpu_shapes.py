"""GPU: every kind of network shape `NetConfig.from_conf` accepts, against the fp64 oracle (tests/shapes_ref.py: the twelve cases).

Depth and skip position choose between the bf16x3 kernels (blocked saves, 24-bit records) and the fp32 256-wide full-workgroup
kernels (point-major saves), separately for the SDF and the radiance net; the rest of the suite runs four shapes, all of them on
the same side of every such condition.  The bars are the project's own for the same quantities -- 2e-5 for outputs and saved
activations (tests/test_gpu_train_forward.py), 1e-4 for parameter gradients (tests/test_gpu_backward.py) -- and
tests/test_shape_frontier.py::test_oracle_fp32_is_well_inside_the_bars shows that the inputs leave the oracle's own fp32-vs-fp64
difference at most a quarter of them.  M = 333 points: three 128-point workgroups, the last one ragged; 37 rays of 9 points.

Every figure is printed (`shape_sweep: ...`) before it is asserted; profiles/shape_sweep.txt is such a run's output."""
import pytest
import torch

import shapes_ref as S
from oracle import i2sdf_oracle as orc
from helpers import rel_max, memo, camera_inputs, make_draws, make_gt
from test_gpu_train_forward import make_engine, dbl

pytestmark = pytest.mark.gpu
CASE_IDS = [c.id for c in S.CASES]
MODES = ["wgrad-bf16x2", "wgrad-bf16x3"]


def _set_mode(monkeypatch, mode):
    """tests/conftest.py runs its list of modules once per weight-gradient mode; this module sets the mode itself, before the engine
    is built (the engine reads the variable in its constructor)"""
    monkeypatch.setenv("I2SDF_WGRAD_BF16X2", "1" if mode == "wgrad-bf16x2" else "0")


class _Sweep:
    """compares like helpers.assert_close, but prints the worst figure of a group of quantities before the first failure is raised"""

    def __init__(self, cid, test, mode="-"):
        self.head, self.rows = f"shape_sweep: {cid} {test} {mode}", []

    def add(self, what, got, ref, tol):
        got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
        assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
        finite = bool(torch.isfinite(got.double()).all())
        err = (rel_max(got, ref) if float(ref.abs().max()) > 0 else float(got.double().abs().max())) if finite else float("inf")
        self.rows.append((what, err, tol))

    def done(self):
        for kind, tol in (("outputs", S.TOL_OUT), ("gradients", S.TOL_GRAD)):
            rows = [r for r in self.rows if r[2] == tol]
            if rows:
                w = max(rows, key=lambda r: r[1])
                print(f"{self.head} worst {kind} {w[1]:.2e} ({w[0]}) bar {tol:.0e}")
        bad = [f"{w}: max-norm relative error {e:.3e} > {t:.1e}" for w, e, t in self.rows if not e <= t]
        assert not bad, "; ".join(bad)


def _setup(cid):
    case = S.BY_ID[cid]
    ocfg, sd = S.case_weights(case)
    return case, ocfg, sd, S.case_inputs(case), S.reference(case)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_sdf_only_forward(cid):
    """the kernel family the sampler and the tracer run, with the depth and the skip layer as run-time arguments"""
    case, ocfg, sd, inp, ref = _setup(cid)
    eng = make_engine(S.case_conf(case), sd)
    x = inp["x"].cuda()
    sw = _Sweep(cid, "sdf_forward")
    sw.add("sdf (sdf only)", eng.sdf_forward(x), ref["sdf"], S.TOL_OUT)
    sdf, feat = eng.sdf_forward(x, want_features=True)
    sw.add("sdf", sdf, ref["sdf"], S.TOL_OUT)
    sw.add("feature", feat, ref["feat"], S.TOL_OUT)
    sw.done()


@pytest.mark.parametrize("cid", CASE_IDS)
def test_training_forward_and_saves(cid):
    """tests/test_gpu_train_forward.py::test_sdf_forward_grad_and_saves at the new shapes: sdf, feature, d sdf/dx and every layer's
    saved h_l and abar_l in whatever layout the shape's kernels store them"""
    case, ocfg, sd, inp, ref = _setup(cid)
    eng = make_engine(S.case_conf(case), sd)
    M = S.M
    out = eng.sdf_forward_grad(points=inp["x"].cuda())
    sw = _Sweep(cid, "sdf_forward_grad")
    sw.add("sdf", out["sdf"], ref["sdf"], S.TOL_OUT)
    sw.add("feature", out["feat"][:M], ref["feat"], S.TOL_OUT)
    sw.add("d sdf/dx", out["grad"], ref["grad"], S.TOL_OUT)
    hs_pm, ab_pm = eng.saved_to_point_major(out["hs"], out["blk"]), eng.saved_pm("abars", out["abars"], M)
    for l in range(ocfg.sdf.n_lin - 1):
        w = ref[f"h_{l + 1}"].shape[1]
        sw.add(f"h_{l + 1}", hs_pm[l, :M, :w], ref[f"h_{l + 1}"], S.TOL_OUT)
        sw.add(f"abar_{l}", ab_pm[l, :M, :w], ref[f"abar_{l}"], S.TOL_OUT)
    sw.done()
    # the layout follows the kernel choice: blocked exactly where the SDF net is on the bf16x3 path
    x3 = case.width == 256 and ocfg.sdf.n_lin >= 4 and (case.skip_in[0] if case.skip_in else -1) != ocfg.sdf.n_lin - 2
    assert (out["blk"] > 0) == x3, (out["blk"], x3)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_radiance_forward(cid):
    case, ocfg, sd, inp, ref = _setup(cid)
    eng = make_engine(S.case_conf(case), sd)
    M, F = S.M, case.width
    featp = torch.zeros(eng.pad_rows(M), F)
    featp[:M] = ref["feat"].float()
    rgb, rs, _ = eng.rgb_forward(inp["dirs"].cuda(), S.N_PER_RAY, featp.cuda(), M)
    sw = _Sweep(cid, "rgb_forward")
    sw.add("rgb", rgb, ref["rgb"], S.TOL_OUT)
    sw.done()
    assert (eng.blocked_points(1, M, eng.pad_rows(M)) > 0) == (case.width == 256 and ocfg.rgb.n_lin >= 3)


def _backward(case, ocfg, sd, inp, eng):
    """the probe loss of shapes_ref.oracle_run through the library: -> ({parameter: gradient}, rgb, lm or None)"""
    M, m_f, n = S.M, inp["m_f"], S.N_PER_RAY
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    fwd = eng.sdf_forward_grad(points=inp["x"].cuda())
    rgb, rs, pev = eng.rgb_forward(inp["dirs"].cuda(), n, fwd["feat"], M)
    gar, ga_last, fbar = eng.rgb_backward(rgb, inp["cw"].cuda(), rs, M)
    fbar[:M] += inp["fw"].cuda()                        # d loss / d feature: the radiance net's share + the probe's own (rows >= m_f: zero)
    lm = light = None
    if case.light:
        lm, hl = eng.light_forward(fwd["feat"], m_f)
        gal0, gal_last = eng.light_backward(lm, inp["lw"][:m_f].reshape(-1).cuda(), hl, m_f)
        light = {"hl": hl, "gal0": gal0, "gal_last": gal_last}
    nvec = fwd["grad"]
    nn = nvec.norm(dim=1, keepdim=True)
    nbar = 2 * (nn - 1) * nvec / nn
    bw = eng.sdf_backward(fwd, sbar=inp["sw"].reshape(-1).cuda(), fbar=fbar, m_fbar=m_f, nbar=nbar)
    gflat = torch.zeros_like(flat)
    eng.weight_grads(flat, gflat, fwd, bw, M_main=m_f, fbar=fbar, rgb_fw={"pev": pev, "rs": rs}, rgb_bw={"gar": gar, "ga_last": ga_last}, light=light)
    return eng.layout.state_dict_from_flat(gflat.cpu()), rgb, lm


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_backward_param_grads(cid, mode, monkeypatch):
    """sum(sdf sw) + sum(feat fw) + sum((|grad| - 1)^2) + sum(rgb cw) [+ sum(lm lw)], the last 37 points without feature gradient:
    s-bar, f-bar, the double backward and the radiance backward; every parameter gradient of every net"""
    _set_mode(monkeypatch, mode)
    case, ocfg, sd, inp, ref = _setup(cid)
    eng = make_engine(S.case_conf(case), sd)
    assert eng.wgrad_bf16x2 == (mode == "wgrad-bf16x2")
    got, rgb, _ = _backward(case, ocfg, sd, inp, eng)
    sw = _Sweep(cid, "backward", mode)
    sw.add("rgb", rgb, ref["rgb"], S.TOL_OUT)
    names = [k[5:] for k in ref if k.startswith("grad.")]
    assert sorted(names) == sorted(k for k in got if k != "density.beta")
    for k in names:
        sw.add(k, got[k], ref["grad." + k], S.TOL_GRAD)
    sw.done()


@pytest.mark.parametrize("cid", S.LIGHT_CASES)
def test_light_head(cid):
    case, ocfg, sd, inp, ref = _setup(cid)
    eng = make_engine(S.case_conf(case), sd)
    got, _, lm = _backward(case, ocfg, sd, inp, eng)
    sw = _Sweep(cid, "light_head")
    sw.add("light mask", lm, ref["lm"], S.TOL_OUT)
    for k in ref:
        if k.startswith("grad.light_network"):
            sw.add(k[5:], got[k[5:]], ref[k], S.TOL_GRAD)
    sw.done()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("parts", [0, 4])
def test_backward_split_k_tail_at_a_fallback_shape(parts, mode, monkeypatch):
    """tests/test_gpu_backward.py::test_backward_split_k_tail for case 2, whose SDF net runs the fp32 256-wide full workgroups as its
    default path: 256 of them and a short tail.  parts = 0: the tail of every kernel as split-K workgroups; parts = 4: the radiance net
    (bf16x3) in four point ranges beside the whole-batch SDF kernels.  The oracle differentiates only the tail and the first 150 points."""
    _set_mode(monkeypatch, mode)
    case = S.BY_ID["c02_w256_s2k1_r2_l128"]
    conf = S.case_conf(case)
    ocfg = orc.NetCfg.from_conf(conf)
    sd = orc.perturb_params(orc.init_params(ocfg, seed=21), 0.05, seed=22)
    eng = make_engine(conf, sd, parts=parts)
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    g = torch.Generator().manual_seed(23)
    n = 7
    B = (256 * 128 + 500 + n - 1) // n
    M = B * n
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * 1.5
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
    idx = torch.cat([torch.arange(0, 150), torch.arange(256 * 128 - 90, M)])
    sel = torch.zeros(M, 1)
    sel[idx] = 1
    cw = torch.randn(M, 3, generator=g) * sel
    sw_ = torch.randn(M, 1, generator=g) * sel
    m_f = M - 29

    def oracle():
        params = {k: v.double().requires_grad_(True) for k, v in sd.items() if not k.startswith("light") and k != "density.beta"}
        sdf, feat, grad = orc.sdf_outputs(params, ocfg.sdf, x.double()[idx], create_graph=True)
        with_rgb = (idx < m_f).double().unsqueeze(1)
        rgb = orc.rgb_forward(params, ocfg.rgb, dirs.double()[idx // n], feat)
        loss = (rgb * cw.double()[idx] * with_rgb).sum() + (sdf * sw_.double()[idx]).sum() + ((grad.norm(2, dim=1) - 1) ** 2).sum()
        names = list(params)
        gr = torch.autograd.grad(loss, [params[k] for k in names], allow_unused=True)
        return {k: (v if v is not None else torch.zeros_like(params[k])).detach() for k, v in zip(names, gr)}

    ref = memo(("shape frontier split-K, case 2",), oracle)
    fwd = eng.sdf_forward_grad(points=x.cuda())
    assert fwd["blk"] == 0, "the fp32 SDF path saves point-major rows"
    rgb_h, rs, pev = eng.rgb_forward(dirs.cuda(), n, fwd["feat"], M)
    cw_d = cw.clone()
    cw_d[m_f:] = 0
    gar, ga_last, fbar = eng.rgb_backward(rgb_h, cw_d.cuda(), rs, M)
    nvec = fwd["grad"]
    nn = nvec.norm(dim=1, keepdim=True)
    nbar = 2 * (nn - 1) * nvec / nn * sel.cuda()
    bw = eng.sdf_backward(fwd, sbar=sw_.reshape(-1).cuda(), fbar=fbar, m_fbar=m_f, nbar=nbar)
    gflat = torch.zeros_like(flat)
    eng.weight_grads(flat, gflat, fwd, bw, M_main=m_f, fbar=fbar, rgb_fw={"pev": pev, "rs": rs}, rgb_bw={"gar": gar, "ga_last": ga_last})
    got = eng.layout.state_dict_from_flat(gflat.cpu())
    sw = _Sweep(case.id, f"split_k_tail_parts{parts}", mode)
    for k in ref:
        sw.add(k, got[k], ref[k], S.TOL_GRAD)
    sw.done()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", ["c04_w256_s3_r1", "c11_w64_s11k10_r11"])
def test_train_step_given_depths(cid, mode, monkeypatch):
    """tests/test_gpu_network.py::test_train_step_given_depths_full_size at two of the shapes: identical depths and draws on both
    sides, outputs to 1e-4, the loss to 1e-5, every parameter gradient to 1e-4 (fp64 oracle).  Case 4 is the mixed-layout step: blocked
    SDF saves beside an fp32 point-major radiance net (the engine turns the point ranges, and with them the 24-bit records, off when one
    net is not on the bf16x3 path: engine.py, _sync_parts)."""
    from i2sdf_amd import I2SDFLoss
    from test_gpu_network import build, cuda
    _set_mode(monkeypatch, mode)
    conf = S.case_conf(S.BY_ID[cid])
    ocfg = orc.NetCfg.from_conf(conf)
    ocfg.use_normal = True
    sd = orc.perturb_params(orc.init_params(ocfg, seed=41), 0.03, seed=42)
    sd["density.beta"] = torch.tensor(0.05)
    B = 40
    inp = camera_inputs(B, (0.0, 0.0, -2.0), seed=5)
    gt = make_gt(B)
    dr = make_draws(ocfg, B, n_row=ocfg.sampler.N_samples_eval, seed=2)
    cam, dirs, dn = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
    z_all, z_eik = orc.sample_z_vals(sd, ocfg, dirs, cam, training=True, draws=dr, force_iters=1)
    weights = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05)
    D = torch.float64

    def oracle():
        d64 = orc.Draws(eik_pts=dr.eik_pts.to(D), nbr_off=dr.nbr_off.to(D))
        gt64 = {k: (v.to(D) if v.dtype.is_floating_point else v) for k, v in gt.items()}
        return orc.training_step_grads(dbl(sd), ocfg, {k: v.to(D) for k, v in inp.items()}, gt64, orc.LossCfg(**weights), d64, step=10,
                                       z_override=(z_all.to(D), z_eik.to(D)))

    ref_out, ref_loss, ref_g = memo(("shape frontier training step", cid), oracle)
    net = build(conf, sd, train=True)
    eng = net._engine_for("cuda:0")
    assert eng.wgrad_bf16x2 == (mode == "wgrad-bf16x2")
    c, d, n = eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
    out = net.render(cuda(inp), c, d, n, z_all.cuda(), z_eik.cuda(), draws={"eik_pts": dr.eik_pts.cuda(), "nbr_off": dr.nbr_off.cuda()})
    losses = I2SDFLoss(**weights)(out, cuda(gt), 10)
    net.zero_grad()
    losses["loss"].backward()
    errs = {k: rel_max(out[k].detach().cpu(), ref_out[k]) for k in ("rgb_values", "depth_values", "weight_sum", "grad_theta")}
    hit = ref_out["weight_sum"].reshape(-1) > 1e-2
    errs["normal_values"] = rel_max(out["normal_values"].detach().cpu()[hit], ref_out["normal_values"][hit])
    e_loss = rel_max(losses["loss"].detach().cpu(), ref_loss["loss"])
    e_g = {n_: rel_max((p.grad if p.grad is not None else torch.zeros_like(p)).cpu(), ref_g[n_]) if float(ref_g[n_].abs().max()) > 0
           else float(p.grad.abs().max()) if p.grad is not None else 0.0 for n_, p in net.named_parameters()}
    wo, wg = max(errs.items(), key=lambda kv: kv[1]), max(e_g.items(), key=lambda kv: kv[1])
    print(f"shape_sweep: {cid} train_step {mode} worst output {wo[1]:.2e} ({wo[0]}) bar 1e-04; loss {e_loss:.2e} bar 1e-05; "
          f"worst gradient {wg[1]:.2e} ({wg[0]}) bar 1e-04")
    for k, e in errs.items():
        assert e <= 1e-4, f"{k}: {e:.3e}"
    assert e_loss <= 1e-5, f"loss: {e_loss:.3e}"
    for k, e in e_g.items():
        assert e <= 1e-4, f"grad {k}: {e:.3e}"


@pytest.mark.parametrize("which", ["light-head-without-kernels", "skip-on-the-output-layer"])
def test_unrunnable_shapes_are_refused_before_any_launch(which):
    """two confs the grid of tests/test_shape_frontier.py refuses: the module and the engine raise with the reason when they are built,
    from the conf (NotImplementedError naming key and value) and from the plan (the C API's own reason text)"""
    from i2sdf_amd import I2SDFNetwork
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.engine import RenderEngine
    from i2sdf_amd.lib import I2SDFError
    if which.startswith("light"):
        conf, key, value, c_reason = S.make_conf(256, 8, [4], 4, [64]), "light_network.dims", "[64]", "light.hidden 64"
    else:
        conf, key, value, c_reason = S.make_conf(256, 8, [8], 4, None), "implicit_network.skip_in", "[8]", "sdf.skip_layer 8"
    for ctor in (I2SDFNetwork, lambda c: RenderEngine(NetConfig.from_conf(c))):
        with pytest.raises(NotImplementedError) as e:
            ctor(conf)
        assert key in str(e.value) and value in str(e.value), str(e.value)
    with pytest.raises(I2SDFError) as e:
        RenderEngine(S.unchecked_cfg(conf))
    assert "i2sdf_plan_create" in str(e.value) and c_reason in str(e.value), str(e.value)
