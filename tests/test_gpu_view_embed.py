"""GPU: the radiance net's view embedders `spherical_harmonics` and `fourier` (rendering_network.embed_type) in both kernel families and
both modes, forward and backward, against tests/embed_ref.py in fp64 (itself held to the reference by tests/test_embed_ref.py).  Bars are
the project's own: 2e-5 on forward values, 1e-4 on gradients.  Both weight-gradient modes (I2SDF_WGRAD_BF16X2, set here: tests/conftest.py
lists the dual-mode modules by name).  Sizes are those of tests/test_gpu_idr.py / tests/test_gpu_hdr.py.

The saved side row.  Spherical harmonics are held to 1e-6 of fp64, the bar of the positional encoding.  For Fourier features the bar is
max(1e-6, 2 d) with d the deviation of the reference's OWN fp32 row from its fp64 row on the same directions and B, computed here from
tests/golden/g22_embed_rows.npz (max-norm relative, d = 9.4e-7 / 1.1e-6 / 2.2e-6 for 1 / 5 / 12 channels, sigma 1): the reference forms
2 pi (v.B) in fp32, an argument of up to ~20 rad whose rounding alone is 1e-6.  Measured deviation of the kernels' rows from fp64 on an MI355X: see
test_rgb_forward's docstring."""
import os

import numpy as np
import pytest
import torch

import embed_ref as ER
from oracle import i2sdf_oracle as orc
from helpers import assert_close, camera_inputs, make_draws, make_gt, memo, rel_max, sd_from_npz, t

pytestmark = pytest.mark.gpu
TOL = 2e-5                   # the bar of the existing forward tests (tests/test_gpu_train_forward.py, tests/test_gpu_idr.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WGRAD_MODES = ["wgrad-bf16x2", "wgrad-bf16x3"]
CASES = {"plumbing": (lambda: orc.plumbing_cfg(False), {}), "synthetic": (lambda: orc.synthetic_cfg(False), {}),
         "synthetic_fp32": (lambda: orc.synthetic_cfg(False), {"bf16x3": False})}
# ("plumbing", 30, 10): 64 wide, fp32 MFMA, one partial workgroup behind two full ones; ("synthetic", 300, 7): 256 wide, 16-point waves, sixteen
# full workgroups and a partial one; parts = 4: the point ranges of I2SDF_OPT_PARTS; ("synthetic", 4750, 7, parts 0), 'nerf' only: more than one
# round of 256 workgroups with a partial last one, the smallest shape that reaches rgb_fwd_split_kernel
SIZES = [("plumbing", 30, 10, None), ("synthetic", 300, 7, None), ("synthetic", 300, 7, 4), ("synthetic_fp32", 300, 7, None)]
TAIL = ("synthetic", 4750, 7, 0)
# degree 1 and 1 channel are the narrowest rows (1 and 5 columns); degree 5 and 12 channels fill 25 and 27 of the 27 view columns
KINDS = [("nerf", k) for k in ("sh1", "sh4", "sh5", "ff1", "ff12")] + [("idr", k) for k in ("sh4", "ff5", "ff12")]
# |pre-activation| of a hidden ReLU unit of the radiance net below this in the fp64 reference: relu' there is 0 or 1 by rounding noise (the
# threshold of helpers.relu_flip_analysis).  The backward probes give such a point no weight (as tests/test_gpu_hdr.py does at the kink of an
# output relu).  Measured before this was done: the 2100-point cases hold 15 to 25 such units among their 2.1 million, and in 4 of 26 cases one
# or two of them had another mask in the library than in fp64 (pre-activations of 1e-8 to 1.2e-7), each moving its point's fbar row by 1e-2.
KINK = 1e-6


def _rows():
    return memo("g22 rows", lambda: np.load(os.path.join(GOLDEN, "g22_embed_rows.npz"), allow_pickle=False))


def _fixture_B(tag):
    """the Fourier matrices of the row fixture: the kernels' rows are judged on the B (and the directions) on which the reference's own fp32
    deviation was recorded"""
    return t(_rows()["B." + tag]) if tag.startswith("ff") else None


def _fourier_row_bar(tag):
    z = _rows()
    d = rel_max(t(z[tag]), t(z[tag + ".f64"]))
    return max(1e-6, 2 * d), d


def _dirs(B):
    """B unit view directions: the fixture's 256 (the six axis directions among them), repeated"""
    d = t(_rows()["dirs"])
    return d[torch.arange(B) % d.shape[0]].contiguous()


def _conf(which, emb, mode, **extra):
    from i2sdf_amd.config import plumbing_conf, synthetic_conf
    conf = ER.embed_conf(plumbing_conf(False) if which.startswith("plumbing") else synthetic_conf(False), emb, mode)
    conf.update(CASES[which][1])
    conf.update(extra)
    return conf


def _engine(conf, sd, parts=None, set_B=True):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.engine import RenderEngine
    eng = RenderEngine(NetConfig.from_conf(conf))
    if parts is not None:
        eng.set_parts(parts)
        assert eng.parts == (parts if parts >= 2 else 0) and eng.blocked_saves
    if ER.B_KEY in sd and set_B:
        eng.set_view_embed(sd[ER.B_KEY])
    eng.pack(eng.layout.flat_from_state_dict(sd).cuda())
    return eng


def _weights(ocfg, tag, mode, seed, scale=0.05):
    emb = ER.parse(tag)
    sd = ER.perturb_params(ER.init_params(ocfg, emb, mode, seed=seed), scale, seed=seed + 1)
    if emb.kind == "fourier":
        sd[ER.B_KEY] = _fixture_B(tag)
    return sd, ER.embed_of(sd, emb.kind, emb.n)


def dbl(sd):
    return {k: v.double() for k, v in sd.items()}


def dbl_emb(emb, dev=None):
    B = None if emb.B is None else (emb.B.double() if dev is None else emb.B.double().to(dev))
    return ER.Embed(emb.kind, emb.n, B)


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
def _fwd_case(which, B, n, mode, tag):
    def make():
        ocfg = CASES[which][0]()
        sd, emb = _weights(ocfg, tag, mode, 51)
        g = torch.Generator().manual_seed(2)
        M, F = B * n, ocfg.rgb.feature_size
        cam = torch.randn(B, 3, generator=g) * 0.3
        dirs = _dirs(B)
        z = torch.cat([torch.sort(torch.rand(B, n, generator=g) * 3.0, -1)[0], torch.full((B, 1), 4.0)], 1)
        pts = (cam.unsqueeze(1) + z[:, :n].unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
        nrm = torch.randn(M, 3, generator=g) * 0.8
        feat = torch.randn(M, F, generator=g) * 0.5
        dflat = dirs.unsqueeze(1).repeat(1, n, 1).reshape(-1, 3)
        idr = mode == "idr"
        e64 = dbl_emb(emb)
        a = (dbl(sd), ocfg.rgb, e64, dflat.double(), feat.double(), pts.double() if idr else None, nrm.double() if idr else None)
        ref = ER.rgb_forward(*a)
        r1 = ER.first_activation(*a)
        side = ER.side_row(e64, dflat.double(), pts.double() if idr else None, nrm.double() if idr else None)
        return ocfg, sd, emb, cam, dirs, z, pts, nrm, feat, ref, r1, side
    return memo(("embed fwd", which, B, n, mode, tag), make)


# (the tail size in 'nerf' mode only, once per kind of embedder: 'idr' mode has no split-K tail)
@pytest.mark.parametrize("which,B,n,parts,mode,tag", [s + k for s in SIZES for k in KINDS] + [TAIL + ("nerf", "sh4"), TAIL + ("nerf", "ff12")])
def test_rgb_forward(which, B, n, parts, mode, tag):
    """rgb and the first saved activation at 2e-5; the saved side row against fp64 (spherical harmonics at 1e-6, Fourier features at
    max(1e-6, 2 d), see the module docstring); its padding columns exactly 0.
    Measured on an MI355X, largest deviation of the saved E(v) columns from fp64 over all sizes (max-norm relative): spherical harmonics
    sh1 5.2e-8, sh4 1.2e-7, sh5 1.7e-7 (bar 1e-6); Fourier features ff1 7.6e-7 (bar 1.9e-6), ff5 7.3e-7 (bar 2.2e-6), ff12 1.4e-6
    (bar 4.3e-6) -- below the reference's own fp32 deviation d (9.4e-7 / 1.1e-6 / 2.2e-6): the phase v.B is one fp32 dot product in
    revolutions, reduced exactly (t - rint(t)) before the hardware sine and cosine."""
    ocfg, sd, emb, cam, dirs, z, pts, nrm, feat, ref, r1, side = _fwd_case(which, B, n, mode, tag)
    M, F = B * n, ocfg.rgb.feature_size
    eng = _engine(_conf(which, emb, mode), sd, parts)
    assert eng.idr == (mode == "idr") and eng.cfg.rgb.embed == emb.kind and eng.cfg.rgb.embed_n == emb.n
    Mp = eng.pad_rows(M)
    featp = torch.zeros(Mp, F)
    featp[:M] = feat
    if mode == "idr":
        rgb, rs, pev = eng.rgb_forward(dirs.cuda(), n, featp.cuda(), M, points=pts.cuda(), normals=nrm.cuda())
        # x from the rays (cam + z dir) as well
        fw = {"rays": (cam.cuda(), dirs.cuda(), z.cuda(), n), "n_ray_pts": M, "grad": nrm.cuda()}
        rgb2, _, _ = eng.rgb_forward(dirs.cuda(), n, featp.cuda(), M, save=False, fw=fw)
        assert_close(rgb2.cpu(), ref, TOL, "rgb (points from rays)")
    else:
        rgb, rs, pev = eng.rgb_forward(dirs.cuda(), n, featp.cuda(), M)
    err = assert_close(rgb.cpu(), ref, TOL, f"rgb ({mode}, {tag})")
    assert_close(eng.saved_pm("rs", rs, M)[0].cpu(), r1, TOL, "r_1")
    # the saved side row: E(v) or [x | E(v) | normal] in its first S columns, exact zeros behind them
    S, e, off = side.shape[1], emb.dim, (3 if mode == "idr" else 0)
    assert S == e + 2 * off and pev.shape == (Mp, 40 if mode == "idr" else 32)
    got = pev.cpu()[:M].double()
    if emb.kind == "fourier":
        bar, d = _fourier_row_bar(tag)
    else:
        bar, d = 1e-6, 0.0
    dev_e = rel_max(got[:, off:off + e], side[:, off:off + e])
    print(f"{which} {B}x{n} parts={parts} {mode} {tag}: rgb error {err:.2e}; saved E(v) deviates from fp64 by {dev_e:.2e} "
          f"(bar {bar:.1e}, the reference's own fp32 deviation {d:.1e})")
    assert dev_e <= bar, f"saved E(v): {dev_e:.3e} > {bar:.1e}"
    assert_close(got[:, :S], side, bar, "saved side row")
    if mode == "idr":
        assert_close(got[:, :3], side[:, :3], 1e-6, "saved points")
        assert torch.equal(got[:, 3 + e:S].float(), nrm), "saved normals, at column 3 + e"
    assert float(pev[:M, S:].abs().max()) == 0.0, "padding columns of the saved side row"
    if emb.kind == "fourier":
        assert torch.equal(got[:, off:off + 3].float(), dirs.repeat_interleave(n, 0)), "the raw direction in front of the sines"
    if parts is not None and parts >= 2:
        assert eng.blocked_points(1, M, Mp) == Mp
    if (which, B, n, parts) == TAIL:
        bulk = _assert_tail_cut(eng, M, Mp)
        assert_close(rgb.cpu()[bulk:], ref[bulk:], TOL, "rgb of the split-K tail")
        assert rel_max(got[bulk:, :e], side[bulk:, :e]) <= bar and float(pev[bulk:M, S:].abs().max()) == 0.0


# ---- 2. radiance backward ----------------------------------------------------------------------------------------------------------------
def _bwd_case(which, B, n, mode, tag, idx=None):
    """probe loss sum(rgb * cw) with the SDF net in front, fp64; `idx`: the points the loss weights (all of them when None)"""
    def make():
        ocfg = CASES[which][0]()
        sd, emb = _weights(ocfg, tag, mode, 13)
        g = torch.Generator().manual_seed(6)
        M = B * n
        x = (torch.rand(M, 3, generator=g) * 2 - 1)
        dirs = _dirs(B)
        cw = torch.randn(M, 3, generator=g)
        sel = torch.arange(M) if idx is None else idx
        keep = torch.zeros(M, 1)
        keep[sel] = 1
        cw = cw * keep
        idr = mode == "idr"
        params = {k: v.double().requires_grad_(True) for k, v in sd.items() if not k.startswith("light") and k not in ("density.beta", ER.B_KEY)}
        dflat = dirs.double()[sel // n]
        if idr:
            sdf, feat, grad = orc.sdf_outputs(params, ocfg.sdf, x.double()[sel], create_graph=True)
        else:
            feat, grad = orc.sdf_forward(params, ocfg.sdf, x.double()[sel])[:, 1:], None
        near = torch.zeros(len(sel), dtype=torch.bool)

        def record(a, l):
            near.logical_or_((a.detach().abs() < KINK).any(dim=1))
            return torch.relu(a)

        with orc.relu_hook(record):
            rgb = ER.rgb_forward(params, ocfg.rgb, dbl_emb(emb), dflat, feat, x.double()[sel] if idr else None, grad)
        cw[sel] = cw[sel] * (~near).float().unsqueeze(1)          # decided here, from the reference alone, before anything is launched
        zeroed = float(near.double().mean())
        loss = (rgb * cw.double()[sel]).sum()
        names = list(params)
        gr = torch.autograd.grad(loss, [feat] + ([grad] if idr else []) + [params[k] for k in names], allow_unused=True)
        k0 = 2 if idr else 1
        ref = {k: (v if v is not None else torch.zeros_like(params[k])) for k, v in zip(names, gr[k0:])}
        return ocfg, sd, emb, x, dirs, cw, rgb.detach(), gr[0], (gr[1] if idr else None), ref, zeroed
    return memo(("embed bwd", which, B, n, mode, tag, None if idx is None else int(idx.sum())), make)


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
    return rgb_h, fbar, nbar, eng.layout.state_dict_from_flat(gflat.cpu())


def _check_lin0_columns(got, ref, emb, mode):
    """the columns of lin0.weight_v by name: E(v) at [off, off + e), and in 'idr' mode the points at [0, 3) and the normals at their shifted
    position [3 + e, 6 + e); the features behind them"""
    g0, r0 = got["rendering_network.lin0.weight_v"], ref["rendering_network.lin0.weight_v"]
    scale = float(r0.abs().max())
    e, off = emb.dim, (3 if mode == "idr" else 0)
    S = e + 2 * off
    assert float(r0[:, off:off + e].abs().max()) > 1e-3 * scale
    assert float((g0[:, off:off + e] - r0[:, off:off + e]).abs().max()) <= 1e-4 * scale, "d W_0, E(v) columns"
    assert float((g0[:, S:] - r0[:, S:]).abs().max()) <= 1e-4 * scale, "d W_0, feature columns"
    if mode == "idr":
        assert float(r0[:, :3].abs().max()) > 1e-3 * scale and float(r0[:, S - 3:S].abs().max()) > 1e-3 * scale
        assert float((g0[:, :3] - r0[:, :3]).abs().max()) <= 1e-4 * scale, "d W_0, point columns"
        assert float((g0[:, S - 3:S] - r0[:, S - 3:S]).abs().max()) <= 1e-4 * scale, "d W_0, normal columns at 3 + e"


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("mode,tag", KINDS)
@pytest.mark.parametrize("which,B,n,parts", SIZES)
def test_rgb_backward_param_feature_and_normal_grads(which, B, n, parts, mode, tag, wgrad):
    """probe loss = sum(rgb * cw) with the SDF net in front, as tests/test_gpu_idr.py has it: fbar, nbar ('idr') and every parameter gradient
    at 1e-4 -- the backward kernels read the saved row and the transposed streams of the new column maps.  A point with a hidden ReLU unit
    within 1e-6 of zero in the fp64 reference carries no weight (KINK above; at most 2 % of the points)."""
    ocfg, sd, emb, x, dirs, cw, rgb_ref, fbar_ref, nbar_ref, ref, zeroed = _bwd_case(which, B, n, mode, tag)
    print(f"{which} {mode} {tag}: {zeroed * 100:.2f} % of the points have a ReLU unit within {KINK} of zero and carry no weight")
    assert zeroed <= 0.02
    M = B * n
    eng = _engine(_conf(which, emb, mode), sd, parts)
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    rgb_h, fbar, nbar, got = _run_backward(eng, flat, x, dirs, n, cw, M, mode == "idr")
    assert_close(rgb_h.cpu(), rgb_ref, TOL, "rgb")
    assert_close(fbar[:M].cpu(), fbar_ref, 1e-4, "fbar")
    if mode == "idr":
        assert_close(nbar.cpu(), nbar_ref, 1e-4, "nbar_rgb")
    assert set(ref) <= set(got)
    for k in ref:
        assert_close(got[k], ref[k], 1e-4, k)
    _check_lin0_columns(got, ref, emb, mode)
    assert float(ref["implicit_network.lin0.weight_v"].abs().max()) > 0


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("tag", ["sh4", "ff12"])
def test_rgb_backward_split_k_tail(tag, wgrad):
    """('synthetic', 4750, 7, parts 0), 'nerf': 256 full workgroups and a tail of 482 points whose forward rgb_fwd_split_kernel takes.  The
    probe loss weights the tail and a few bulk points, so the oracle differentiates just those (tests/test_gpu_backward.py)."""
    which, B, n, parts = TAIL
    M = B * n
    idx = torch.cat([torch.arange(0, 150), torch.arange(256 * 128 - 90, M)])
    ocfg, sd, emb, x, dirs, cw, rgb_ref, fbar_ref, _, ref, zeroed = _bwd_case(which, B, n, "nerf", tag, idx)
    assert zeroed <= 0.02
    eng = _engine(_conf(which, emb, "nerf"), sd, parts)
    bulk = _assert_tail_cut(eng, M, eng.pad_rows(M))
    assert bulk == 256 * 128 and int((idx >= bulk).sum()) == M - bulk and float(cw[bulk:].abs().max()) > 0
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    rgb_h, fbar, _, got = _run_backward(eng, flat, x, dirs, n, cw, M, False)
    assert_close(rgb_h.cpu()[idx], rgb_ref, TOL, "rgb")
    assert_close(fbar[:M].cpu()[idx], fbar_ref, 1e-4, "fbar")
    assert_close(fbar[bulk:M].cpu(), fbar_ref[idx >= bulk], 1e-4, "fbar of the split-K tail")
    for k in ref:
        assert_close(got[k], ref[k], 1e-4, k)
    _check_lin0_columns(got, ref, emb, "nerf")


# ---- 3. the recorded reference on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("mode,tag", [("nerf", "sh4"), ("nerf", "sh5"), ("nerf", "ff12"), ("idr", "sh4"), ("idr", "ff5")])
def test_recorded_reference_through_the_engine(mode, tag, wgrad):
    """tests/golden/g22_embed_<mode>_<kind>.npz: the reference's own radiance net (plumbing size) on 64 points -- rgb at 2e-5, the gradients
    of sum(rgb * rgb_bar) with respect to every radiance parameter, the features and ('idr') the normals at 1e-4.  The SDF net in front is
    any: the features are the fixture's, written over the SDF forward's before the radiance net reads them."""
    z = np.load(os.path.join(GOLDEN, f"g22_embed_{mode}_{tag}.npz"), allow_pickle=False)
    ocfg = orc.plumbing_cfg(False)
    emb = ER.parse(tag)
    sd = ER.init_params(ocfg, emb, mode, seed=1)
    sd.update(sd_from_npz(z))
    assert list(sd).index("rendering_network.lin0.bias") > list(sd).index("implicit_network.lin0.bias")
    eng = _engine(_conf("plumbing", emb, mode), sd)
    flat = eng.layout.flat_from_state_dict(sd).cuda()
    M = 64
    idr = mode == "idr"
    pts = t(z["points"]) if idr else torch.zeros(M, 3)
    fwd = eng.sdf_forward_grad(points=pts.cuda())
    fwd["feat"][:M] = t(z["feat"]).cuda()
    view, w = t(z["view_dirs"]).cuda(), t(z["rgb_bar"]).cuda()
    if idr:
        rgb, rs, pev = eng.rgb_forward(view, 1, fwd["feat"], M, points=pts.cuda(), normals=t(z["normals"]).cuda())
        nbar = torch.full((M, 3), float("nan"), device="cuda")
        gar, ga_last, fbar = eng.rgb_backward(rgb, w, rs, M, nbar=nbar, accumulate=False)
    else:
        rgb, rs, pev = eng.rgb_forward(view, 1, fwd["feat"], M)
        nbar = None
        gar, ga_last, fbar = eng.rgb_backward(rgb, w, rs, M)
    bw = eng.sdf_backward(fwd, sbar=None, fbar=fbar, m_fbar=M, nbar=nbar)
    gflat = torch.zeros_like(flat)
    eng.weight_grads(flat, gflat, fwd, bw, M_main=M, fbar=fbar, rgb_fw={"pev": pev, "rs": rs}, rgb_bw={"gar": gar, "ga_last": ga_last})
    got = eng.layout.state_dict_from_flat(gflat.cpu())
    assert_close(rgb.cpu(), t(z["rgb"]), TOL, "rgb")
    assert_close(fbar[:M].cpu(), t(z["fbar"]), 1e-4, "fbar")
    if idr:
        assert_close(nbar.cpu(), t(z["nbar"]), 1e-4, "nbar")
    names = [k[len("grad."):] for k in z.files if k.startswith("grad.")]
    assert len(names) == 9
    for k in names:
        assert_close(got[k], t(z["grad." + k]), 1e-4, k)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def _train_case(which, mode, tag):
    ocfg = CASES[which][0]()
    ocfg.use_normal = True
    sd, emb = _weights(ocfg, tag, mode, 41, scale=0.03)
    sd["density.beta"] = torch.tensor(0.05)
    B = 64
    inp = camera_inputs(B, (0.0, 0.0, -2.0), seed=5)
    gt = make_gt(B)
    dr = make_draws(ocfg, B, n_row=ocfg.sampler.N_samples_eval, seed=2)
    lkw = dict(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=None, depth_weight=0.1, normal_weight=0.05, angular_weight=0.05)

    def oracle():
        cam, dirs, _ = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
        z_all, z_eik = orc.sample_z_vals(sd, ocfg, dirs, cam, training=True, draws=dr, force_iters=1)
        D, dev = torch.float64, "cuda"            # the fp64 restatement as eager ops on the GPU (tests/test_gpu_network.py: _oracle_fp64_on_gpu)
        c = lambda v: (v.to(D) if v.dtype.is_floating_point else v).to(dev)
        d64 = orc.Draws(eik_pts=c(dr.eik_pts), nbr_off=c(dr.nbr_off))
        out, losses, grads = ER.training_step_grads({k: c(v) for k, v in sd.items()}, ocfg, dbl_emb(emb, dev), mode, {k: c(v) for k, v in inp.items()},
                                                    {k: c(v) for k, v in gt.items()}, orc.LossCfg(**lkw), d64, step=10,
                                                    z_override=(c(z_all), c(z_eik)))
        cpu = lambda x_: {k: v.detach().cpu() for k, v in x_.items() if torch.is_tensor(v)}
        return z_all, z_eik, cpu(out), cpu(losses), cpu(grads)

    return sd, emb, inp, gt, dr, lkw, memo(("embed train", which, mode, tag), oracle)


def _net(which, emb, mode, sd, train=True):
    from i2sdf_amd import I2SDFNetwork
    net = I2SDFNetwork(_conf(which, emb, mode, use_normal=True))
    net.load_state_dict(sd)
    net = net.cuda()
    return net.train() if train else net.eval()


def _step(which, emb, mode, sd, inp, gt, dr, lkw, z_all, z_eik):
    from i2sdf_amd import I2SDFLoss
    net = _net(which, emb, mode, sd)
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    eng = net._engine_for("cuda:0")
    c, d, nn = eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
    out = net.render(cu(inp), c, d, nn, z_all.cuda(), z_eik.cuda(), draws={"eik_pts": dr.eik_pts.cuda(), "nbr_off": dr.nbr_off.cuda()})
    losses = I2SDFLoss(**lkw)(out, cu(gt), 10)
    net.zero_grad()
    losses["loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for k, p in net.named_parameters()}
    node = out["rgb_values"].grad_fn              # the render core's autograd node keeps the saved radiance activations it used (relu(a) > 0: its masks)
    M_main = node.M_main
    masks = lambda: eng.saved_to_point_major(node.rs, eng.blocked_points(1, M_main, node.rs.shape[1]))[:, :M_main]
    return net, {k: v.detach() for k, v in out.items()}, losses["loss"].detach(), grads, masks


def _assert_grads_modulo_relu_flips(which, emb, mode, route, grads, ref_g, masks, sd, inp, gt, dr, lkw, z_all, z_eik):
    """tests/test_gpu_idr.py: _assert_grads_modulo_relu_flips, the same bars -- the difference must be a 0/1 combination of at most 4
    backward-mask flips of ReLU units whose pre-activation is zero within rounding (|pre-activation| < 1e-6) plus a residual inside 1e-4, the
    library's masks may differ from the restatement's only at such units, and every flip used must be one the library really has.  Only
    entered where the plain check misses."""
    from helpers import explain_by_relu_flips, hip_mask_flips, relu_flip_analysis
    ocfg = CASES[which][0]()
    ocfg.use_normal = True
    c = lambda v: (v.to(torch.float64) if v.dtype.is_floating_point else v).cuda()
    d64 = orc.Draws(eik_pts=c(dr.eik_pts), nbr_off=c(dr.nbr_off))
    run = lambda: ER.training_step_grads({k: c(v) for k, v in sd.items()}, ocfg, dbl_emb(emb, "cuda"), mode, {k: c(v) for k, v in inp.items()},
                                         {k: c(v) for k, v in gt.items()}, orc.LossCfg(**lkw), d64, step=10, z_override=(c(z_all), c(z_eik)))[2]
    _, cands, deltas = relu_flip_analysis(run, tau=1e-6)
    pre = relu_flip_analysis.pre
    scale = {k: float(ref_g[k].abs().max()) for k in ref_g}
    err = {k: grads[k].cpu().double().reshape(-1) - ref_g[k].double().reshape(-1) for k in ref_g}
    chosen, res = explain_by_relu_flips(err, [{k: d[k].detach().cpu().reshape(-1) for k in d} for d in deltas], scale)
    print(f"{which} {mode} {route}: {len(cands)} ReLU units with |pre-activation| < 1e-6; flips that explain the difference:",
          [(cands[i][0], cands[i][1], cands[i][2], "%.1e" % cands[i][3]) for i in chosen], "residual %.2e" % max(res.values()))
    assert len(chosen) <= 4 and max(res.values()) <= 1e-4, (chosen, {k: v for k, v in res.items() if v > 1e-4})
    flips, worst = hip_mask_flips(masks().cpu(), pre)
    assert worst < 1e-6, f"a backward mask differs at a unit whose pre-activation is {worst:.2e}: not a rounding-level flip"
    for i in chosen:
        assert (cands[i][0], cands[i][1], cands[i][2]) in flips, f"flip {cands[i]} explains the difference but the library's mask of that unit equals the restatement's"


@pytest.mark.parametrize("wgrad", WGRAD_MODES, indirect=True)
@pytest.mark.parametrize("tag", ["sh4", "ff12"])
@pytest.mark.parametrize("mode", ["nerf", "idr"])
@pytest.mark.parametrize("which", ["plumbing", "synthetic"])
def test_train_step_parity(which, mode, tag, wgrad, monkeypatch):
    """64 rays end to end against embed_ref.training_step_grads in fp64, depths and draws given, through the fused loss route and the
    separate one, at the bars of test_train_step_parity in tests/test_gpu_idr.py; then one FusedAdam step, which moves every parameter and
    leaves the Fourier matrix bit for bit what it was."""
    from i2sdf_amd import FusedAdam
    sd, emb, inp, gt, dr, lkw, (z_all, z_eik, ref_out, ref_loss, ref_g) = _train_case(which, mode, tag)
    assert float(ref_out["rgb_values"].abs().max()) > 1e-2 and float(ref_g["rendering_network.lin0.weight_v"][:, :emb.dim].abs().max()) > 0
    routes = {}
    for route, env in (("fused", "1"), ("separate", "0")):
        monkeypatch.setenv("I2SDF_FUSED_RENDER_LOSS", env)
        net, out, loss, grads, masks = _step(which, emb, mode, sd, inp, gt, dr, lkw, z_all, z_eik)
        assert set(grads) == set(ref_g) and ER.B_KEY not in grads
        for k in ("rgb_values", "depth_values", "weight_sum", "grad_theta"):
            assert_close(out[k].cpu(), ref_out[k], 1e-4, f"{k} ({route})")
        hit = ref_out["weight_sum"].reshape(-1) > 1e-2
        assert_close(out["normal_values"].cpu()[hit], ref_out["normal_values"][hit], 1e-4, f"normal_values ({route}, weight_sum > 0.01)")
        assert_close(loss.cpu(), ref_loss["loss"], 1e-5, f"loss ({route})")
        worst = max(rel_max(grads[k].cpu(), ref_g[k]) for k in grads)
        print(f"{which} {mode} {tag} {route}: worst relative parameter-gradient error {worst:.2e}")
        if worst > 1e-4:
            _assert_grads_modulo_relu_flips(which, emb, mode, route, grads, ref_g, masks, sd, inp, gt, dr, lkw, z_all, z_eik)
        for k in grads:
            assert grads[k].shape == ref_g[k].shape and bool(torch.isfinite(grads[k]).all()), k
        routes[route] = (loss, grads)
    assert_close(routes["separate"][0].cpu(), routes["fused"][0].cpu(), 1e-6, "loss, separate vs fused route")
    for k in routes["fused"][1]:
        assert_close(routes["separate"][1][k].cpu(), routes["fused"][1][k].cpu(), 1e-6, f"grad {k}, separate vs fused route")
    # one optimizer step on the last net: the buffer is no parameter
    opt = FusedAdam(net.parameters(), lr=1e-3)
    assert all(p is not getattr(net.rendering_network.embedview_fn, "B", None) for g_ in opt.param_groups for p in g_["params"])
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt.step()
    torch.cuda.synchronize()
    after = net.state_dict()
    assert not torch.equal(after["rendering_network.lin0.weight_v"], before["rendering_network.lin0.weight_v"])
    if emb.kind == "fourier":
        assert torch.equal(after[ER.B_KEY], before[ER.B_KEY]) and torch.equal(after[ER.B_KEY].cpu(), sd[ER.B_KEY])
        assert torch.equal(net._engine_for("cuda:0").view_embed_B, sd[ER.B_KEY])
    else:
        assert ER.B_KEY not in after


@pytest.mark.parametrize("mode,tag", [("nerf", "sh4"), ("nerf", "ff12"), ("idr", "sh4"), ("idr", "ff12")])
def test_eval_render_of_a_small_view(mode, tag):
    """a 12 x 16 view of the plumbing net in eval mode: render_image equals the chunked forward bit for bit, evaluate_views and render_path
    run on it, and the render is the embedder's -- with depths given it agrees with embed_ref in fp64 at 1e-4"""
    from i2sdf_amd import views as V
    ocfg = orc.plumbing_cfg(False)
    ocfg.use_normal = True
    sd, emb = _weights(ocfg, tag, mode, 41, scale=0.03)
    sd["density.beta"] = torch.tensor(0.05)
    net = _net("plumbing", emb, mode, sd, train=False)
    H, W = 12, 16
    P = H * W
    inp = {k: v.cuda() for k, v in camera_inputs(P, (0.0, 0.1, -2.0), W=W, H=H, f=14.0, seed=4, train_layout=False).items()}
    full = net.render_image(inp, split_n_pixels=80)
    parts = []
    with torch.no_grad():
        for lo in range(0, P, 80):
            d = dict(inp)
            d["uv"] = inp["uv"][:, lo:lo + 80].contiguous()
            parts.append(net(d))
    for k in full:
        assert torch.equal(full[k].reshape(P, -1), torch.cat([p[k] for p in parts], 0).reshape(P, -1)), k
    assert float(full["rgb_values"].std()) > 1e-4
    # the depths the library chose, through the fp64 restatement
    eng = net._engine_for("cuda:0")
    c, d_, nn = eng.ray_setup(inp["uv"], inp["pose"], inp["intrinsics"])
    with torch.no_grad():
        z_all, z_eik, _ = eng.sample_rays(net._flat, c, d_, training=False)
        out = net.render(inp, c, d_, nn, z_all, z_eik)
    c64 = lambda v: (v.double() if v.dtype.is_floating_point else v)
    ref = ER.network_forward({k: c64(v).cuda() for k, v in sd.items()}, ocfg, dbl_emb(emb, "cuda"), mode, {k: c64(v) for k, v in inp.items()}, False,
                             z_override=(z_all.double(), z_eik.double() if z_eik is not None else None))
    for k in ("rgb_values", "depth_values", "weight_sum"):
        assert_close(out[k].cpu().reshape(ref[k].shape), ref[k].detach().cpu(), 1e-4, k)
    # the view routines on top of render_image
    poses = inp["pose"][:1].repeat(2, 1, 1)
    poses[1, 0, 3] += 0.05
    K = inp["intrinsics"][0]
    res = net.evaluate_views(poses, K, (H, W), gt_rgb=torch.rand(2, P, 3, device="cuda"), split_n_pixels=80)
    one = net.render_image({"uv": V.pixel_grid(H, W, "cuda"), "pose": poses[:1], "intrinsics": K[None]}, 80)
    assert torch.equal(res["rgb_values"][0], one["rgb_values"].reshape(P, 3)) and bool(torch.isfinite(res["psnr"]).all())
    assert float(res["rgb_values"].std()) > 1e-4
    path = net.render_path(poses[0], poses[1], K, (H, W), num_frames=3, split_n_pixels=80)
    assert tuple(path["rgb8"].shape) == (3, H, W, 3) and float(path["rgb8"].float().std()) > 0


@pytest.mark.parametrize("mode,tag", [("nerf", "ff12"), ("idr", "ff5"), ("nerf", "sh5")])
def test_fixture_checkpoint_loads_and_renders_the_fixtures_rgb(mode, tag):
    """load_state_dict with the reference's recorded radiance checkpoint on a module that has ALREADY built its engine with another B: the
    plan gets the loaded matrix, and the radiance net renders the fixture's rgb"""
    from i2sdf_amd import I2SDFNetwork
    z = np.load(os.path.join(GOLDEN, f"g22_embed_{mode}_{tag}.npz"), allow_pickle=False)
    emb = ER.parse(tag)
    net = I2SDFNetwork(_conf("plumbing", emb, mode)).cuda().eval()
    eng = net._engine_for("cuda:0")                              # built with the matrix drawn at construction
    if emb.kind == "fourier":
        assert torch.equal(eng.view_embed_B, net.rendering_network.embedview_fn.B.cpu())
    full = dict(net.state_dict())
    full.update({k: v.cuda() for k, v in sd_from_npz(z).items()})
    net.load_state_dict(full)
    if emb.kind == "fourier":
        assert torch.equal(eng.view_embed_B, t(z["sd." + ER.B_KEY])) and not torch.equal(eng.view_embed_B, torch.zeros(3, emb.n))
    eng = net._engine_for("cuda:0")                              # repacks the loaded weights
    M, F = 64, 64
    featp = torch.zeros(eng.pad_rows(M), F, device="cuda")
    featp[:M] = t(z["feat"]).cuda()
    kw = dict(points=t(z["points"]).cuda(), normals=t(z["normals"]).cuda()) if mode == "idr" else {}
    rgb, _, _ = eng.rgb_forward(t(z["view_dirs"]).cuda(), 1, featp, M, save=False, **kw)
    assert_close(rgb.cpu(), t(z["rgb"]), TOL, "rgb of the loaded checkpoint")


# ---- 5. refusal ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,mode", [("plumbing", "nerf"), ("synthetic", "nerf"), ("synthetic", "idr")])
def test_fourier_forward_without_the_matrix_is_refused_and_launches_nothing(which, mode):
    from i2sdf_amd.lib import I2SDFError
    ocfg = CASES[which][0]()
    sd, emb = _weights(ocfg, "ff12", mode, 3)
    eng = _engine(_conf(which, emb, mode), sd, set_B=False)
    B, n = 20, 7
    M, F = B * n, ocfg.rgb.feature_size
    Mp = eng.pad_rows(M)
    feat = torch.randn(Mp, F, device="cuda")
    kw = dict(points=torch.randn(M, 3, device="cuda"), normals=torch.randn(M, 3, device="cuda")) if mode == "idr" else {}
    # the raw entry point with buffers of this test's own, filled with a sentinel: refused, and after a synchronisation nothing was written
    from i2sdf_amd import lib as L
    h = L.load()
    rgb = torch.full((M, 3), -7.0, device="cuda")
    rs = torch.full((ocfg.rgb.n_lin - 1, Mp, ocfg.rgb.dims[0]), -7.0, device="cuda")
    pev = torch.full((Mp, 40 if mode == "idr" else 32), -7.0, device="cuda")
    dirs = _dirs(B).cuda()
    torch.cuda.synchronize()
    if mode == "idr":
        rc = h.i2sdf_rgb_forward_idr(eng._plan, eng._pk(), L.ptr(kw["points"]), None, L.ptr(dirs), None, 0, n, L.ptr(kw["normals"]), L.ptr(feat), M, Mp,
                                     L.ptr(rgb), L.ptr(rs), L.ptr(pev), L.stream_ptr())
    else:
        rc = h.i2sdf_rgb_forward(eng._plan, eng._pk(), L.ptr(dirs), n, L.ptr(feat), M, Mp, L.ptr(rgb), L.ptr(rs), L.ptr(pev), L.stream_ptr())
    assert rc == -1 and "i2sdf_plan_set_view_embed" in h.i2sdf_last_hip_error().decode()
    torch.cuda.synchronize()
    assert bool((rgb == -7.0).all()) and bool((rs == -7.0).all()) and bool((pev == -7.0).all())
    # the module's driver says why
    with pytest.raises(I2SDFError, match=r"\(-1\).*Fourier view embedder has no matrix B yet \(i2sdf_plan_set_view_embed\)"):
        eng.rgb_forward(dirs, n, feat, M, **kw)
    # with the matrix set the same call runs, and the saved row carries E(v)
    eng.set_view_embed(sd[ER.B_KEY])
    rgb2, rs2, pev2 = eng.rgb_forward(dirs, n, feat, M, **kw)
    assert bool(torch.isfinite(rgb2).all()) and float(pev2[:M].abs().max()) > 0
