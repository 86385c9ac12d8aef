"""CPU: the radiance net's view embedders `spherical_harmonics` and `fourier` (rendering_network.embed_type).  tests/embed_ref.py, the
plain-torch restatement the GPU tests compare with, against the numbers the reference recorded (tests/golden/g22_embed_*.npz,
tests/golden/gen_golden_embed.py) and, where it can be imported, against the live reference; and the host side: the configuration is read
and refuses what it must, the module's state_dict is the reference's, the descriptor carries the embedder, the plan accepts and refuses,
the new entry point is declared, exported, bound and validates its arguments."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import embed_ref as ER
from oracle import i2sdf_oracle as orc
from helpers import assert_close, sd_from_npz, t as tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NETS = [("nerf", "sh4"), ("nerf", "sh5"), ("nerf", "ff12"), ("idr", "sh4"), ("idr", "ff5")]
ROW_TAGS = ["sh1", "sh2", "sh3", "sh4", "sh5", "ff1", "ff5", "ff12"]
WIDTH = {"sh1": 1, "sh2": 4, "sh3": 9, "sh4": 16, "sh5": 25, "ff1": 5, "ff5": 13, "ff12": 27}


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def _ulps(a, b):
    """distance of two fp32 tensors in units in the last place of the larger magnitude"""
    a, b = a.float(), b.float()
    spacing = torch.from_numpy(np.spacing(np.maximum(np.abs(a.numpy()), np.abs(b.numpy())).astype(np.float32)))
    return float(((a.double() - b.double()).abs() / spacing.double()).max())


# ---- embed_ref against the reference's recorded numbers --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ROW_TAGS)
def test_rows_match_the_recorded_reference(tag):
    z = _load("g22_embed_rows")
    dirs = tensor(z["dirs"])
    assert dirs.shape == (256, 3) and float((dirs.norm(dim=1) - 1).abs().max()) < 1e-6
    for ax in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]):
        assert bool((dirs == torch.tensor(ax, dtype=torch.float32)).all(dim=1).any()), ax
    emb = ER.parse(tag)
    if emb.kind == "fourier":
        emb.B = tensor(z["B." + tag])
        assert emb.B.shape == (3, emb.n) and emb.B.dtype == torch.float32
    ref32, ref64 = tensor(z[tag]), tensor(z[tag + ".f64"])
    assert ref32.shape == (256, WIDTH[tag]) == (256, emb.dim) and ref32.dtype == torch.float32 and ref64.dtype == torch.float64
    got32, got64 = ER.embed(dirs, emb), ER.embed(dirs.double(), emb)
    assert got32.dtype == torch.float32 and got64.dtype == torch.float64
    u = _ulps(got32, ref32)
    print(f"{tag}: fp32 rows within {u:.2f} ulp of the reference's, fp64 within {float((got64 - ref64).abs().max()):.1e}")
    # the same elementwise torch expressions: the same bits, or a last-place difference where an expression was regrouped
    assert torch.equal(got32, ref32) or u <= 1.0
    assert float((got64 - ref64).abs().max()) < 1e-14
    if emb.kind == "fourier":
        assert torch.equal(got32[:, :3], dirs)


def test_sh_sixth_term_is_not_the_unit_sphere_shortcut():
    """result[..., 6] = C2[2] (2 zz - xx - yy): equal to C2[2] (3 zz - 1) on the unit sphere only; off it (a direction that is not
    normalised) the two differ, and the reference's form is the one to follow"""
    v = torch.tensor([[0.3, -0.2, 0.9], [1.0, 2.0, -0.5]], dtype=torch.float64)
    got = ER.spherical_harmonics(v, 3)[:, 6]
    x, y, z = v.unbind(-1)
    assert torch.allclose(got, ER.C2[2] * (2 * z * z - x * x - y * y), rtol=0, atol=1e-15)
    assert float((got - ER.C2[2] * (3 * z * z - 1)).abs().max()) > 0.1


@pytest.mark.parametrize("mode,tag", NETS)
def test_radiance_net_matches_the_recorded_reference(mode, tag):
    z = _load(f"g22_embed_{mode}_{tag}")
    biggest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("g21_hdr_"))
    assert os.path.getsize(os.path.join(GOLDEN, f"g22_embed_{mode}_{tag}.npz")) <= biggest
    sd = sd_from_npz(z)
    emb = ER.parse(tag)
    idr = mode == "idr"
    assert tuple(sd["rendering_network.lin0.weight_v"].shape) == (64, emb.dim + (6 if idr else 0) + 64)
    assert (ER.B_KEY in sd) == (emb.kind == "fourier")
    emb = ER.embed_of(sd, emb.kind, emb.n)
    rgb, fbar, nbar, grads = ER.rgb_grads(sd, orc.plumbing_cfg().rgb, emb, tensor(z["view_dirs"]), tensor(z["feat"]), tensor(z["rgb_bar"]),
                                          tensor(z["points"]) if idr else None, tensor(z["normals"]) if idr else None)
    assert_close(rgb, tensor(z["rgb"]), 1e-6, "rgb")
    assert_close(fbar, tensor(z["fbar"]), 1e-6, "d/d feature")
    if idr:
        assert_close(nbar, tensor(z["nbar"]), 1e-6, "d/d normals")
    ref = {k[len("grad."):]: tensor(z[k]) for k in z.files if k.startswith("grad.")}
    assert set(ref) == set(grads) and ER.B_KEY not in ref
    for k, v in ref.items():
        assert_close(grads[k], v, 1e-6, k)


# ---- embed_ref against the live reference ------------------------------------------------------------------------------------------------
def _live_reference():
    sys.path.insert(0, GOLDEN)
    import ref_import
    if not ref_import.available():
        pytest.skip("the reference is not on this machine")
    return ref_import, ref_import.import_reference()[0]


def _ref_kwargs(tag):
    return dict(embed_type="spherical_harmonics", degree=int(tag[2:])) if tag.startswith("sh") else \
        dict(embed_type="fourier", channels=int(tag[2:]), sigma=1.5)


@pytest.mark.parametrize("tag", ["sh1", "sh2", "sh3", "sh4", "sh5", "ff1", "ff7", "ff12"])
def test_rows_match_the_live_reference(tag):
    _live_reference()
    from model.network.embedder import get_embedder
    torch.manual_seed(11)
    kw = _ref_kwargs(tag)
    fn, width = get_embedder(kw.pop("embed_type"), input_dims=3, **kw)
    v = torch.nn.functional.normalize(torch.randn(1000, 3, generator=torch.Generator().manual_seed(4)), dim=1)
    emb = ER.parse(tag)
    if emb.kind == "fourier":
        emb.B = fn.B.detach().clone()
    assert width == emb.dim
    with torch.no_grad():
        ref = fn(v)
    got = ER.embed(v, emb)
    assert torch.equal(got, ref) or _ulps(got, ref) <= 1.0


@pytest.mark.parametrize("mode", ["nerf", "idr"])
@pytest.mark.parametrize("tag", ["sh4", "sh2", "ff12", "ff3"])
def test_radiance_net_matches_the_live_reference(mode, tag):
    _live_reference()
    from model.network.mlp import RenderingNetwork
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(3)
    rnet = RenderingNetwork(64, mode=mode, d_in=9 if mode == "idr" else 3, d_out=3, dims=[64, 64], weight_norm=True, **_ref_kwargs(tag))
    sd = {"rendering_network." + k: v.detach().clone() for k, v in rnet.state_dict().items()}
    emb = ER.parse(tag)
    emb = ER.embed_of(sd, emb.kind, emb.n)
    idr = mode == "idr"
    M = 100
    pts, nrm = torch.randn(M, 3, generator=g), torch.randn(M, 3, generator=g)
    view = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1)
    feat, w = torch.randn(M, 64, generator=g), torch.randn(M, 3, generator=g)
    f_, n_ = feat.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
    rgb_ref = rnet(pts, n_, view, f_)
    (rgb_ref * w).sum().backward()
    rgb, fbar, nbar, grads = ER.rgb_grads(sd, orc.plumbing_cfg().rgb, emb, view, feat, w, pts if idr else None, nrm if idr else None)
    assert_close(rgb, rgb_ref, 1e-6, "rgb")
    assert_close(fbar, f_.grad, 1e-6, "d/d feature")
    if idr:
        assert_close(nbar, n_.grad, 1e-6, "d/d normals")
    for n, p in rnet.named_parameters():
        assert_close(grads["rendering_network." + n], p.grad, 1e-6, n)
    # the module's state_dict is the reference's: keys, order, shapes
    from i2sdf_amd import I2SDFNetwork
    from i2sdf_amd.config import plumbing_conf
    mine = [(k, tuple(v.shape)) for k, v in I2SDFNetwork(ER.embed_conf(plumbing_conf(), emb, mode)).state_dict().items() if k.startswith("rendering_network.")]
    assert mine == [(k, tuple(v.shape)) for k, v in sd.items()]


def test_the_reference_raises_on_multires_beside_the_new_types():
    _live_reference()
    from model.network.mlp import RenderingNetwork
    for kw in (_ref_kwargs("sh4"), _ref_kwargs("ff12")):
        with pytest.raises(TypeError):
            RenderingNetwork(64, mode="nerf", d_in=3, d_out=3, dims=[64, 64], weight_norm=True, multires=4, **kw)


@pytest.mark.parametrize("mode,tag", [("nerf", "sh4"), ("idr", "ff12")])
def test_network_forward_and_step_differ_from_the_positional_ones_only_behind_the_embedder(mode, tag):
    """embed_ref.network_forward / training_step_grads are hdr_ref's around another embedder: the depths and the SDF side are the same bits,
    the render is another; B gets no gradient entry"""
    import hdr_ref
    from helpers import camera_inputs, make_draws, make_gt
    cfg = orc.plumbing_cfg(False)
    cfg.use_normal = True
    emb = ER.parse(tag)
    sd = ER.perturb_params(ER.init_params(cfg, emb, mode, seed=3), 0.03, seed=4)
    emb = ER.embed_of(sd, emb.kind, emb.n)
    assert (ER.B_KEY in sd) == (emb.kind == "fourier")
    if emb.kind == "fourier":
        assert list(sd).index(ER.B_KEY) + 1 == list(sd).index("rendering_network.lin0.bias")
    B = 8
    inp, gt, dr = camera_inputs(B, (0.0, 0.0, -2.0), seed=5), make_gt(B), make_draws(cfg, B, n_row=cfg.sampler.N_samples_eval, seed=2)
    lc = orc.LossCfg()
    cam, dirs, _ = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
    zo = orc.sample_z_vals(sd, cfg, dirs, cam, training=True, draws=dr, force_iters=1)
    sd0 = hdr_ref.init_params(cfg, mode, seed=3)
    sd0 = {k: (sd[k] if k.startswith("implicit_network") or k == "density.beta" else v) for k, v in sd0.items()}
    base = hdr_ref.training_step_grads(sd0, cfg, "sigmoid", mode, inp, gt, lc, dr, 0, z_override=zo)
    mine = ER.training_step_grads(sd, cfg, emb, mode, inp, gt, lc, dr, 0, z_override=zo)
    assert torch.equal(mine[0]["depth_values"], base[0]["depth_values"]) and not torch.equal(mine[0]["rgb_values"], base[0]["rgb_values"])
    assert ER.B_KEY not in mine[2] and set(mine[2]) == set(sd) - {ER.B_KEY}
    assert float(mine[2]["rendering_network.lin0.weight_v"][:, :emb.dim + (3 if mode == "idr" else 0)].abs().max()) > 0


# ---- the host side -------------------------------------------------------------------------------------------------------------------
def _conf(tag, mode="nerf", base=None, **extra):
    from i2sdf_amd.config import plumbing_conf
    conf = ER.embed_conf(base if base is not None else plumbing_conf(), ER.parse(tag), mode)
    conf["rendering_network"].update(extra)
    return conf


def test_config_reads_both_types_and_refuses_with_the_reason():
    from i2sdf_amd.config import NetConfig, plumbing_conf, synthetic_conf
    for base, F in ((plumbing_conf(), 64), (synthetic_conf(), 256)):
        for mode in ("nerf", "idr"):
            for tag in ROW_TAGS + ["ff7"]:
                emb = ER.parse(tag)
                cfg = NetConfig.from_conf(_conf(tag, mode, base))
                e = emb.dim
                assert (cfg.rgb.embed, cfg.rgb.embed_n, cfg.rgb.multires) == (emb.kind, emb.n, 0) and cfg.rgb_mode == mode
                assert cfg.rgb.pe_dim == e + (6 if mode == "idr" else 0) and cfg.rgb.dims[0] == (base["rendering_network"]["dims"][0], cfg.rgb.pe_dim + F)
            # what was read before is read as before
            pos = NetConfig.from_conf(ER.hdr_ref.hdr_conf(base, None, mode))
            assert (pos.rgb.embed, pos.rgb.embed_n, pos.rgb.multires, pos.rgb.pe_dim) == ("positional", 0, 4, 33 if mode == "idr" else 27)
    cfg = NetConfig.from_conf(_conf("ff5", sigma=2.5))
    assert cfg.rgb_embed_sigma == 2.5 and NetConfig.from_conf(_conf("ff5", include_input=True)).rgb.embed_n == 5
    conf = _conf("sh4")
    del conf["rendering_network"]["degree"]
    assert NetConfig.from_conf(conf).rgb.embed_n == 4                      # SHEncoder's default degree
    refusals = [
        (_conf("sh4", multires=4), r"multires beside embed_type 'spherical_harmonics'.*TypeError"),
        (_conf("ff12", multires=4), r"multires beside embed_type 'fourier'.*TypeError"),
        (_conf("sh4", degree=0), r"degree must be 1\.\.5.*got 0"),
        (_conf("sh4", degree=6), r"degree must be 1\.\.5.*got 6"),
        (_conf("ff12", channels=0), r"channels must be 1\.\.12.*got 0"),
        (_conf("ff12", channels=13), r"channels must be 1\.\.12.*27 view columns.*got 13"),
        (_conf("ff12", include_input=False), r"include_input: false"),
        (_conf("sh4", embed_type="hashgrid"), r"embed_type must be 'positional', 'spherical_harmonics' or 'fourier'.*got 'hashgrid'"),
    ]
    for conf, why in refusals:
        with pytest.raises((NotImplementedError, ValueError), match=why):
            NetConfig.from_conf(conf)
    # the SDF net's embedder stays positional-only
    for etype in ("spherical_harmonics", "fourier"):
        conf = plumbing_conf()
        conf["implicit_network"]["embed_type"] = etype
        with pytest.raises(NotImplementedError, match="only embed_type='positional'"):
            NetConfig.from_conf(conf)


@pytest.mark.parametrize("mode,tag", NETS)
def test_state_dict_is_the_fixtures_and_a_fixture_checkpoint_loads(mode, tag):
    """Keys, order and shapes of the module's state_dict equal the recorded reference's, and its checkpoint loads.  (Before the embedders were
    read, `embed_type: spherical_harmonics` without `multires` was taken for "no view encoding": lin0 had 3 + F columns and this load failed.)"""
    from i2sdf_amd import I2SDFNetwork
    z = _load(f"g22_embed_{mode}_{tag}")
    sd = sd_from_npz(z)
    net = I2SDFNetwork(_conf(tag, mode))
    mine = {k: v for k, v in net.state_dict().items() if k.startswith("rendering_network.")}
    assert list(mine) == list(sd), (list(mine), list(sd))
    assert all(mine[k].shape == sd[k].shape and mine[k].dtype == sd[k].dtype for k in sd)
    full = dict(net.state_dict())
    full.update(sd)
    net.load_state_dict(full)
    after = net.state_dict()
    assert all(torch.equal(after[k], sd[k]) for k in sd)
    names = [n for n, _ in net.named_parameters()]
    assert ER.B_KEY not in names and all("embedview_fn" not in n for n in names)
    assert ER.B_KEY not in net.layout.index and net.layout.n_params == sum(p.numel() for p in net.parameters())
    if tag.startswith("ff"):
        assert [n for n, _ in net.named_buffers()] == [ER.B_KEY] and not net.rendering_network.embedview_fn.B.requires_grad
        assert net.rendering_network.embedview_fn.out_dim == ER.parse(tag).dim
    else:
        assert list(net.named_buffers()) == [] and net.rendering_network.embedview_fn is None


def test_fourier_matrix_is_drawn_once_at_construction_with_sigma():
    from i2sdf_amd import I2SDFNetwork
    torch.manual_seed(5)
    a = I2SDFNetwork(_conf("ff12", sigma=1.0))
    torch.manual_seed(5)
    b = I2SDFNetwork(_conf("ff12", sigma=3.0))
    Ba, Bb = a.rendering_network.embedview_fn.B, b.rendering_network.embedview_fn.B
    assert Ba.shape == (3, 12) and float(Ba.abs().max()) > 0 and torch.allclose(Bb, 3.0 * Ba)
    # the SDF net in front of it and the radiance layers behind it are initialised as they are without it: only B's draw lies between
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa if k != ER.B_KEY)
    torch.manual_seed(5)
    c = I2SDFNetwork(_conf("sh4"))
    assert all(torch.equal(sa[k], c.state_dict()[k]) for k in sa if k.startswith("implicit_network"))


def test_descriptor_bits():
    from i2sdf_amd.config import NetConfig, plumbing_conf, synthetic_conf
    from i2sdf_amd.params import ParamLayout
    from i2sdf_amd import lib as L
    assert L.RGB_EMBEDS == {"positional": 0, "spherical_harmonics": 1, "fourier": 2} and L.RGB_EMBED_MAX_CHANNELS == 12
    for base in (plumbing_conf(), synthetic_conf(True)):
        for mode in ("nerf", "idr"):
            for code, act in enumerate(("sigmoid", "relu", "softplus")):
                for tag in ("sh1", "sh5", "ff1", "ff12"):
                    emb = ER.parse(tag)
                    conf = _conf(tag, mode, base, output_activation=act)
                    desc = ParamLayout(NetConfig.from_conf(conf)).net_desc()
                    kind = 1 if emb.kind == "spherical_harmonics" else 2
                    assert desc.rgb.reserved == (1 if mode == "idr" else 0) | code << 8 | kind << 24
                    assert desc.rgb.multires == emb.n and desc.rgb.in0 == emb.dim + (6 if mode == "idr" else 0) + desc.sdf.d_out - 1
                    assert desc.sdf.reserved == 0 and desc.light.reserved == 0
                # a positional descriptor keeps its value: nothing above bit 15
                pos = ParamLayout(NetConfig.from_conf(ER.hdr_ref.hdr_conf(base, act, mode))).net_desc()
                assert pos.rgb.reserved == (1 if mode == "idr" else 0) | code << 8 and pos.rgb.multires == 4


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def _plan(h, desc):
    plan = C.c_void_p()
    rc = h.i2sdf_plan_create(C.byref(desc), C.byref(plan))
    return rc, plan


def test_plan_create_accepts_and_refuses(lib):
    from i2sdf_amd.config import NetConfig, plumbing_conf, synthetic_conf
    from i2sdf_amd.params import ParamLayout
    h = lib.load()
    for base in (plumbing_conf(), synthetic_conf()):
        for mode in ("nerf", "idr"):
            rc, plan = _plan(h, ParamLayout(NetConfig.from_conf(ER.hdr_ref.hdr_conf(base, None, mode))).net_desc())
            assert rc == 0
            sizes = (h.i2sdf_plan_pack_floats(plan), h.i2sdf_plan_wgrad_floats(plan))
            h.i2sdf_plan_destroy(plan)
            for tag in ROW_TAGS:
                desc = ParamLayout(NetConfig.from_conf(_conf(tag, mode, base))).net_desc()
                rc, plan = _plan(h, desc)
                assert rc == 0, (mode, tag, h.i2sdf_last_hip_error())
                # no stream, stage count or weight-gradient block depends on the embedder: the sizes are the positional plan's
                assert (h.i2sdf_plan_pack_floats(plan), h.i2sdf_plan_wgrad_floats(plan)) == sizes, (mode, tag)
                h.i2sdf_plan_destroy(plan)
            desc = ParamLayout(NetConfig.from_conf(_conf("sh4", mode, base))).net_desc()
            low = desc.rgb.reserved & 0xffff

            def refused(reserved, multires, in0, *words):
                d = type(desc).from_buffer_copy(desc)
                d.rgb.reserved, d.rgb.multires, d.rgb.in0 = reserved, multires, in0
                d.rgb.in_dim[0] = in0
                rc, _ = _plan(h, d)
                msg = h.i2sdf_last_hip_error().decode()
                assert rc == -1 and all(w in msg for w in words), (reserved, multires, in0, rc, msg)

            in0 = desc.rgb.in0
            for kind in (3, 7, 15):
                refused(low | kind << 24, 4, in0, "view embedder", "I2SDF_RGB_EMBED_FOURIER")
            refused(low | 1 << 24 | 1 << 28, 4, in0, "view embedder", "bits 28..31")
            for deg in (0, 6, -1):
                refused(low | 1 << 24, deg, in0, "degree", "1..5")
            for c in (0, 13, 64):
                refused(low | 2 << 24, c, in0, "channels", "1..12")
            refused(low | 1 << 24, 4, in0 + 1, "in0", "disagrees", "degree 4")
            refused(low | 1 << 24, 5, in0, "in0", "disagrees", "degree 5")
            refused(low | 2 << 24, 12, in0, "in0", "disagrees", "channels 12")
            # bits 16..23 keep the output activation's message
            refused(low | 1 << 24 | 1 << 16, 4, in0, "output activation")


def test_set_view_embed_is_declared_exported_bound_and_validates(lib):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.params import ParamLayout
    header = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    assert re.search(r"int\s+i2sdf_plan_set_view_embed\(i2sdf_plan\* plan, const float\* B_host, int32_t rows, int32_t cols\);", header)
    for name, val in (("POSITIONAL", 0), ("SH", 1), ("FOURIER", 2)):
        assert re.search(rf"#define I2SDF_RGB_EMBED_{name} {val}\b", header)
    assert lib.SIGNATURES["i2sdf_plan_set_view_embed"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32])
    assert getattr(C.CDLL(lib.LIB_PATH), "i2sdf_plan_set_view_embed") is not None
    h = lib.load()
    msg = lambda: h.i2sdf_last_hip_error().decode()
    B = np.ascontiguousarray(np.random.default_rng(0).standard_normal((3, 12)).astype(np.float32))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert h.i2sdf_plan_set_view_embed(None, ptr(B), 3, 12) == -1
    rc, plan = _plan(h, ParamLayout(NetConfig.from_conf(_conf("ff12"))).net_desc())
    assert rc == 0
    assert h.i2sdf_plan_set_view_embed(plan, None, 3, 12) == -1 and "NULL" in msg()
    for rows, cols in ((2, 12), (12, 3), (3, 11), (3, 13), (3, 0), (3, -1)):
        assert h.i2sdf_plan_set_view_embed(plan, ptr(B), rows, cols) == -1 and "(3, 12)" in msg(), (rows, cols)
    for bad in (np.nan, np.inf, -np.inf):
        Bn = B.copy()
        Bn[1, 7] = bad
        assert h.i2sdf_plan_set_view_embed(plan, ptr(Bn), 3, 12) == -1 and "B[1][7] is not finite" in msg()
    # a radiance forward in front of the first accepted call is refused before anything is looked at or launched (made-up pointers)
    P = C.c_void_p(4096)
    assert h.i2sdf_rgb_forward(plan, P, P, 4, P, 128, 128, P, None, None, None) == -1 and "i2sdf_plan_set_view_embed" in msg()
    assert h.i2sdf_plan_set_view_embed(plan, ptr(B), 3, 12) == 0
    h.i2sdf_plan_destroy(plan)
    rc, plan = _plan(h, ParamLayout(NetConfig.from_conf(_conf("ff12", "idr"))).net_desc())
    assert rc == 0
    assert h.i2sdf_rgb_forward_idr(plan, P, P, None, P, None, 0, 4, P, P, 128, 128, P, None, None, None) == -1 and "i2sdf_plan_set_view_embed" in msg()
    h.i2sdf_plan_destroy(plan)
    # a plan of another embedder has no matrix to take
    rc, plan = _plan(h, ParamLayout(NetConfig.from_conf(_conf("sh4"))).net_desc())
    assert rc == 0 and h.i2sdf_plan_set_view_embed(plan, ptr(B), 3, 12) == -1 and "no Fourier view embedder" in msg()
    h.i2sdf_plan_destroy(plan)
    from i2sdf_amd.config import plumbing_conf
    rc, plan = _plan(h, ParamLayout(NetConfig.from_conf(plumbing_conf())).net_desc())
    assert rc == 0 and h.i2sdf_plan_set_view_embed(plan, ptr(B), 3, 12) == -1 and "no Fourier view embedder" in msg()
    h.i2sdf_plan_destroy(plan)
