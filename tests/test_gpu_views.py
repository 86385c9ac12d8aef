"""GPU: rendered views on the device (i2sdf_amd.views, csrc/imgops.hip) against the restatement of tests/views_ref.py.

SSIM map: max |map - fp64 restatement| <= 2 E32, E32 = the fp32 2-D-window restatement's own maximum error against fp64 on the same
input (the reference's arithmetic; the factor 2 because the separable order differs from the 2-D order).  Both are printed.
SSIM mean: the fp64 mean of the kernel's own map at 1e-12 relative (the reduction drops or repeats no tile); bit-identical with and
without the map and from run to run; ssim(x, x) == 1 exactly.
PSNR / stats: the squared error at 1e-12 relative against fp64 on the same fp32 inputs; min, max and depth max exact; bit-identical
from run to run; psnr(x, x) == inf.
Frames: rgb8 exact; normal8, depth8, depth_rgb8 equal except where the fp64 value before truncation lies within 1e-4 of an integer
(at most 0.5 % of the values); fp32 n_cam within 3 fp32 ulp of fp64.
evaluate_views / render_path: bitwise the per-view render_image calls and image_metrics / to_frames on their outputs."""
import math

import numpy as np
import pytest
import torch

import views_ref as VR

pytestmark = pytest.mark.gpu

TX, TY = 32, 16                                            # I2SDF_SSIM_TILE_X, I2SDF_SSIM_TILE_Y (asserted below)
SIZES = [(11, 11), (11, 75), (53, 11), (48, 64), (59, 83), (2 * TY + 13, 2 * TX + 15)]
SMALL = [(1, 1), (7, 5)]
N_VIEWS = 3
_cache = {}


def _inputs(H, W, noise):
    """3 seeded views and their restatements, computed once and shared (read-only)."""
    key = (H, W, noise)
    if key not in _cache:
        pairs = [VR.view_pair(H, W, seed=1000 * H + 10 * W + v, noise=noise) for v in range(N_VIEWS)]
        pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
        entry = {"pred": pred, "gt": gt, "ref": {}}
        _cache[key] = entry
    return _cache[key]


def _ssim_refs(entry, H, W, R):
    if R not in entry["ref"]:
        f64 = np.stack([VR.ssim_map_f64(entry["pred"][v].reshape(H, W, 3), entry["gt"][v].reshape(H, W, 3), R) for v in range(N_VIEWS)])
        f32 = np.stack([VR.ssim_map_f32_conv2d(entry["pred"][v].reshape(H, W, 3), entry["gt"][v].reshape(H, W, 3), R) for v in range(N_VIEWS)])
        entry["ref"][R] = (f64, float(np.abs(f32.astype(np.float64) - f64).max()))
    return entry["ref"][R]


def test_tile_constants():
    from i2sdf_amd import lib as L
    assert (L.SSIM_TILE_X, L.SSIM_TILE_Y) == (TX, TY)


@pytest.mark.parametrize("data_range", [None, 1.0])
@pytest.mark.parametrize("noise", [0.05, 0.002])
@pytest.mark.parametrize("H,W", SIZES)
def test_ssim_map_and_mean(H, W, noise, data_range):
    from i2sdf_amd import views as V
    e = _inputs(H, W, noise)
    ref, e32 = _ssim_refs(e, H, W, data_range)
    pred, gt = torch.from_numpy(e["pred"]).cuda(), torch.from_numpy(e["gt"]).cuda()
    mean, smap = V.ssim(pred, gt, (H, W), data_range=data_range, return_map=True)
    assert mean.shape == (N_VIEWS,) and mean.dtype == torch.float64 and smap.shape == (N_VIEWS, H - 10, W - 10, 3)
    got = smap.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"{H}x{W} noise {noise} data_range {data_range}: kernel {err:.3e}, fp32 2-D restatement E32 {e32:.3e}, ratio {err / e32:.3f}")
    assert e32 > 0
    assert err <= 2 * e32, (err, e32)
    # the reduction: the mean is the fp64 mean of the kernel's own map
    own = got.reshape(N_VIEWS, -1).mean(1)
    rel = np.abs(mean.cpu().numpy() - own) / np.abs(own)
    assert rel.max() <= 1e-12, rel
    # bit-identical without the map, and from run to run
    assert torch.equal(V.ssim(pred, gt, (H, W), data_range=data_range), mean)
    mean2, smap2 = V.ssim(pred, gt, (H, W), data_range=data_range, return_map=True)
    assert torch.equal(mean2, mean) and torch.equal(smap2, smap)
    # one view alone gives its value of the batch (a view's slots are its own)
    assert torch.equal(V.ssim(pred[1], gt[1], (H, W), data_range=data_range), mean[1:2])


@pytest.mark.parametrize("H,W", SIZES)
def test_ssim_of_identical_images_is_one(H, W):
    from i2sdf_amd import views as V
    x = torch.from_numpy(_inputs(H, W, 0.05)["pred"]).cuda()
    for R in (None, 1.0):
        mean, smap = V.ssim(x, x, (H, W), data_range=R, return_map=True)
        assert bool((smap == 1.0).all()) and mean.cpu().tolist() == [1.0] * N_VIEWS


@pytest.mark.parametrize("H,W", SIZES + SMALL)
def test_psnr_and_stats(H, W):
    from i2sdf_amd import views as V
    e = _inputs(H, W, 0.05)
    rng = np.random.default_rng(H * 7 + W)
    depth = rng.uniform(0, 6, (N_VIEWS, H * W, 1)).astype(np.float32)
    pred, gt, d = (torch.from_numpy(a).cuda() for a in (e["pred"], e["gt"], depth))
    st = V.image_stats(pred, gt, (H, W), depth=d)
    assert st.shape == (N_VIEWS, 8) and st.dtype == torch.float64
    s = st.cpu().numpy()
    for v in range(N_VIEWS):
        want = VR.sse(e["pred"][v], e["gt"][v])
        print(f"{H}x{W} view {v}: sse {s[v, 0]:.17g} vs fp64 {want:.17g}, rel {abs(s[v, 0] - want) / want:.2e}")
        assert abs(s[v, 0] - want) <= 1e-12 * want
        assert s[v, 1:6].tolist() == [float(e["pred"][v].min()), float(e["pred"][v].max()), float(e["gt"][v].min()), float(e["gt"][v].max()),
                                      float(depth[v].max())]
    assert torch.equal(V.image_stats(pred, gt, (H, W), depth=d), st)
    ps = V.psnr(pred, gt, (H, W))
    assert ps.shape == (N_VIEWS,) and ps.dtype == torch.float64 and torch.equal(V.psnr(pred, gt, (H, W)), ps)
    for v in range(N_VIEWS):
        assert abs(float(ps[v]) - VR.psnr(e["pred"][v], e["gt"][v])) <= 1e-10
    assert V.psnr(pred, pred, (H, W)).cpu().tolist() == [math.inf] * N_VIEWS
    if H >= 11 and W >= 11:                               # one stats pass shared by both metrics: the same bits as the two calls
        m = V.image_metrics(pred, gt, (H, W))
        assert torch.equal(m["psnr"], ps) and torch.equal(m["ssim"], V.ssim(pred, gt, (H, W)))


@pytest.mark.parametrize("H,W", [(7, 5), (48, 64)])
def test_frames(H, W):
    from i2sdf_amd import views as V
    rng = np.random.default_rng(100 * H + W)
    hw = H * W
    rgb = rng.uniform(-0.1, 1.1, (N_VIEWS, hw, 3)).astype(np.float32)
    nrm = rng.standard_normal((N_VIEWS, hw, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    depth = rng.uniform(0, 6, (N_VIEWS, hw, 1)).astype(np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (N_VIEWS, 1, 1))
    for v in range(N_VIEWS):
        poses[v, :3, :3] = VR.random_rotation(rng)
        poses[v, :3, 3] = rng.uniform(-2, 2, 3)
    lut = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    cu = lambda a: torch.from_numpy(a).cuda()
    out = V.to_frames(rgb=cu(rgb), normal_map=cu(nrm), depth=cu(depth), pose=cu(poses), img_res=(H, W), lut=cu(lut), camera_normals=True)
    assert sorted(out) == ["depth8", "depth_rgb8", "normal8", "normal_cam", "rgb8"]
    for k, c in (("rgb8", 3), ("normal8", 3), ("depth8", 1), ("depth_rgb8", 3)):
        assert out[k].shape == (N_VIEWS, H, W, c) and out[k].dtype == torch.uint8, k
    got = {k: t.cpu().numpy() for k, t in out.items()}
    assert np.array_equal(got["rgb8"].reshape(N_VIEWS, hw, 3), VR.rgb8_f32(rgb))
    assert got["rgb8"].min() == 0 and got["rgb8"].max() == 255              # the clip is exercised on both sides
    n_pre = np.stack([VR.normal8_pre(nrm[v], poses[v]) for v in range(N_VIEWS)])
    d_pre = np.stack([VR.depth8_pre(depth[v]) for v in range(N_VIEWS)])
    n_near, d_near = VR.near_integer(n_pre), VR.near_integer(d_pre)
    print(f"{H}x{W}: pre-truncation values within 1e-4 of an integer: normal {n_near.mean() * 100:.3f} %, depth {d_near.mean() * 100:.3f} %")
    # The restatement alone stays far inside the cap (uniform fractional parts put 0.02 % there) -- but for one pixel per view that
    # is there by construction: the view's maximum maps to 255 max / (max + 1e-6), within 1e-4 of 255 whenever max > 0.00255, and
    # it is 1 of the 35 pixels of the 7 x 5 view.  It is left out of this count (only of this one: it stays an allowed exception
    # below, and the cap on the exceptions the kernel actually takes is asserted over every value).
    is_max = depth == depth.max(axis=1, keepdims=True)
    assert is_max.sum() == N_VIEWS and d_near[is_max].all()
    assert n_near.mean() <= 0.005 and (d_near & ~is_max).mean() <= 0.005
    n8, d8 = np.floor(n_pre).astype(np.uint8), np.floor(d_pre).astype(np.uint8)
    n_diff = got["normal8"].reshape(N_VIEWS, hw, 3) != n8
    d_diff = got["depth8"].reshape(N_VIEWS, hw, 1) != d8
    assert not (n_diff & ~n_near).any() and not (d_diff & ~d_near).any()
    assert n_diff.mean() <= 0.005 and d_diff.mean() <= 0.005
    assert np.abs(got["normal8"].reshape(N_VIEWS, hw, 3).astype(int) - n8.astype(int)).max() <= 1
    assert np.array_equal(got["depth_rgb8"].reshape(N_VIEWS, hw, 3), lut[got["depth8"].reshape(N_VIEWS, hw)])   # the table look-up itself
    c_diff = (got["depth_rgb8"].reshape(N_VIEWS, hw, 3) != lut[d8[..., 0]]).any(-1, keepdims=True)
    assert not (c_diff & ~d_near).any() and c_diff.mean() <= 0.005
    # fp32 n_cam within 3 fp32 ulp of the fp64 value -- the ulp of that value itself, however small a cancelling sum leaves it
    want = np.stack([VR.normal_cam_f64(nrm[v], poses[v]) for v in range(N_VIEWS)])
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    e_n = np.abs(got["normal_cam"].astype(np.float64) - want) / ulp
    print(f"{H}x{W}: n_cam error {e_n.max():.2f} ulp")
    assert e_n.max() <= 3.0
    with pytest.raises(ValueError, match="lut"):            # a host table would be copied on every call: refused
        V.to_frames(depth=cu(depth), img_res=(H, W), lut=torch.from_numpy(lut))
    # outputs are optional, one by one
    only = V.to_frames(depth=cu(depth), img_res=(H, W))
    assert sorted(only) == ["depth8"] and torch.equal(only["depth8"], out["depth8"])
    one = V.to_frames(rgb=cu(rgb[1]), normal_map=cu(nrm[1]), pose=cu(poses[1]), img_res=(H, W))
    assert sorted(one) == ["normal8", "rgb8"] and torch.equal(one["rgb8"], out["rgb8"][1:2]) and torch.equal(one["normal8"], out["normal8"][1:2])


@pytest.fixture(scope="module")
def net_and_views():
    from i2sdf_amd import I2SDFNetwork, plumbing_conf
    from oracle import i2sdf_oracle as orc
    H, W = 24, 32
    conf = dict(plumbing_conf())
    conf["use_normal"] = True
    ocfg = orc.plumbing_cfg()
    ocfg.use_normal = True
    sd = orc.perturb_params(orc.init_params(ocfg, seed=41), 0.05, seed=42)
    sd["density.beta"] = torch.tensor(0.05)
    net = I2SDFNetwork(conf)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    K = torch.eye(4); K[0, 0] = K[1, 1] = 30.0; K[0, 2], K[1, 2] = W / 2, H / 2
    p0, p1 = VR.pose_pair(3, 25.0, t_scale=0.3)
    p0[:3, 3] += -1.8 * p0[:3, 2]; p1[:3, 3] += -1.8 * p1[:3, 2]          # step back along the view axis: the scene is in front
    poses = torch.from_numpy(np.stack([p0, p1])).float()
    gt = torch.from_numpy(np.stack([VR.view_pair(H, W, 50 + v, 0.0)[1] for v in range(2)])).cuda()
    return net, poses.cuda(), K.cuda(), gt, (H, W)


def test_evaluate_views_equals_per_view_calls(net_and_views):
    from i2sdf_amd import views as V
    net, poses, K, gt, (H, W) = net_and_views
    CH = 300                                               # not a divisor of 768: a ragged last chunk
    res = net.evaluate_views(poses, K, (H, W), gt_rgb=gt, split_n_pixels=CH, frames=True)
    uv = V.pixel_grid(H, W, poses.device)
    names = {"rgb_values": 3, "depth_values": 1, "normal_map": 3}
    for i in range(2):
        one = net.render_image({"uv": uv, "pose": poses[i:i + 1], "intrinsics": K[None]}, CH)
        for k, c in names.items():
            assert res[k].shape == (2, H * W, c) and torch.equal(res[k][i], one[k].reshape(H * W, c)), (i, k)
        assert torch.equal(res["sampler_iters"][i], net.last_sampler_iters), i
    assert res["sampler_iters"].shape == (2, 3) and bool((res["sampler_iters"] >= 1).all())
    m = V.image_metrics(res["rgb_values"], gt, (H, W))
    assert torch.equal(res["psnr"], m["psnr"]) and torch.equal(res["ssim"], m["ssim"])
    assert bool(torch.isfinite(res["psnr"]).all()) and bool(((res["ssim"] > -1) & (res["ssim"] < 1)).all())
    f = V.to_frames(rgb=res["rgb_values"], normal_map=res["normal_map"], depth=res["depth_values"], pose=poses, img_res=(H, W))
    for k in ("rgb8", "normal8", "depth8"):
        assert res[k].shape[:3] == (2, H, W) and torch.equal(res[k], f[k]), k
    lean = net.evaluate_views(poses, K, (H, W), gt_rgb=gt, split_n_pixels=CH, frames=True, keep_outputs=False)
    assert "rgb_values" not in lean and "normal_map" not in lean
    for k in ("psnr", "ssim", "rgb8", "normal8", "depth8", "sampler_iters"):
        assert torch.equal(lean[k], res[k]), k
    assert float(res["rgb_values"].std()) > 1e-3           # the views show something


def test_render_image_refuses_output_buffers_that_do_not_fit(net_and_views):
    from i2sdf_amd import views as V
    net, poses, K, gt, (H, W) = net_and_views
    dev, P = poses.device, H * W
    eng = net._engine_for(dev)
    uv = V.pixel_grid(H, W, dev)[0]
    f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    for bad in ({"rgb": f(P, 4)}, {"rgb": f(P - 1, 3)}, {"rgb": f(P, 3, dt=torch.float64)}, {"depth": f(P, 2)[:, 0]}, {"depth": f(P, 1)},
                {"iters": f(3)}, {"iters": f(2, dt=torch.int32)}, {"z": f(P, eng.n_z)}, {"rgb": torch.empty(P, 3)}, {"colour": f(P, 3)}):
        with pytest.raises(ValueError, match="does not fit"):
            eng.render_image(net._flat, uv, poses[0], K, 300, out=bad)
    buf = {"rgb": f(P, 3), "iters": f(3, dt=torch.int32)}
    o = eng.render_image(net._flat, uv, poses[0], K, 300, out=buf)
    assert o["rgb"] is buf["rgb"] and o["iters"] is buf["iters"]
    assert torch.equal(o["rgb"], eng.render_image(net._flat, uv, poses[0], K, 300)["rgb"])


def test_render_path(net_and_views):
    from i2sdf_amd import views as V
    net, poses, K, gt, (H, W) = net_and_views
    out = net.render_path(poses[0], poses[1], K, (H, W), num_frames=3, split_n_pixels=300)
    assert out["rgb8"].shape == (3, H, W, 3) and out["normal8"].shape == (3, H, W, 3) and out["rgb8"].dtype == torch.uint8
    assert out["sampler_iters"].shape == (3, 3)
    want = V.interpolate_poses(poses[0], poses[1], 3)
    assert out["poses"].shape == (3, 4, 4) and torch.equal(out["poses"].cpu(), want)
    assert torch.equal(out["poses"][0].cpu(), poses[0].cpu())           # ratio_0 = 0
    direct = net.evaluate_views(want, K, (H, W), split_n_pixels=300, frames=True)
    assert torch.equal(out["rgb8"], direct["rgb8"]) and torch.equal(out["normal8"], direct["normal8"])
    assert "normal8" not in net.render_path(poses[0], poses[1], K, (H, W), num_frames=1, use_normal=False, split_n_pixels=300)
