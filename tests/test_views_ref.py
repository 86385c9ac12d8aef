"""CPU: the restatement the view tests are held against (tests/views_ref.py) is itself right -- against closed forms, against the
padded route torchmetrics takes, and, for the camera path, against scipy used the way dataset/eval_dataset.py:219-239 uses it.
i2sdf_amd.views.interpolate_poses runs on the host, so it is checked here too."""
import math

import numpy as np
import pytest
import torch

import views_ref as VR


def test_gaussian_sums_to_one_and_is_symmetric():
    g = VR.gaussian()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 1e-15
    assert np.array_equal(g, g[::-1]) and int(np.argmax(g)) == 5
    assert abs(g[4] / g[5] - math.exp(-(1 / 1.5) ** 2 / 2)) <= 1e-15
    g32 = VR.gaussian(np.float32)
    assert g32.dtype == np.float32 and np.abs(g32.astype(np.float64) - g).max() <= 2.0 ** -24


@pytest.mark.parametrize("H,W", [(11, 11), (11, 30), (23, 37), (40, 29)])
def test_reflect_pad_and_crop_equals_the_valid_window(H, W):
    pred, gt = VR.view_pair(H, W, seed=H * 100 + W, noise=0.05)
    p, t = pred.reshape(H, W, 3), gt.reshape(H, W, 3)
    for R in (None, 1.0):
        a, b = VR.ssim_map_f64(p, t, R), VR.ssim_map_f64_padded(p, t, R)
        assert a.shape == b.shape == (H - 10, W - 10, 3)
        assert np.abs(a - b).max() <= 1e-12


def test_identical_images():
    pred, _ = VR.view_pair(24, 31, seed=3, noise=0.05)
    x = pred.reshape(24, 31, 3)
    assert np.all(VR.ssim_map_f64(x, x) == 1.0) and VR.ssim(x, x) == 1.0
    assert np.all(VR.ssim_map_f32_conv2d(x, x) == 1.0) and np.all(VR.ssim_map_f32_separable(x, x) == 1.0)
    assert VR.psnr(x, x) == math.inf


def test_psnr_of_a_constant_offset():
    rng = np.random.default_rng(0)
    for d in (0.5, 0.125, 2.0 ** -6):                     # (exact in fp32, so x + d - x == d for x in [0, 0.5))
        x = (rng.integers(0, 1 << 12, (19 * 23, 3)) / float(1 << 13)).astype(np.float32)
        y = x + np.float32(d)
        assert np.all(y.astype(np.float64) - x.astype(np.float64) == d)
        assert abs(VR.psnr(x, y) - (-20.0 * math.log10(d))) <= 1e-12


def test_ssim_of_two_constant_images():
    for a, b, R in ((0.25, 0.75, 1.0), (0.5, 0.5, 1.0), (0.125, 0.875, 2.0)):
        p, t = np.full((13, 17, 3), a, np.float32), np.full((13, 17, 3), b, np.float32)
        c1 = (0.01 * R) ** 2
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        got = VR.ssim_map_f64(p, t, R)
        assert np.abs(got - want).max() <= 1e-12 and abs(VR.ssim(p, t, R) - want) <= 1e-12


def test_fp32_forms_are_near_fp64_and_the_separable_one_is_no_worse():
    H, W = 37, 45
    pred, gt = VR.view_pair(H, W, seed=11, noise=0.05)
    p, t = pred.reshape(H, W, 3), gt.reshape(H, W, 3)
    ref = VR.ssim_map_f64(p, t)
    e2d = np.abs(VR.ssim_map_f32_conv2d(p, t) - ref).max()
    esep = np.abs(VR.ssim_map_f32_separable(p, t) - ref).max()
    print(f"fp32 2-D window {e2d:.2e}, fp32 separable {esep:.2e}")
    assert 0 < e2d < 1e-2 and esep <= 2 * e2d


def test_frame_restatements():
    rgb = np.array([[-0.1, 0.0, 0.5], [1.0, 1.1, 0.999]], np.float32)
    assert VR.rgb8_f32(rgb).tolist() == [[0, 0, 127], [255, 255, 254]]
    pose = np.eye(4)
    pose[:3, :3] = VR.random_rotation(np.random.default_rng(1))
    n = np.random.default_rng(2).standard_normal((5, 3)).astype(np.float32)
    want = np.stack([pose[:3, :3].astype(np.float32).astype(np.float64).T @ v.astype(np.float64) for v in n])
    assert np.abs(VR.normal_cam_f64(n, pose) - want).max() <= 1e-15
    d = np.array([0.0, 1.5, 3.0], np.float32)
    pre = VR.depth8_pre(d)
    assert pre[0] == 0 and abs(pre[1] - 127.5) < 1e-4 and 254.99 < pre[2] < 255
    assert VR.near_integer(np.array([3.00005, 3.5, 3.99995])).tolist() == [True, False, True]


def test_view_pair_is_seeded_and_has_its_flat_patch():
    a, b = VR.view_pair(24, 30, 5, 0.05)
    a2, b2 = VR.view_pair(24, 30, 5, 0.05)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and a.dtype == np.float32 and a.shape == (720, 3)
    assert np.all(b.reshape(24, 30, 3)[:12, :10] == np.float32(0.95)) and a.min() >= 0 and a.max() <= 1
    assert not np.array_equal(VR.view_pair(24, 30, 6, 0.05)[1], b)


ANGLES = (3.0, 45.0, 90.0, 135.0, 170.0)


def _scipy_path(p0, p1, num_frames):
    """The camera path through scipy, as the reference's InterpolateDataset builds it: Slerp over [0, 1] between the TRANSPOSED
    rotations of the two poses, evaluated at VR.ratios(), transposed back; the translations blended with the same ratios."""
    from scipy.spatial.transform import Rotation, Slerp
    s = np.array(VR.ratios(num_frames))
    between = Slerp([0.0, 1.0], Rotation.from_matrix([p0[:3, :3].T, p1[:3, :3].T]))
    path = np.tile(np.eye(4), (num_frames, 1, 1))
    path[:, :3, :3] = between(s).as_matrix().transpose(0, 2, 1)
    path[:, :3, 3] = np.outer(1.0 - s, p0[:3, 3]) + np.outer(s, p1[:3, 3])
    return path


@pytest.mark.parametrize("num_frames", [1, 2, 60])
def test_interpolate_poses_matches_scipy(num_frames):
    """Inputs are fp64 poses with rotations orthogonal to fp64 rounding, so both sides do fp64 work on the same numbers; what remains
    is the fp32 rounding of the output: entries of R are <= 1 (half an ulp: 6e-8), of t <= 4 (1.2e-7).  Bar 2e-7 on every entry."""
    from i2sdf_amd.views import interpolate_poses
    for seed, ang in enumerate(ANGLES):
        p0, p1 = VR.pose_pair(seed, ang)
        got = interpolate_poses(torch.from_numpy(p0), torch.from_numpy(p1), num_frames)
        assert got.shape == (num_frames, 4, 4) and got.dtype == torch.float32
        want = _scipy_path(p0, p1, num_frames)
        err = np.abs(got.numpy().astype(np.float64) - want).max()
        own = np.abs(VR.pose_path_axis_angle(p0, p1, num_frames) - want).max()
        print(f"angle {ang}: views vs scipy {err:.2e}, axis-angle restatement vs scipy {own:.2e}")
        assert own <= 1e-12
        assert err <= 2e-7
        assert np.array_equal(got.numpy()[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (num_frames, 1)))
        if num_frames == 1:                               # ratio_0 = 0: the first pose, rounded to fp32
            assert np.array_equal(got[0].numpy(), p0.astype(np.float32))


def test_interpolate_poses_takes_the_shortest_arc_and_refuses_bad_input():
    from i2sdf_amd.views import interpolate_poses
    p0, p1 = VR.pose_pair(7, 170.0)
    path = interpolate_poses(p0, p1, 60).numpy().astype(np.float64)
    step = [math.degrees(math.acos(min(1.0, (np.trace(path[i + 1, :3, :3] @ path[i, :3, :3].T) - 1) / 2))) for i in range(59)]
    assert sum(step) < 170.0 + 1e-3 and max(step) < 5.0
    assert np.abs(path[:, :3, :3] @ path[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    with pytest.raises(ValueError):
        interpolate_poses(p0, p1, 0)
    with pytest.raises(ValueError):
        interpolate_poses(p0[:3], p1, 4)


def test_pixel_grid_is_x_fastest_xy_order():
    from i2sdf_amd.views import pixel_grid
    uv = pixel_grid(3, 4)
    assert uv.shape == (1, 12, 2) and uv.dtype == torch.float32
    assert uv[0, :5].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [0, 1]] and uv[0, -1].tolist() == [3, 2]
