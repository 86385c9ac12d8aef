"""Restatement for the tests of i2sdf_amd.views (csrc/imgops.hip): numpy / torch on the CPU, fp64 unless said.

SSIM is torchmetrics 0.11.4's `structural_similarity_index_measure` with its defaults, restated from its source (the library is not
available where this project is built, so this file -- checked against closed forms in tests/test_views_ref.py -- is the yardstick):
Gaussian window of 11 taps, sigma 1.5, k1 = 0.01, k2 = 0.03, reflect-pad by 5, five windowed moments, crop 5, mean.
Images here are (H, W, 3) arrays (the (H W, 3) render layout reshaped)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
PAD = WIN // 2


def gaussian(dtype=np.float64):
    d = np.arange(WIN, dtype=np.float64) - PAD
    g = np.exp(-(d / SIGMA) ** 2 / 2.0)
    return (g / g.sum()).astype(dtype)


def data_range_of(pred, gt):
    """torchmetrics' data_range=None: max(max p - min p, max t - min t), from the fp32 images."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    return float(max(np.float32(pred.max()) - np.float32(pred.min()), np.float32(gt.max()) - np.float32(gt.min())))


def _formula(m, c1, c2):
    ep, et, epp, ett, ept = m
    pp, tt, pt = ep * ep, et * et, ep * et
    sp, st, spt = epp - pp, ett - tt, ept - pt
    return ((2 * pt + c1) * (2 * spt + c2)) / ((pp + tt + c1) * (sp + st + c2))


def _valid_window_2d(x, k2d):
    """(H - 10, W - 10, C): correlation of x (H, W, C) with the 2-D window over the positions where it lies inside."""
    H, W = x.shape[:2]
    out = np.zeros((H - WIN + 1, W - WIN + 1) + x.shape[2:], dtype=x.dtype)
    for j in range(WIN):
        for i in range(WIN):
            out += k2d[j, i] * x[j:j + H - WIN + 1, i:i + W - WIN + 1]
    return out


def ssim_map_f64(pred, gt, data_range=None):
    """(H - 10, W - 10, 3) fp64 from the fp32 images: the 2-D window (outer product of the Gaussian) on the valid positions."""
    R = data_range_of(pred, gt) if data_range is None else float(data_range)
    p, t = np.asarray(pred, np.float32).astype(np.float64), np.asarray(gt, np.float32).astype(np.float64)
    g = gaussian()
    k2d = np.outer(g, g)
    m = [_valid_window_2d(x, k2d) for x in (p, t, p * p, t * t, p * t)]
    return _formula(m, (K1 * R) ** 2, (K2 * R) ** 2)


def ssim_map_f64_padded(pred, gt, data_range=None):
    """The same through the library's own route: reflect-pad by 5, window at every position of the padded image that fits, crop 5."""
    R = data_range_of(pred, gt) if data_range is None else float(data_range)
    p, t = np.asarray(pred, np.float32).astype(np.float64), np.asarray(gt, np.float32).astype(np.float64)
    pad = lambda x: np.pad(x, ((PAD, PAD), (PAD, PAD), (0, 0)), mode="reflect")
    p, t = pad(p), pad(t)
    g = gaussian()
    k2d = np.outer(g, g)
    m = [_valid_window_2d(x, k2d) for x in (p, t, p * p, t * t, p * t)]          # (H, W, 3): one value per original pixel
    full = _formula(m, (K1 * R) ** 2, (K2 * R) ** 2)
    return full[PAD:-PAD, PAD:-PAD]


def ssim_map_f32_conv2d(pred, gt, data_range=None):
    """fp32, the reference's arithmetic: F.conv2d of the five stacked inputs with the (11, 11) fp32 window per channel (groups = 3),
    on the valid positions (what remains of the padded result after the crop)."""
    R = data_range_of(pred, gt) if data_range is None else float(data_range)
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(pred, np.float32))).permute(2, 0, 1).unsqueeze(0)
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(gt, np.float32))).permute(2, 0, 1).unsqueeze(0)
    g = torch.from_numpy(gaussian(np.float32)).reshape(1, WIN)
    k = (g.t() @ g).expand(3, 1, WIN, WIN).contiguous()
    x = torch.cat([p, t, p * p, t * t, p * t], 0)
    m = F.conv2d(x, k, groups=3)
    c1, c2 = np.float32((K1 * R) ** 2), np.float32((K2 * R) ** 2)
    return _formula([m[i] for i in range(5)], float(c1), float(c2)).permute(1, 2, 0).numpy()


def ssim_map_f32_separable(pred, gt, data_range=None):
    """fp32 separable: horizontal pass then vertical pass, taps ascending, every product and sum rounded -- the kernel's order."""
    R = data_range_of(pred, gt) if data_range is None else float(data_range)
    p, t = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    g = gaussian(np.float32)
    H, W = p.shape[:2]

    def window(x):
        h = np.zeros((H, W - WIN + 1, 3), np.float32)
        for k in range(WIN):
            h += g[k] * x[:, k:k + W - WIN + 1]
        v = np.zeros((H - WIN + 1, W - WIN + 1, 3), np.float32)
        for j in range(WIN):
            v += g[j] * h[j:j + H - WIN + 1]
        return v

    m = [window(x) for x in (p, t, p * p, t * t, p * t)]
    c1, c2 = np.float32((K1 * R) ** 2), np.float32((K2 * R) ** 2)
    ep, et, epp, ett, ept = m
    pp, tt, pt = ep * ep, et * et, ep * et
    sp, st, spt = epp - pp, ett - tt, ept - pt
    two = np.float32(2.0)
    return ((two * pt + c1) * (two * spt + c2)) / (((pp + tt) + c1) * ((sp + st) + c2))


def ssim(pred, gt, data_range=None):
    return float(ssim_map_f64(pred, gt, data_range).mean())


def sse(pred, gt):
    d = np.asarray(pred, np.float32).astype(np.float64) - np.asarray(gt, np.float32).astype(np.float64)
    return float((d * d).sum())


def psnr(pred, gt):
    """utils/rend_util.py:get_psnr in fp64."""
    mse = sse(pred, gt) / np.asarray(pred).size
    return math.inf if mse == 0.0 else -10.0 * math.log10(mse)


def rgb8_f32(rgb):
    """trunc(clip(rgb * 255, 0, 255)) with the one fp32 multiply of the reference (plots.py:500-501, recon.py:273)."""
    return (np.asarray(rgb, np.float32) * np.float32(255)).clip(0, 255).astype(np.uint8)


def normal_cam_f64(normal, pose):
    """n_cam = pose[:3, :3]^T n, fp64 from the fp32 inputs; normal (P, 3)."""
    R = np.asarray(pose, np.float32).astype(np.float64)[:3, :3]
    return np.asarray(normal, np.float32).astype(np.float64) @ R          # (R^T n)^T = n^T R


def normal8_pre(normal, pose):
    """the fp64 value before truncation: clip((n_cam + 1) / 2 * 255, 0, 255)"""
    return ((normal_cam_f64(normal, pose) + 1.0) / 2.0 * 255.0).clip(0, 255)


def depth8_pre(depth):
    """the fp64 value before truncation: d / (max + 1e-6) * 255, the maximum over the view; fp32 depth, fp32 sum as in plots.py:551"""
    d = np.asarray(depth, np.float32)
    m = np.float64(np.float32(d.max()) + np.float32(1e-6))
    return (d.astype(np.float64) / m * 255.0).clip(0, 255)


def near_integer(pre, tol=1e-4):
    """where truncation is ill-conditioned: the value lies within tol of an integer"""
    return np.abs(pre - np.round(pre)) <= tol


def ratios(num_frames):
    return [math.sin((i / num_frames - 0.5) * math.pi) * 0.5 + 0.5 for i in range(num_frames)]


def _rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def pose_pair(seed, angle_deg, t_scale=4.0):
    """Two fp64 camera-to-world poses whose rotations differ by `angle_deg` about a seeded axis; |t| entries <= t_scale."""
    rng = np.random.default_rng(seed)
    R0 = random_rotation(rng)
    R1 = _rodrigues(rng.standard_normal(3), math.radians(angle_deg)) @ R0
    p0, p1 = np.eye(4), np.eye(4)
    p0[:3, :3], p1[:3, :3] = R0, R1
    p0[:3, 3], p1[:3, 3] = rng.uniform(-t_scale, t_scale, 3), rng.uniform(-t_scale, t_scale, 3)
    return p0, p1


def pose_path_axis_angle(p0, p1, num_frames):
    """The pose path by its definition R(s) = exp(s log(R1 R0^T)) R0 -- log through the eigenvector of eigenvalue 1 (no scipy)."""
    R0, R1 = p0[:3, :3], p1[:3, :3]
    Q = R1 @ R0.T
    w, v = np.linalg.eig(Q)
    axis = np.real(v[:, int(np.argmin(np.abs(w - 1.0)))])
    ang = math.acos(min(1.0, max(-1.0, (np.trace(Q) - 1.0) / 2.0)))
    if np.abs(_rodrigues(axis, ang) - Q).max() > np.abs(_rodrigues(-axis, ang) - Q).max():
        axis = -axis
    out = np.zeros((num_frames, 4, 4))
    for i, s in enumerate(ratios(num_frames)):
        out[i, :3, :3] = _rodrigues(axis, s * ang) @ R0
        out[i, :3, 3] = (1 - s) * p0[:3, 3] + s * p1[:3, 3]
        out[i, 3, 3] = 1.0
    return out


def view_pair(H, W, seed, noise):
    """(pred, gt) fp32 (H W, 3): a smooth sinusoidal rgb pattern with a flat bright patch (0.95) over the top-left H/2 x W/3 -- where
    E[xx] - E[x]^2 cancels worst in fp32; gt is the pattern, pred = clip(gt + noise N(0, 1), 0, 1)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rng.uniform(0, 2 * math.pi, (3, 2))
    fr = rng.uniform(0.05, 0.35, (3, 2))
    gt = np.stack([0.5 + 0.25 * np.sin(fr[c, 0] * x + ph[c, 0]) + 0.2 * np.cos(fr[c, 1] * y + ph[c, 1]) for c in range(3)], -1)
    gt[:H // 2, :W // 3] = 0.95
    pred = np.clip(gt + noise * rng.standard_normal(gt.shape), 0.0, 1.0)
    return pred.reshape(H * W, 3).astype(np.float32), gt.reshape(H * W, 3).astype(np.float32)
