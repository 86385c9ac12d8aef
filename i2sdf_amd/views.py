"""Rendered views on the device (csrc/imgops.hip; include/i2sdf.h, "Rendered views"): what the reference's test-time image branch
does with a finished view -- PSNR and SSIM (model/eval/recon.py:197-201), the camera-space normal map (:184-189, :276-280), the
8-bit frames its writers get (utils/plots.py:492-506, :538-555; recon.py:272-273) and the camera path of a view interpolation
(dataset/eval_dataset.py:213-241).

HDR data (`is_hdr: True`): the reference tone-maps prediction and ground truth with `rend_util.linear_to_srgb(x.clamp(0, 1))` before the
metrics and the 8-bit images and keeps the raw values beside them (model/trainer/recon.py:320-350): `linear_to_srgb`, and `hdr=True` of
`psnr` / `ssim` / `image_metrics` / `to_frames`, which run it into a scratch stack first -- the same kernels then see the same numbers as
after an explicit `linear_to_srgb` call, bit for bit.

Images keep the render outputs' layout: (H W, C) or (n_views, H W, C) fp32 on the device, pixel p = y W + x; `img_res` = (H, W).
There is no CPU path: a CPU tensor raises ValueError before the library is loaded.  Nothing here synchronises with the host.

Restated, not checked against the libraries (none of them is available where this project is built): SSIM follows the source of
torchmetrics 0.11.4 (`structural_similarity_index_measure` with its defaults) and is tested against tests/views_ref.py and closed forms.
Not imitated: LPIPS, cv2's colour-map tables (pass your own `lut`), PNG / EXR / video writing."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import lib as L

SSIM_WINDOW = 11


def _res(img_res, what, min_side=1):
    try:
        H, W = (int(v) for v in img_res)
    except Exception:
        raise ValueError(f"{what}: img_res must be (H, W)")
    if H < min_side or W < min_side or H * W > 2 ** 31 - 1:
        raise ValueError(f"{what}: H and W must be at least {min_side} with H * W < 2^31 (got {H}, {W})")
    return H, W


def _stack(t, hw, c, what, name):
    """(n, hw, c) contiguous fp32 view of a device image or image stack."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a tensor on a GPU (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if c == 1 and t.dim() >= 1 and t.shape[-1] == hw and t.dim() <= 2:      # depth as (HW,) or (n, HW): the render's own shape
        t = t.unsqueeze(-1)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[1] != hw or t.shape[2] != c:
        raise ValueError(f"{what}: {name} must be ({hw}, {c}) or (n, {hw}, {c}), got {tuple(t.shape)}")
    if t.shape[0] > 65535:
        raise ValueError(f"{what}: at most 65535 views")
    return t.detach().contiguous()


def _pair(pred, gt, img_res, what, min_side=1):
    H, W = _res(img_res, what, min_side)
    p, g = _stack(pred, H * W, 3, what, "pred"), _stack(gt, H * W, 3, what, "gt")
    if p.shape != g.shape or p.device != g.device:
        raise ValueError(f"{what}: pred {tuple(p.shape)} on {p.device} and gt {tuple(g.shape)} on {g.device} do not match")
    return p, g, H, W


def _workspace(lib, n, H, W, dev):
    nbytes = int(lib.i2sdf_image_workspace_bytes(n, H, W))
    if nbytes <= 0:
        raise ValueError(f"image size not supported: {n} views of {H} x {W}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _stats(lib, pred, gt, depth, n, H, W, ws):
    """(n, 8) fp64: sum of squared differences, min / max of pred, min / max of gt, max of depth."""
    stats = torch.empty(n, L.IMAGE_STATS, dtype=torch.float64, device=ws.device)
    L.check(lib.i2sdf_image_stats(L.ptr(pred), L.ptr(gt), L.ptr(depth), n, H, W, L.ptr(ws), L.ptr(stats), L.stream_ptr()),
            "i2sdf_image_stats")
    return stats


def _psnr_of(stats, H, W):
    return -10.0 * torch.log10(stats[:, 0] / (3.0 * H * W))


def _data_range(data_range, what):
    if data_range is None:
        return float("nan")
    r = float(data_range)
    if not (0.0 < r < float("inf")):
        raise ValueError(f"{what}: data_range must be finite and positive (or None), got {data_range!r}")
    return r


def _ssim_of(lib, pred, gt, n, H, W, data_range, stats, ws, return_map):
    dev = pred.device
    out = torch.empty(n, dtype=torch.float64, device=dev)
    smap = torch.empty(n, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1, 3, dtype=torch.float32, device=dev) if return_map else None
    L.check(lib.i2sdf_image_ssim(L.ptr(pred), L.ptr(gt), n, H, W, data_range, L.ptr(stats), L.ptr(ws), L.ptr(out), L.ptr(smap),
                                 L.stream_ptr()), "i2sdf_image_ssim")
    return out, smap


@torch.no_grad()
def linear_to_srgb(x, clamp: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """utils/rend_util.py:linear_to_srgb on the device, elementwise, any shape: x <= 0.0031308 ? 12.92 x : 1.055 x^(1/2.4) - 0.055, with
    `clamp` (the default: what the reference's validation does with HDR images) on clamp(x, 0, 1).  0 maps to 0 and, clamped, everything
    from 1 up to 1, exactly.  Returns a new fp32 tensor, or `out` (same shape, contiguous fp32, same device; `out is x` tone-maps in place)."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("linear_to_srgb: x must be a tensor on a GPU (there is no CPU path)")
    if x.dtype != torch.float32:
        raise ValueError(f"linear_to_srgb: x must be float32, got {x.dtype}")
    src = x.detach().contiguous()
    if out is None:
        out = torch.empty_like(src)
    elif not torch.is_tensor(out) or out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError("linear_to_srgb: out must be a contiguous float32 tensor of x's shape on x's device")
    if src.numel():
        with torch.cuda.device(src.device):
            L.check(L.load().i2sdf_linear_to_srgb(L.ptr(src), L.ptr(out), src.numel(), int(bool(clamp)), L.stream_ptr()),
                    "i2sdf_linear_to_srgb")
    return out


def _tone(hdr, *imgs):
    """the images as the metrics and frames see them: tone-mapped copies (clamped, as get_plot_data does) with `hdr`, else as they are"""
    return tuple(linear_to_srgb(t, True) if (hdr and t is not None) else t for t in imgs)


@torch.no_grad()
def image_stats(pred, gt, img_res, depth=None) -> torch.Tensor:
    """(n, 8) fp64 device: [0] sum over the 3 H W values of (pred - gt)^2 in fp64, [1:3] min, max of pred, [3:5] min, max of gt,
    [5] max of `depth` (-inf without one).  One pass; bitwise reproducible."""
    p, g, H, W = _pair(pred, gt, img_res, "image_stats")
    n = p.shape[0]
    d = None if depth is None else _stack(depth, H * W, 1, "image_stats", "depth")
    if d is not None and d.shape[0] != n:
        raise ValueError(f"image_stats: {d.shape[0]} depth maps for {n} views")
    if n == 0:
        return torch.empty(0, L.IMAGE_STATS, dtype=torch.float64, device=p.device)
    lib = L.load()
    with torch.cuda.device(p.device):
        return _stats(lib, p, g, d, n, H, W, _workspace(lib, n, H, W, p.device))


@torch.no_grad()
def psnr(pred, gt, img_res, hdr: bool = False) -> torch.Tensor:
    """(n,) fp64 device: -10 log10(mean((pred - gt)^2)) per view (utils/rend_util.py:get_psnr, which takes the mean in fp32; here the
    differences, squares and sums are fp64).  +inf for identical images, as in the reference.  Any size from 1 x 1.
    hdr: of linear_to_srgb(clamp(., 0, 1)) of both images."""
    H, W = _res(img_res, "psnr")
    p, g, _, _ = _pair(pred, gt, img_res, "psnr")
    p, g = _tone(hdr, p, g)
    return _psnr_of(image_stats(p, g, img_res), H, W)


@torch.no_grad()
def ssim(pred, gt, img_res, data_range: Optional[float] = None, return_map: bool = False, hdr: bool = False):
    """(n,) fp64 device: the SSIM of torchmetrics 0.11.4 with the reference's defaults (Gaussian window of 11 taps, sigma 1.5), per
    view -- the definition is written out in include/i2sdf.h.  `data_range` None: max(max pred - min pred, max gt - min gt) of each
    view, taken on the device (what torchmetrics does for the one-view batch the reference passes).  H, W >= 11.
    return_map: also the (n, H - 10, W - 10, 3) fp32 per-pixel values; the mean is bit-identical either way.
    hdr: of linear_to_srgb(clamp(., 0, 1)) of both images."""
    p, g, H, W = _pair(pred, gt, img_res, "ssim", SSIM_WINDOW)
    p, g = _tone(hdr, p, g)
    r = _data_range(data_range, "ssim")
    n, dev = p.shape[0], p.device
    if n == 0:
        e = torch.empty(0, dtype=torch.float64, device=dev)
        return (e, torch.empty(0, H - 10, W - 10, 3, dtype=torch.float32, device=dev)) if return_map else e
    lib = L.load()
    with torch.cuda.device(dev):
        ws = _workspace(lib, n, H, W, dev)
        stats = _stats(lib, p, g, None, n, H, W, ws) if data_range is None else None
        out, smap = _ssim_of(lib, p, g, n, H, W, r, stats, ws, return_map)
    return (out, smap) if return_map else out


@torch.no_grad()
def image_metrics(pred, gt, img_res, data_range: Optional[float] = None, hdr: bool = False) -> dict:
    """{"psnr": (n,) fp64, "ssim": (n,) fp64} on the device: one stats pass serves both (the squared error for PSNR, the value range
    for SSIM).  H, W >= 11.  hdr: both images go through linear_to_srgb(clamp(., 0, 1)) first (model/trainer/recon.py: get_plot_data
    with is_hdr); bit-identical to image_metrics(linear_to_srgb(pred), linear_to_srgb(gt), ...)."""
    p, g, H, W = _pair(pred, gt, img_res, "image_metrics", SSIM_WINDOW)
    p, g = _tone(hdr, p, g)
    r = _data_range(data_range, "image_metrics")
    n, dev = p.shape[0], p.device
    if n == 0:
        e = torch.empty(0, dtype=torch.float64, device=dev)
        return {"psnr": e, "ssim": e.clone()}
    lib = L.load()
    with torch.cuda.device(dev):
        ws = _workspace(lib, n, H, W, dev)
        stats = _stats(lib, p, g, None, n, H, W, ws)
        out, _ = _ssim_of(lib, p, g, n, H, W, r, stats, ws, False)
    return {"psnr": _psnr_of(stats, H, W), "ssim": out}


@torch.no_grad()
def to_frames(rgb=None, normal_map=None, depth=None, pose=None, img_res=None, lut=None, camera_normals: bool = False,
              hdr: bool = False) -> dict:
    """The 8-bit images the reference hands to its writers, as uint8 device tensors (n, H, W, C); a key per input given:
      "rgb8"        trunc(clip(rgb * 255, 0, 255))                                     (plots.py:500-501, recon.py:273)
                    hdr=True: of linear_to_srgb(clamp(rgb, 0, 1)); the other frames do not change
      "normal8"     from the WORLD-space `normal_map` and `pose` ((4, 4) or (n, 4, 4), camera-to-world): n_cam = pose[:3, :3]^T n
                    (recon.py:184-186), then trunc(clip((n_cam + 1) / 2 * 255, 0, 255)); camera_normals=True adds "normal_cam",
                    the fp32 (n, H W, 3) map the reference writes as .exr
      "depth8"      trunc(depth / (max over the view + 1e-6) * 255)                     (plots.py:551-552); the maximum is taken on the device
      "depth_rgb8"  lut[depth8] when a (256, 3) uint8 device table is passed: the slot for a colour map (none is shipped)"""
    H, W = _res(img_res, "to_frames")
    hw = H * W
    r = None if rgb is None else _stack(rgb, hw, 3, "to_frames", "rgb")
    r, = _tone(hdr, r)
    nm = None if normal_map is None else _stack(normal_map, hw, 3, "to_frames", "normal_map")
    d = None if depth is None else _stack(depth, hw, 1, "to_frames", "depth")
    given = [t for t in (r, nm, d) if t is not None]
    if not given:
        raise ValueError("to_frames: give at least one of rgb, normal_map, depth")
    n, dev = given[0].shape[0], given[0].device
    if any(t.shape[0] != n or t.device != dev for t in given):
        raise ValueError("to_frames: the inputs must hold the same number of views on one device")
    if nm is not None:
        if pose is None:
            raise ValueError("to_frames: normal_map needs the views' poses")
        pose = torch.as_tensor(pose).detach().to(dev, torch.float32)
        pose = pose.reshape(1, 4, 4).expand(n, 4, 4) if pose.dim() == 2 else pose
        if tuple(pose.shape) != (n, 4, 4):
            raise ValueError(f"to_frames: pose must be (4, 4) or ({n}, 4, 4), got {tuple(pose.shape)}")
        pose = pose.contiguous()
    if lut is not None:
        if not torch.is_tensor(lut) or not lut.is_cuda or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError("to_frames: lut must be a (256, 3) uint8 tensor on a GPU")
        lut = lut.to(dev).contiguous()
    u8 = lambda c: torch.empty(n, H, W, c, dtype=torch.uint8, device=dev)
    out = {}
    if r is not None:
        out["rgb8"] = u8(3)
    if nm is not None:
        out["normal8"] = u8(3)
        if camera_normals:
            out["normal_cam"] = torch.empty(n, hw, 3, dtype=torch.float32, device=dev)
    if d is not None:
        out["depth8"] = u8(1)
        if lut is not None:
            out["depth_rgb8"] = u8(3)
    if n == 0:
        return out
    lib = L.load()
    with torch.cuda.device(dev):
        stats = _stats(lib, None, None, d, n, H, W, _workspace(lib, n, H, W, dev)) if d is not None else None
        L.check(lib.i2sdf_image_frames(L.ptr(r), L.ptr(nm), L.ptr(d), L.ptr(pose if nm is not None else None), L.ptr(stats),
                                       L.ptr(lut if d is not None else None), n, H, W, L.ptr(out.get("rgb8")), L.ptr(out.get("normal8")),
                                       L.ptr(out.get("normal_cam")), L.ptr(out.get("depth8")), L.ptr(out.get("depth_rgb8")),
                                       L.stream_ptr()), "i2sdf_image_frames")
    return out


def _rotation_vector(Q):
    """log of a rotation matrix as angle * axis, angle in [0, pi]: through the unit quaternion (largest-component rule), which stays
    accurate near pi where the antisymmetric part vanishes."""
    tr = Q[0, 0] + Q[1, 1] + Q[2, 2]
    cand = np.array([tr, Q[0, 0], Q[1, 1], Q[2, 2]])
    k = int(np.argmax(cand))
    if k == 0:
        q = np.array([1.0 + tr, Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])          # (w, x, y, z)
    else:
        i, j, l = k - 1, k % 3, (k + 1) % 3
        v = np.zeros(3)
        v[i] = 1.0 - tr + 2.0 * Q[i, i]
        v[j] = Q[j, i] + Q[i, j]
        v[l] = Q[l, i] + Q[i, l]
        q = np.array([Q[l, j] - Q[j, l], v[0], v[1], v[2]])
    q = q / np.linalg.norm(q)
    if q[0] < 0.0:
        q = -q                                       # the shortest arc
    s = np.linalg.norm(q[1:])
    if s == 0.0:
        return np.zeros(3)
    return (2.0 * math.atan2(s, q[0]) / s) * q[1:]


def _rotation_exp(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    a = w / th
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def interpolate_poses(pose0, pose1, num_frames: int) -> torch.Tensor:
    """(num_frames, 4, 4) fp32 CPU: the camera path of InterpolateDataset (dataset/eval_dataset.py:219-240) between two camera-to-world
    poses.  ratio_i = sin((i / num_frames - 0.5) pi) / 2 + 1 / 2 (eases in and out; the last frame stops short of pose1, as there),
    translation (1 - ratio) t0 + ratio t1, rotation R(s) = exp(s log(R1 R0^T)) R0 along the shortest arc -- what scipy's Slerp gives
    on the transposed rotations, transposed back.  Host arithmetic in fp64, rounded to fp32 once; no kernel."""
    num_frames = int(num_frames)
    if num_frames < 1:
        raise ValueError(f"interpolate_poses: num_frames must be at least 1, got {num_frames}")
    p0, p1 = (np.asarray(torch.as_tensor(p).detach().cpu().to(torch.float64).numpy()) for p in (pose0, pose1))
    if p0.shape != (4, 4) or p1.shape != (4, 4) or not (np.isfinite(p0).all() and np.isfinite(p1).all()):
        raise ValueError("interpolate_poses: poses must be finite (4, 4) matrices")
    R0, R1 = p0[:3, :3], p1[:3, :3]
    w = _rotation_vector(R1 @ R0.T)
    out = np.zeros((num_frames, 4, 4))
    for i in range(num_frames):
        ratio = math.sin((i / num_frames - 0.5) * math.pi) * 0.5 + 0.5
        out[i, :3, :3] = _rotation_exp(ratio * w) @ R0
        out[i, :3, 3] = (1.0 - ratio) * p0[:3, 3] + ratio * p1[:3, 3]
        out[i, 3, 3] = 1.0
    return torch.from_numpy(out).to(torch.float32)


def pixel_grid(H: int, W: int, device=None) -> torch.Tensor:
    """(1, H W, 2) float: the uv grid of PlotDataset.get_uv / InterpolateDataset.__getitem__ -- x fastest, (x, y) order."""
    ys, xs = torch.meshgrid(torch.arange(int(H), device=device), torch.arange(int(W), device=device), indexing="ij")
    return torch.stack([xs, ys], -1).to(torch.float32).reshape(1, -1, 2)
