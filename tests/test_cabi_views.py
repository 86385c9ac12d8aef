"""CPU: the rendered-view entry points of the C ABI (i2sdf_image_*, csrc/imgops.hip) on the cross-compiled library: declared, exported
and bound; the size query monotone and 0 for what is not supported; bad arguments refused on the host before any launch (no call below
reaches a launch: a launch without a device would return the HIP error code -2, not -1)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMAGE = ["i2sdf_image_workspace_bytes", "i2sdf_image_stats", "i2sdf_image_ssim", "i2sdf_image_frames"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from i2sdf_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, check=True)
    return L


def test_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "i2sdf.h")).read()
    for name, value in (("I2SDF_IMAGE_STATS", lib.IMAGE_STATS), ("I2SDF_SSIM_TILE_X", lib.SSIM_TILE_X), ("I2SDF_SSIM_TILE_Y", lib.SSIM_TILE_Y)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == value, name
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(i2sdf_image_[a-z0-9_]+)\s*\(", text)) == set(IMAGE)
    raw = C.CDLL(lib.LIB_PATH)
    for s in IMAGE:
        assert hasattr(raw, s), f"{s} declared in include/i2sdf.h but not exported"
        assert s in lib.SIGNATURES, f"{s} has no ctypes signature in i2sdf_amd/lib.py"
    assert "imgops.hip" in open(os.path.join(ROOT, "i2sdf_amd", "csrc", "build.sh")).read()
    import i2sdf_amd
    for name in ("psnr", "ssim", "image_metrics", "to_frames", "interpolate_poses", "pixel_grid"):
        assert callable(getattr(i2sdf_amd, name)), name
    for name in ("evaluate_views", "render_path"):
        assert callable(getattr(i2sdf_amd.I2SDFNetwork, name)), name


def test_workspace_query_is_monotone_and_zero_for_unsupported_sizes(lib):
    h = lib.load()
    ws = lambda n, H, W: int(h.i2sdf_image_workspace_bytes(n, H, W))
    sides = [1, 2, 10, 11, 12, 26, 27, 42, 43, 100, 480, 640, 4096, 46340]
    for n in (1, 3, 20, 65535):
        for other in (1, 11, 59, 480):
            by_h = [ws(n, s, other) for s in sides]
            by_w = [ws(n, other, s) for s in sides]
            assert all(g > 0 for g in by_h + by_w), (n, other)
            assert all(b >= a for a, b in zip(by_h, by_h[1:])), by_h
            assert all(b >= a for a, b in zip(by_w, by_w[1:])), by_w
    for H, W in ((1, 1), (11, 11), (480, 640)):
        got = [ws(n, H, W) for n in (1, 2, 3, 20, 1000, 65535)]
        assert all(b > a for a, b in zip(got, got[1:])), got
    # one fp64 slot per SSIM tile of the result and view, next to the stats slots
    tiles = lambda H, W: -(-(H - 10) // lib.SSIM_TILE_Y) * -(-(W - 10) // lib.SSIM_TILE_X)
    assert ws(2, 480, 640) - ws(2, 480, 10) >= 2 * 8 * tiles(480, 640)
    assert ws(1, 480, 640) < 1 << 16                       # a view needs a few KiB, not an image
    for bad in ((0, 48, 64), (-1, 48, 64), (65536, 48, 64), (1, 0, 64), (1, 48, 0), (1, -48, 64), (1, 48, -1), (1, 1 << 16, 1 << 15),
                (1, 1 << 30, 4)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1 << 15, (1 << 16) - 1) > 0               # H W = 2^31 - 2^15: the largest sizes are answered without overflow


def test_bad_arguments_return_einval_before_any_launch(lib):
    h = lib.load()
    P, N = C.c_void_p(4096), None

    # stats: pred, gt, depth, n_views, H, W, workspace, stats, stream
    def stats(pred=P, gt=P, depth=P, n=2, H=48, W=64, ws=P, out=P):
        return h.i2sdf_image_stats(pred, gt, depth, n, H, W, ws, out, N)

    assert stats(n=0) == 0 and stats(n=0, ws=N, out=N) == 0                    # no views: nothing to do
    sizes = (dict(n=-1), dict(n=65536), dict(H=0), dict(W=0), dict(H=-3), dict(W=-3), dict(H=1 << 16, W=1 << 15))
    for kw in sizes + (dict(ws=N), dict(out=N), dict(pred=N), dict(gt=N), dict(pred=N, gt=N, depth=N)):
        assert stats(**kw) == -1, kw
    for kw in sizes:
        assert stats(n=0, **{k: v for k, v in kw.items() if k != "n"}) == (0 if "n" in kw else -1), kw

    # ssim: pred, gt, n_views, H, W, data_range, stats, workspace, ssim, map, stream
    def ssim(pred=P, gt=P, n=2, H=48, W=64, R=1.0, st=P, ws=P, out=P, smap=N):
        return h.i2sdf_image_ssim(pred, gt, n, H, W, R, st, ws, out, smap, N)

    assert ssim(n=0) == 0 and ssim(n=0, R=NAN, st=N, ws=N, out=N) == 0
    for kw in sizes + (dict(H=10), dict(W=10), dict(H=10, W=10), dict(H=1, W=1), dict(pred=N), dict(gt=N), dict(ws=N), dict(out=N),
                       dict(R=0.0), dict(R=-1.0), dict(R=INF), dict(R=-INF), dict(R=NAN, st=N)):
        assert ssim(**kw) == -1, kw
    for R in (0.0, -1.0, INF):
        assert ssim(n=0, R=R) == -1                                          # (refused even with nothing to do)

    # frames: rgb, normal, depth, pose, stats, lut, n_views, H, W, rgb8, normal8, normal_cam, depth8, depth_rgb8, stream
    def frames(rgb=P, normal=P, depth=P, pose=P, st=P, lut=P, n=2, H=48, W=64, rgb8=P, normal8=P, ncam=P, depth8=P, drgb8=P):
        return h.i2sdf_image_frames(rgb, normal, depth, pose, st, lut, n, H, W, rgb8, normal8, ncam, depth8, drgb8, N)

    assert frames(n=0) == 0
    assert frames(rgb8=N, normal8=N, ncam=N, depth8=N, drgb8=N) == 0          # no output asked for: nothing is launched
    assert frames(rgb=N, normal=N, depth=N, pose=N, st=N, lut=N, rgb8=N, normal8=N, ncam=N, depth8=N, drgb8=N) == 0
    for kw in sizes + (dict(rgb=N), dict(normal=N), dict(pose=N), dict(depth=N), dict(st=N), dict(lut=N),
                       dict(normal=N, normal8=N), dict(pose=N, ncam=N), dict(depth=N, depth8=N), dict(st=N, drgb8=N)):
        assert frames(**kw) == -1, kw
    only = dict(rgb8=N, normal8=N, ncam=N, depth8=N, drgb8=N)
    assert frames(**{**only, "rgb8": P, "rgb": N}) == -1
    assert frames(**{**only, "drgb8": P, "lut": N}) == -1


def test_python_front_end_refuses_bad_arguments_without_a_gpu():
    """The image arguments come first and must be device tensors, so a CPU tensor raises ValueError before the library is even loaded;
    so does an image smaller than the SSIM window."""
    import torch
    import i2sdf_amd as A
    x = torch.zeros(48 * 64, 3)
    for fn in (A.psnr, A.ssim, A.image_metrics, A.image_stats):
        with pytest.raises(ValueError):
            fn(x, x, (48, 64))
    with pytest.raises(ValueError):
        A.to_frames(rgb=x, img_res=(48, 64))
    with pytest.raises(ValueError):
        A.to_frames(depth=torch.zeros(48 * 64, 1), img_res=(48, 64))
    with pytest.raises(ValueError):
        A.to_frames(img_res=(48, 64))
    small = torch.zeros(10 * 64, 3)
    for H, W in ((10, 64), (64, 10)):
        with pytest.raises(ValueError, match="at least 11"):
            A.ssim(small, small, (H, W))
        with pytest.raises(ValueError, match="at least 11"):
            A.image_metrics(small, small, (H, W))
    with pytest.raises(ValueError):
        A.ssim(x, x, (48, 64), data_range=0.0)
    with pytest.raises(ValueError):
        A.ssim(x, x, (48, 64), data_range=float("inf"))
    net = A.I2SDFNetwork(A.plumbing_conf())
    with pytest.raises(ValueError):
        net.evaluate_views(torch.eye(4)[None], torch.eye(4), (24, 32), gt_rgb=torch.zeros(1, 24 * 32, 3))
