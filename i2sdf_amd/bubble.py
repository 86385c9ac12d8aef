"""Bubble-loss point-cloud PDF: the per-point sampling density the trainer maintains next to the render path.

Mirrors the three methods of VolumeRenderSystem that touch it (model/trainer/recon.py):
  update_pdf           :142-152   value clamp / prune / scatter through the pixel->point links -- here ONE kernel fused with the
                                  error it is fed (i2sdf_pdf_update; the reference spends ~10 launches + an index_put per call)
  sample_bubble        :154-170   uniform or importance sampling of bubble_batch_size points: the reference's torch.multinomial chain by
                                  default, or (sampler="device") ONE stream-ordered i2sdf_bubble_sample call with no host read and no
                                  2^24 limit (a different random stream, the same successive-sampling law)
  initialize_bubble_pdf:172-199   the sweep over every pixel of every training image with model.forward(data, True); here the
                                  rays come from the HBM-resident RayBatcher (no per-ray K / pose stacks) and each split costs one
                                  render + one update launch.
and the part of the data set in front of it (dataset/train_dataset.py:112-141): BubblePDF.from_depth un-projects the depth maps into
the point cloud and builds the pixel<->point links on the device (i2sdf_depth_unproject_*).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch

from . import lib as L_


class BubblePDF:
    """pointcloud (n_points,3), pointlinks (n_images*H*W,) int64 with -1 = no point (dataset/train_dataset.py:105-138)."""

    def __init__(self, pointcloud: torch.Tensor, pointlinks: torch.Tensor, pdf_criterion: str = "DEPTH", pdf_max: Optional[float] = None,
                 pdf_prune: float = 0.0, uniform_bubble: bool = False, device="cuda", sampler: str = "multinomial", seed: Optional[int] = None):
        """sampler: "multinomial" (default) = the reference's eager chain on torch's random stream; "device" = i2sdf_bubble_sample,
        keyed by (seed, self.draws) -- seed defaults to torch.initial_seed().  The ranks of a data-parallel run must pass DIFFERENT
        seeds (e.g. seed + rank): with equal seeds and equal PDFs every rank would draw the same points."""
        assert pdf_criterion in ("RGB", "DEPTH")                         # model/trainer/recon.py:55-56
        if sampler not in ("multinomial", "device"):
            raise ValueError(f"sampler must be 'multinomial' or 'device', not {sampler!r}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L_.I2SDFError("BubblePDF needs a ROCm device (there is no CPU path)")
        self._lib = L_.load()
        self.device = dev
        self.pointcloud = torch.as_tensor(pointcloud).to(dev, torch.float32).contiguous()
        self.pointlinks = torch.as_tensor(pointlinks).to(dev, torch.int64).contiguous()
        self.pdf_criterion, self.pdf_max, self.pdf_prune, self.uniform_bubble = pdf_criterion, pdf_max, float(pdf_prune), uniform_bubble
        self.pdf = torch.zeros(self.pointcloud.shape[0], dtype=torch.float32, device=dev)
        self.sample_count = torch.zeros(self.pointcloud.shape[0], dtype=torch.float32, device=dev)
        self._n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sampler = sampler
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.draws = 0                                                   # calls of the device sampler so far (its 32-bit counter)
        self._short = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws: Dict[int, torch.Tensor] = {}
        self._last_ws: Optional[torch.Tensor] = None
        self.pixlinks = None                                             # from_depth fills these two
        self.depth_masks = None

    @classmethod
    def from_depth(cls, depth_images: torch.Tensor, intrinsics_all: torch.Tensor, pose_all: torch.Tensor, img_res, lo: float = 1e-3,
                   hi: float = 6.0, device="cuda", **kwargs) -> "BubblePDF":
        """The cloud and the links from the depth maps (n_img, H*W), built on the device in the reference's order
        (dataset/train_dataset.py:112-141); `pixlinks` (n_points) and `depth_masks` (n_img, H*W) bool are kept as attributes.
        The remaining arguments are the constructor's."""
        masks, pointlinks, pixlinks, cloud = depth_unproject(depth_images, intrinsics_all, pose_all, img_res, lo, hi, device)
        bp = cls(cloud, pointlinks, device=device, **kwargs)
        bp.pixlinks, bp.depth_masks = pixlinks, masks
        return bp

    def bad_indices(self) -> int:
        return int(self._n_bad.item())

    def shortfall(self) -> int:
        """Rows the device sampler had to repeat because fewer entries than asked for were eligible, summed over its calls
        (+1 per call whose threshold key collided more than batch_size times); reads the device counter."""
        return int(self._short.item())

    def last_passes(self) -> int:
        """Passes over the PDF the latest device draw made (2 to 4: the histogram passes that ran and the collect pass; 0 before the
        first draw).  Reads the draw's workspace, so it waits for the device: for measurements, not for the step."""
        if self._last_ws is None:
            return 0
        o = L_.BUBBLE_WS_PASSES_OFFSET
        return int(self._last_ws[o:o + 4].view(torch.int32).item())

    def sampler_state(self) -> Tuple[int, int]:
        """(seed, draws) of the device sampler, for a checkpoint."""
        return self.seed, self.draws

    def load_sampler_state(self, state) -> None:
        seed, draws = state
        self.seed, self.draws = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draws) & 0xFFFFFFFF

    # ------------------------------------------------------------------------------------------
    def update_pdf(self, model_outputs: Dict[str, torch.Tensor], ground_truth: Dict[str, torch.Tensor], indices=None, first_pixel: int = 0):
        """pdf[pointlinks[indices]] = pruned, clamped error of this batch.  `indices`: global pixel indices (B,), or None for the
        run first_pixel .. first_pixel+B-1."""
        if self.pdf_criterion == "RGB":
            pred, tgt, ch = model_outputs["rgb_values"], ground_truth["rgb"], 3
        else:
            pred, tgt, ch = model_outputs["depth_values"], ground_truth["depth"], 1
        pred = pred.detach().to(torch.float32).reshape(-1, ch).contiguous()
        tgt = tgt.detach().to(self.device, torch.float32).reshape(-1, ch).contiguous()
        if not pred.is_cuda:
            raise L_.I2SDFError("BubblePDF.update_pdf needs device tensors (there is no CPU path)")
        n = pred.shape[0]
        assert tgt.shape[0] == n
        if indices is not None:
            indices = torch.as_tensor(indices).to(self.device, torch.int64).contiguous()
            assert indices.numel() == n
        with torch.cuda.device(self.device):
            L_.check(self._lib.i2sdf_pdf_update(L_.ptr(pred), L_.ptr(tgt), ch, L_.ptr(indices), int(first_pixel), n, L_.ptr(self.pointlinks),
                                                self.pointlinks.numel(), math.nan if self.pdf_max is None else float(self.pdf_max),
                                                self.pdf_prune, L_.ptr(self.pdf), self.pdf.numel(), L_.ptr(self._n_bad), L_.stream_ptr()),
                     "i2sdf_pdf_update")

    def sample_bubble(self, batch_size: int) -> torch.Tensor:
        """model/trainer/recon.py:154-170 (torch.multinomial keeps the reference's random stream and its 2^24 category limit)."""
        if self.sampler == "device":
            return self.sample_bubble_device(batch_size)[1]
        if self.uniform_bubble:
            return self.pointcloud[torch.randperm(self.pointcloud.shape[0], device=self.device)[:batch_size]]
        sample_idx = torch.where(self.pdf > 0)[0]
        if sample_idx.shape[0] >= (1 << 24):
            raise RuntimeError("PDF capacity exceeds the 2^24 category limit of torch.multinomial")
        idx = torch.multinomial(self.pdf[sample_idx], batch_size, replacement=False)
        self.sample_count[sample_idx[idx]] += 1
        return self.pointcloud[sample_idx[idx]]

    def sample_bubble_device(self, batch_size: int):
        """One i2sdf_bubble_sample call on the current stream: (idx (k,) int64, points (k,3)) in the order of the successive draws;
        uniform_bubble passes no weights.  Nothing here waits for the device; self.draws moves on by one."""
        k = int(batch_size)
        if not 1 <= k <= L_.BUBBLE_MAX_K:
            raise L_.I2SDFError(f"the device bubble sampler draws 1..{L_.BUBBLE_MAX_K} points per call, not {k}")
        n = self.pdf.numel()
        if n >= 1 << 31:
            raise L_.I2SDFError("the device bubble sampler indexes fewer than 2^31 points")
        with torch.cuda.device(self.device):
            ws = self._ws.get(k)
            if ws is None:
                ws = self._ws[k] = torch.empty(int(self._lib.i2sdf_bubble_sample_workspace_bytes(k)), dtype=torch.uint8, device=self.device)
            idx = torch.empty(k, dtype=torch.int64, device=self.device)
            pts = torch.empty(k, 3, dtype=torch.float32, device=self.device)
            L_.check(self._lib.i2sdf_bubble_sample(None if self.uniform_bubble else L_.ptr(self.pdf), n, L_.ptr(self.pointcloud), k, self.seed,
                                                   self.draws, L_.ptr(ws), L_.ptr(idx), L_.ptr(pts), L_.ptr(self.sample_count),
                                                   L_.ptr(self._short), L_.stream_ptr()), "i2sdf_bubble_sample")
        self.draws = (self.draws + 1) & 0xFFFFFFFF
        self._last_ws = ws
        return idx, pts

    @torch.no_grad()
    def initialize_bubble_pdf(self, model, batcher, split_size: int, images=None, draws_for=None):
        """The initial sweep: every pixel of every image rendered with model.forward(data, True) in the model's CURRENT mode (the
        reference calls it from training_step, i.e. training mode under no_grad: perturbed sampling, no eikonal / normal outputs)
        and scattered into the PDF.  `batcher`: the RayBatcher holding the training views.  `draws_for(image, first_pixel, n)`
        may return the sampler draws to use (tests)."""
        tp = batcher.total_pixels
        for i in (range(batcher.n_images) if images is None else images):
            for lo in range(0, tp, split_size):
                n = min(split_size, tp - lo)
                tidx = torch.arange(i * tp + lo, i * tp + lo + n, dtype=torch.int64, device=self.device)
                _, _, sample, gt = batcher.batch(tidx)
                out = model(sample, True) if draws_for is None else model(sample, True, draws=draws_for(i, lo, n))
                self.update_pdf(out, gt, None, first_pixel=i * tp + lo)


def depth_unproject(depth_images: torch.Tensor, intrinsics_all: torch.Tensor, pose_all: torch.Tensor, img_res, lo: float = 1e-3,
                    hi: float = 6.0, device="cuda"):
    """(depth_masks (n_img, H*W) bool, pointlinks (n_img*H*W,) int64, pixlinks (n_points,) int64, pointcloud (n_points, 3)) of the
    depth maps: dataset/train_dataset.py:112-141 as a stream compaction on the device.  One host read (n_points sizes the outputs)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L_.I2SDFError("depth_unproject needs a ROCm device (there is no CPU path)")
    lib = L_.load()
    H, W = int(img_res[0]), int(img_res[1])
    depth = torch.as_tensor(depth_images).to(dev, torch.float32).contiguous()
    n_img = depth.shape[0] if depth.dim() > 1 else 1
    if depth.numel() != n_img * H * W:
        raise ValueError(f"depth_images holds {depth.numel()} values, not {n_img} x {H} x {W}")
    K = torch.as_tensor(intrinsics_all).to(dev, torch.float32).reshape(-1, 4, 4).contiguous()
    pose = torch.as_tensor(pose_all).to(dev, torch.float32).reshape(-1, 4, 4).contiguous()
    if K.shape[0] != n_img or pose.shape[0] != n_img:
        raise ValueError(f"{n_img} depth maps need {n_img} intrinsics and poses (4x4), got {K.shape[0]} and {pose.shape[0]}")
    with torch.cuda.device(dev):
        nbytes = int(lib.i2sdf_depth_unproject_workspace_bytes(n_img, H, W))
        if nbytes == 0:
            raise L_.I2SDFError(f"depth_unproject: unsupported size {n_img} x {H} x {W}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        masks = torch.empty(n_img, H * W, dtype=torch.bool, device=dev)
        links = torch.empty(n_img * H * W, dtype=torch.int64, device=dev)
        n_points = C.c_int64(0)
        L_.check(lib.i2sdf_depth_unproject_count(L_.ptr(depth), n_img, H, W, lo, hi, L_.ptr(ws), L_.ptr(masks), C.byref(n_points), L_.stream_ptr()),
                 "i2sdf_depth_unproject_count")
        pix = torch.empty(n_points.value, dtype=torch.int64, device=dev)
        cloud = torch.empty(n_points.value, 3, dtype=torch.float32, device=dev)
        L_.check(lib.i2sdf_depth_unproject_write(L_.ptr(depth), L_.ptr(K), L_.ptr(pose), n_img, H, W, lo, hi, L_.ptr(ws), n_points.value,
                                                 L_.ptr(links), L_.ptr(pix), L_.ptr(cloud), L_.stream_ptr()), "i2sdf_depth_unproject_write")
    return masks, links, pix, cloud
