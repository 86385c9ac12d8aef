"""GPU: the point cloud and the pixel<->point links from the depth maps (i2sdf_depth_unproject_*, BubblePDF.from_depth) against the
reference's own (tests/golden/g17_bubble_cloud.npz) and against the numpy restatement at odd sizes; update_pdf through the built links."""
import numpy as np
import pytest
import torch

import bubble_ref as R

pytestmark = pytest.mark.gpu


def _check(bp, masks, pointlinks, pixlinks, cloud):
    assert bp.depth_masks.dtype == torch.bool and np.array_equal(bp.depth_masks.cpu().numpy(), masks)
    assert np.array_equal(bp.pointlinks.cpu().numpy(), pointlinks) and np.array_equal(bp.pixlinks.cpu().numpy(), pixlinks)
    got = bp.pointcloud.cpu().numpy().astype(np.float64)
    assert got.shape == cloud.shape
    if cloud.size:
        err = np.abs(got - cloud).max() / np.abs(cloud).max()
        print(f"point cloud: {cloud.shape[0]} points, max error {err:.2e} of the largest coordinate")
        assert err <= 1e-5
    assert bp.pdf.shape == (cloud.shape[0],) and bp.sample_count.shape == (cloud.shape[0],)


def test_from_depth_matches_the_reference(golden):
    from i2sdf_amd import BubblePDF
    z = golden("g17_bubble_cloud")
    H, W = int(z["H"]), int(z["W"])
    bp = BubblePDF.from_depth(torch.from_numpy(z["depth"]), torch.from_numpy(z["intrinsics"]), torch.from_numpy(z["pose"]), (H, W),
                              pdf_criterion="DEPTH", pdf_prune=0.1)
    assert bp.pdf_prune == 0.1 and bp.sampler == "multinomial"
    _check(bp, z["depth_masks"], z["pointlinks"], z["pixlinks"], z["pointcloud"].astype(np.float64))


def _views(n_img, H, W, seed):
    g = np.random.default_rng(seed)
    depth = g.uniform(0.2, 7.0, (n_img, H * W)).astype(np.float32)           # some above hi = 6
    depth[g.uniform(size=depth.shape) < 0.2] = 0.0
    depth[0, 5], depth[0, 6] = np.nan, np.inf
    K = np.tile(np.eye(4, dtype=np.float32), (n_img, 1, 1))
    K[:, 0, 0], K[:, 1, 1] = g.uniform(30, 50, n_img), g.uniform(30, 50, n_img)
    K[:, 0, 2], K[:, 1, 2], K[:, 0, 1] = W / 2 + 0.3, H / 2 - 0.4, g.uniform(-1, 1, n_img)
    pose = np.tile(np.eye(4, dtype=np.float32), (n_img, 1, 1))
    q, _ = np.linalg.qr(g.normal(size=(n_img, 3, 3)))
    pose[:, :3, :3], pose[:, :3, 3] = q, g.uniform(-2, 2, (n_img, 3))
    return depth, K, pose


def test_from_depth_matches_the_restatement_at_odd_sizes():
    """3 views of 33 x 47 (odd, more than one block per view, blocks that straddle two views), one view entirely invalid."""
    from i2sdf_amd import BubblePDF
    H, W = 33, 47
    depth, K, pose = _views(3, H, W, 5)
    depth[1] = 0.0
    want = R.depth_unproject(depth, K, pose, H, W)
    assert not want[0][1].any() and want[0][0].any() and want[0][2].any()
    bp = BubblePDF.from_depth(torch.from_numpy(depth), torch.from_numpy(K), torch.from_numpy(pose), (H, W))
    _check(bp, *want)
    # no valid pixel at all: an empty cloud, every link -1
    empty = BubblePDF.from_depth(torch.zeros(2, H * W), torch.from_numpy(K[:2]), torch.from_numpy(pose[:2]), (H, W))
    assert empty.pointcloud.shape == (0, 3) and empty.pixlinks.shape == (0,) and bool((empty.pointlinks == -1).all())
    # other bounds
    want = R.depth_unproject(depth, K, pose, H, W, lo=1.0, hi=3.0)
    bp = BubblePDF.from_depth(torch.from_numpy(depth), torch.from_numpy(K), torch.from_numpy(pose), (H, W), lo=1.0, hi=3.0)
    _check(bp, *want)


def test_update_pdf_through_the_built_links_writes_exactly_the_linked_points():
    from i2sdf_amd import BubblePDF
    H, W = 33, 47
    depth, K, pose = _views(2, H, W, 9)
    bp = BubblePDF.from_depth(torch.from_numpy(depth), torch.from_numpy(K), torch.from_numpy(pose), (H, W), pdf_criterion="DEPTH")
    bp.pdf.fill_(-1.0)
    g = torch.Generator().manual_seed(1)
    pix = torch.randperm(2 * H * W, generator=g)[:300].cuda()
    pred, tgt = torch.rand(300, generator=g).cuda() + 2.0, torch.rand(300, generator=g).cuda()
    bp.update_pdf({"depth_values": pred}, {"depth": tgt}, pix)
    links = bp.pointlinks[pix]
    hit = links[links >= 0]
    assert 0 < hit.numel() < 300
    assert torch.equal(bp.pixlinks[hit], pix[links >= 0])                   # the two link tables are inverse to each other
    want = torch.full_like(bp.pdf, -1.0)
    want[hit] = (pred - tgt).abs()[links >= 0]
    assert torch.equal(bp.pdf, want) and bp.bad_indices() == 0
