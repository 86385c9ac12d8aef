"""Generates tests/golden/g17_bubble_cloud.npz: the bubble point cloud and the pixel<->point links of two small views, from the live
reference's `depth_to_world` (utils/rend_util.py:81-89, imported through tests/golden/ref_import.py) with the data set's link loop
(dataset/train_dataset.py:112-141) restated around it -- the data set itself reads image files from a directory.

Two views of 5 x 7 pixels with skewed intrinsics; the depths include 0, values above 6 (both outside the reference's 1e-3 < d < 6) and
one NaN.  Run on a machine that has the reference:  python tests/golden/gen_bubble_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402


def main():
    _, ref_utils = ref_import.import_reference()
    H, W, n_img = 5, 7, 2
    total = H * W
    g = torch.Generator().manual_seed(17)
    depth = torch.rand(n_img, total, generator=g) * 5.0 + 0.5
    depth[0, 3] = 0.0
    depth[0, 11] = 6.5
    depth[0, 20] = float("nan")
    depth[1, 0] = 0.0
    depth[1, 17] = 9.0
    depth[1, 34] = 0.0005
    K = torch.eye(4).repeat(n_img, 1, 1)
    K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2], K[0, 0, 1] = 9.0, 8.5, 3.4, 2.3, 0.6
    K[1, 0, 0], K[1, 1, 1], K[1, 0, 2], K[1, 1, 2], K[1, 0, 1] = 7.5, 8.0, 3.6, 2.6, -0.4
    pose = torch.eye(4).repeat(n_img, 1, 1)
    for i, (axis, ang, t) in enumerate((((0.2, 1.0, 0.1), 0.4, (0.1, -0.2, -1.5)), ((1.0, -0.3, 0.5), -0.7, (-0.4, 0.3, 1.2)))):
        a = torch.tensor(axis) / torch.tensor(axis).norm()
        A = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        pose[i, :3, :3] = torch.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * (A @ A)
        pose[i, :3, 3] = torch.tensor(t)
    # the data set's pixel grid is (x, y) = (column, row) in row-major pixel order: u = p mod W, v = p div W
    p = torch.arange(total)
    uv = torch.stack([p % W, p // W], 1).float()
    # the links as the data set defines them: points are numbered image by image, in pixel order, over the pixels with 1e-3 < d < 6
    masks = (depth > 1e-3) & (depth < 6)
    flat = masks.reshape(-1)
    pixlinks = torch.nonzero(flat)[:, 0]
    pointlinks = torch.where(flat, torch.cumsum(flat.long(), 0) - 1, torch.tensor(-1))
    n_points = int(flat.sum())
    cloud = [ref_utils.rend_util.depth_to_world(uv, K[i], pose[i], depth[i], masks[i]) for i in range(n_img)]
    cloud = torch.cat(cloud, 0)
    cloud = cloud[:, :3] / cloud[:, 3:]
    np.savez_compressed(os.path.join(HERE, "g17_bubble_cloud.npz"), H=np.int32(H), W=np.int32(W), depth=depth.numpy(), intrinsics=K.numpy(),
                        pose=pose.numpy(), depth_masks=masks.numpy(), pointlinks=pointlinks.numpy(),
                        pixlinks=pixlinks.numpy(), pointcloud=cloud.numpy())
    print(f"g17_bubble_cloud: {n_points} points of {n_img * total} pixels")


if __name__ == "__main__":
    main()
