"""numpy restatement of the device bubble sampler's law (include/i2sdf.h, i2sdf_bubble_sample) and of the depth un-projection
(i2sdf_depth_unproject_*): what the GPU tests compare against, itself checked on the CPU by tests/test_bubble_ref.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
FLT_MAX = np.float32(3.4028234663852886e38)
BUBBLE_STREAM = 7


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit counter words (any broadcastable shapes); returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def bubble_words(n, seed, draw):
    """x_i, i < n: word i & 3 of Philox at counter (lo32(i >> 2), hi32(i >> 2), 7, draw), key (lo32(seed), hi32(seed))."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(q & MASK, q >> np.uint64(32), BUBBLE_STREAM, int(draw) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return np.stack(w, 1).reshape(-1)[:n]


def eligible(weights):
    w = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (w > 0) & (w < np.inf)


def bubble_keys(weights, n, seed, draw):
    """fp32 keys (+inf where not eligible): v in fp32 as the device forms it, E = -log1p(-v) and the quotient in fp64, rounded once to
    fp32, clamped to FLT_MAX.  weights None: all ones."""
    w = np.ones(n, np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    assert w.shape == (n,)
    x = bubble_words(n, seed, draw)
    v = (x.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    ok = eligible(w)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        key = (-np.log1p(-v.astype(np.float64)) / np.where(ok, w, 1).astype(np.float64)).astype(np.float32)
    key = np.minimum(key, FLT_MAX)
    return np.where(ok, key, np.float32(np.inf)).astype(np.float32)


def select(keys, k):
    """The selection from fp32 keys (+inf = not eligible): (idx (k,) int64, m).  The m = min(k, eligible) entries with the smallest
    composite (bits(key), index) in ascending order; row j >= m repeats row j mod m; m = 0 gives -1."""
    keys = np.asarray(keys, dtype=np.float32)
    bits = keys.view(np.uint32).astype(np.uint64)
    comp = (bits << np.uint64(32)) | np.arange(keys.shape[0], dtype=np.uint64)
    comp = np.sort(comp[bits < np.uint64(0x7F800000)])
    m = int(min(k, comp.shape[0]))
    if m == 0:
        return np.full(k, -1, np.int64), 0
    idx = (comp[:m] & MASK).astype(np.int64)
    return idx[np.arange(k) % m], m


def sample(weights, n, k, seed, draw):
    return select(bubble_keys(weights, n, seed, draw), k)


def depth_unproject(depth, intrinsics, pose, H, W, lo=1e-3, hi=6.0):
    """dataset/train_dataset.py:112-141 with utils/rend_util.py's lift and depth_to_world, fp64 arithmetic on the fp32 inputs:
    (masks (n_img, HW) bool, pointlinks (n_img HW,) int64, pixlinks (n_points,) int64, pointcloud (n_points, 3) fp64)."""
    depth = np.asarray(depth, dtype=np.float32).reshape(-1, H * W)
    n_img = depth.shape[0]
    K = np.asarray(intrinsics, dtype=np.float64).reshape(n_img, 4, 4)
    P = np.asarray(pose, dtype=np.float64).reshape(n_img, 4, 4)
    with np.errstate(invalid="ignore"):
        masks = (depth > np.float32(lo)) & (depth < np.float32(hi))
    flat = masks.reshape(-1)
    pixlinks = np.nonzero(flat)[0].astype(np.int64)
    pointlinks = np.full(flat.shape[0], -1, np.int64)
    pointlinks[pixlinks] = np.arange(pixlinks.shape[0])
    img, p = pixlinks // (H * W), pixlinks % (H * W)
    u, v, d = (p % W).astype(np.float64), (p // W).astype(np.float64), depth.reshape(-1)[pixlinks].astype(np.float64)
    fx, fy, cx, cy, sk = K[img, 0, 0], K[img, 1, 1], K[img, 0, 2], K[img, 1, 2], K[img, 0, 1]
    xl = (u - cx + cy * sk / fy - sk * v / fy) / fx * d
    yl = (v - cy) / fy * d
    cam = np.stack([xl, yl, d, np.ones_like(d)], 1)
    world = np.einsum("nij,nj->ni", P[img], cam)
    return masks, pointlinks, pixlinks, world[:, :3] / world[:, 3:]


# ---- the statistical cases shared by the CPU test of this restatement and the GPU test of the kernel ----------------------------
STAT_SEED = 2024
FIRST_N, FIRST_K, FIRST_DRAWS = 64, 8, 4000
PAIR_W = [0.05, 0.2, 0.1, 0, 0.15, 0.07, 0.2, 0.12]
PAIR_K, PAIR_DRAWS = 2, 6000


def first_draw_weights():
    w = np.random.default_rng(1).uniform(0.05, 0.2, FIRST_N).astype(np.float32)
    w[::5] = 0
    return w


def chi2_first_draw(w, firsts):
    """(chi^2 of the first-draw counts over the positive entries against w / W, degrees of freedom, draws that hit a zero weight)."""
    w = np.asarray(w, dtype=np.float64)
    firsts = np.asarray(firsts)
    pos = np.nonzero(w > 0)[0]
    counts = np.bincount(firsts, minlength=w.shape[0])
    expect = firsts.shape[0] * w[pos] / w.sum()
    return float(((counts[pos] - expect) ** 2 / expect).sum()), pos.shape[0] - 1, int(counts[w <= 0].sum())


def chi2_pairs(w, pairs):
    """Ordered pairs (draws, 2) against the exact successive-sampling law P(i, j) = w_i / W * w_j / (W - w_i)."""
    w = np.asarray(w, dtype=np.float64)
    pairs = np.asarray(pairs)
    n, W = w.shape[0], w.sum()
    counts = np.zeros((n, n))
    np.add.at(counts, (pairs[:, 0], pairs[:, 1]), 1)
    P = (w[:, None] / W) * (w[None, :] / (W - w[:, None]))
    np.fill_diagonal(P, 0)
    cells = P > 0
    expect = pairs.shape[0] * P[cells]
    return float(((counts[cells] - expect) ** 2 / expect).sum()), int(cells.sum()) - 1, int(counts[~cells].sum())
