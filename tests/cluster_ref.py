"""numpy restatement of the device clustering's two laws (include/i2sdf.h, "Emitter clustering"): the k-means++ seeding of
i2sdf_kmeans_pp and the Lloyd iteration of i2sdf_kmeans_fit.  What the GPU tests compare against, itself checked on the CPU by
tests/test_cluster_ref.py.  The Philox and the key's constants are those of tests/bubble_ref.py."""
import numpy as np

from bubble_ref import FLT_MAX, MASK, eligible, philox4x32_10

KMEANS_STREAM = 9
F32 = np.float32


def fixture_a():
    """4099 points (no multiple of 4 or 256): five Gaussian blobs, sigma 0.12, centres about 1.5 apart, shuffled.  k = 5."""
    rng = np.random.default_rng(11)
    centres = np.array([[0, 0, 0], [1.5, 0, 0], [0, 1.5, 0], [0, 0, 1.5], [1.5, 1.5, 0]], dtype=np.float64) - 0.6
    sizes = [820, 820, 820, 820, 819]
    pts = np.concatenate([c + 0.12 * rng.standard_normal((m, 3)) for c, m in zip(centres, sizes)])
    return pts[rng.permutation(pts.shape[0])].astype(F32), 5


def fixture_b():
    """4099 points uniform in [-1, 1]^3.  k = 7."""
    return np.random.default_rng(12).uniform(-1, 1, (4099, 3)).astype(F32), 7


def dist2_f32(P, c):
    """((x - cx)^2 + (y - cy)^2) + (z - cz)^2 with every operation rounded to fp32 (numpy's fp32 arithmetic has no FMA)"""
    P, c = np.asarray(P, dtype=F32), np.asarray(c, dtype=F32)
    dx, dy, dz = P[:, 0] - c[0], P[:, 1] - c[1], P[:, 2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def seeding_words(n, seed, rnd):
    """x_j, j < n: word j & 3 of Philox at counter (lo32(j >> 2), hi32(j >> 2), 9, rnd), key (lo32(seed), hi32(seed))."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(q & MASK, q >> np.uint64(32), KMEANS_STREAM, rnd, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return np.stack(w, 1).reshape(-1)[:n]


def first_index(n, seed):
    x = philox4x32_10(0, 0, KMEANS_STREAM, 0, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)[0]
    return (int(x) * n) >> 32


def kmeans_pp(points, k, seed):
    """-> (idx (k,) int64, gaps (k - 1,)): the seeding draws, and for every round the relative gap between the two smallest keys
    (fp64 keys; +inf with fewer than two eligible points).  d is fp32 as on the device; E and the quotient are fp64, rounded once."""
    P = np.asarray(points, dtype=F32)
    n = P.shape[0]
    idx = [first_index(n, seed)]
    d = np.full(n, np.inf, dtype=F32)
    gaps = []
    for rnd in range(1, k):
        d = np.minimum(d, np.sqrt(dist2_f32(P, P[idx[-1]])))
        ok = eligible(d)
        x = seeding_words(n, seed, rnd)
        v = (x.astype(F32) + F32(0.5)) * F32(2.0 ** -32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            key64 = -np.log1p(-v.astype(np.float64)) / np.where(ok, d, 1).astype(np.float64)
        key = np.minimum(key64.astype(F32), FLT_MAX)
        if not ok.any():
            idx.append(0)                       # the reference's argmax of an all-false mask
            gaps.append(np.inf)
            continue
        comp = (key.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        idx.append(int(comp[ok].min() & MASK))
        two = np.sort(key64[ok])[:2]
        gaps.append(float((two[1] - two[0]) / two[0]) if two.shape[0] == 2 else np.inf)
    return np.asarray(idx, dtype=np.int64), np.asarray(gaps, dtype=np.float64)


def assign(points, centroids):
    """fp64: (labels (n,) int64 -- nearest centroid, lowest index on ties --, relative gap between the two smallest squared distances
    per point (+inf for k = 1))"""
    P, c = np.asarray(points, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    d2 = ((P[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    labels = d2.argmin(1)                       # numpy's argmin returns the first minimum
    if c.shape[0] == 1:
        return labels.astype(np.int64), np.full(P.shape[0], np.inf)
    two = np.partition(d2, 1, axis=1)[:, :2]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    return labels.astype(np.int64), gap


def cluster_means(points, labels, k):
    """fp64 mean of each cluster's points; (0, 0, 0) for an empty cluster"""
    P = np.asarray(points, dtype=np.float64)
    sums = np.zeros((k, 3))
    np.add.at(sums, labels, P)
    cnt = np.bincount(labels, minlength=k).astype(np.float64)
    return np.where(cnt[:, None] > 0, sums / np.maximum(cnt, 1)[:, None], 0.0)


def lloyd(points, centroids, max_iter=100, tol=1e-4, keep_fp32=True):
    """fit_predict's loop -> dict(labels, gap, centroids, means, n_iter, errors).  Arithmetic in fp64; keep_fp32: the centroids are
    rounded to fp32 between iterations, as the device (and the library) keep them.  `means` are the last update's fp64 means before
    that rounding; labels and gap are those of the last iteration run (they belong to the centroids before the final update)."""
    c = np.asarray(centroids, dtype=F32).astype(np.float64)
    k = c.shape[0]
    errors = []
    for _ in range(max_iter):
        labels, gap = assign(points, c)
        means = cluster_means(points, labels, k)
        new = means.astype(F32).astype(np.float64) if keep_fp32 else means
        errors.append(float(((new - c) ** 2).sum()))
        c = new
        if errors[-1] <= tol:
            break
    return dict(labels=labels, gap=gap, centroids=c, means=means, n_iter=len(errors), errors=errors)


def n_iter_is_decided(errors, tol, max_iter):
    """The condition under which fp32 roundings cannot change the iteration count: the error is a factor 2 away from tol at the last two
    iterations (above it at the one before the last, below it at the last -- or the run ended on max_iter, above it)."""
    if len(errors) >= 2 and not errors[-2] >= 2 * tol:
        return False
    return errors[-1] <= tol / 2 or (len(errors) == max_iter and errors[-1] >= 2 * tol)


# ---- the statistical case shared by the CPU test of this restatement and the GPU test of the kernel ------------------------------
LAW_N, LAW_K, LAW_SEEDS, LAW_BAR = 8, 2, 4000, 40.5      # chi2.isf(1e-6, 7) = 40.5


def law_points():
    return np.random.default_rng(5).uniform(-1, 1, (LAW_N, 3)).astype(F32)


def chi2_second_pick(points, pairs):
    """The second picks (pairs (draws, 2)) against utils.kmeans_pp_centroid's law, conditioned on the first: the expected count of point j
    is the sum over the draws of d(first, j) / sum_j d(first, j).  -> (chi^2 over the n cells, degrees of freedom n - 1)."""
    P = np.asarray(points, dtype=np.float64)
    pairs = np.asarray(pairs)
    D = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    prob = D / D.sum(1, keepdims=True)
    expect = prob[pairs[:, 0]].sum(0)
    counts = np.bincount(pairs[:, 1], minlength=P.shape[0])
    return float(((counts - expect) ** 2 / expect).sum()), P.shape[0] - 1
