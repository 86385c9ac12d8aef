"""The density-clustering law of include/i2sdf.h ("Density clustering") in numpy fp64: brute force over all pairs, row-chunked, and the
fixtures that tests/test_dbscan_ref.py (against scikit-learn) and tests/test_gpu_dbscan.py (the device against this file) share.

`dbscan` takes three switches that each break the law in one place; tests/test_dbscan_ref.py shows that scikit-learn tells each of
them from the law."""
import numpy as np

CHUNK = 512


def neighbour_matrix(P, eps, strict=False):
    """(n, n) bool: d2 <= eps*eps with every difference, product and sum rounded on its own in fp64 and added x, y, z; a point with a
    non-finite coordinate is nobody's neighbour (not even its own).  -> (matrix, min |d2 - eps^2| / eps^2 over the finite pairs)"""
    P = np.asarray(P, dtype=np.float32)
    n = P.shape[0]
    X = P.astype(np.float64)
    eps2 = np.float64(eps) * np.float64(eps)
    finite = np.isfinite(X).all(1)
    A = np.zeros((n, n), dtype=bool)
    margin = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, CHUNK):
            a = X[lo:lo + CHUNK]
            dx = a[:, None, 0] - X[None, :, 0]
            dy = a[:, None, 1] - X[None, :, 1]
            dz = a[:, None, 2] - X[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = finite[lo:lo + CHUNK, None] & finite[None, :]
            A[lo:lo + CHUNK] = ((d2 < eps2) if strict else (d2 <= eps2)) & ok
            if ok.any():
                margin = min(margin, float((np.abs(d2[ok] - eps2) / eps2).min()))
    return A, margin


def dbscan(P, eps, min_samples, strict=False, border="min", numbering="core"):
    """-> (labels int64 (n,), core bool (n,), n_clusters).  The law: strict=False, border="min", numbering="core".
    Mutations: strict=True tests d2 < eps^2; border="max" gives a border point the largest neighbouring cluster; numbering="member"
    numbers clusters by their first member (border points included) instead of their first core point."""
    A, _ = neighbour_matrix(P, eps, strict)
    n = A.shape[0]
    core = A.sum(1) >= min_samples
    labels = np.full(n, -1, dtype=np.int64)
    k = 0
    for i in np.flatnonzero(core):                 # ascending: a new cluster starts at its smallest core index
        if labels[i] >= 0:
            continue
        member = np.zeros(n, dtype=bool)
        member[i] = True
        front = member.copy()
        while front.any():
            reach = A[front].any(0) & core & ~member
            member |= reach
            front = reach
        labels[member] = k
        k += 1
    for i in np.flatnonzero(~core):
        near = labels[A[i] & core]
        if near.size:
            labels[i] = near.max() if border == "max" else near.min()
    if numbering == "member" and k:
        first = np.array([np.flatnonzero(labels == c)[0] for c in range(k)])
        new = np.empty(k, dtype=np.int64)
        new[np.argsort(first, kind="stable")] = np.arange(k)
        labels = np.where(labels >= 0, new[np.maximum(labels, 0)], -1)
    return labels, core, k


# ---- fixtures ---------------------------------------------------------------------------------------
# name: (seed, blobs, points per blob, blob sigma, box half-width, noise points, eps, min_samples)
CLOUDS = {
    "blobs_0.5_5": (11, 6, 270, 0.45, 9.0, 300, 0.5, 5),
    "blobs_0.12_5": (12, 6, 180, 0.10, 1.5, 220, 0.12, 5),
    "blobs_0.08_4": (13, 8, 110, 0.08, 1.0, 120, 0.08, 4),
    "blobs_0.2_1": (14, 5, 150, 0.25, 3.0, 150, 0.2, 1),
    "blobs_0.15_12": (15, 5, 300, 0.12, 1.2, 200, 0.15, 12),
}


def cloud(name):
    """blobs plus uniform noise, shuffled -> (points (n, 3) float32, eps, min_samples)"""
    seed, blobs, per, sigma, half, noise, eps, min_samples = CLOUDS[name]
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-half, half, (blobs, 3))
    parts = [c + sigma * rng.standard_normal((per, 3)) for c in centres] + [rng.uniform(-half - 1, half + 1, (noise, 3))]
    P = np.concatenate(parts).astype(np.float32)
    return P[rng.permutation(P.shape[0])], eps, min_samples


def _clump(sign, rng):
    """7 points within 0.03 of (sign 0.58, 0, 0) and one arm point 0.45 from the origin: 8 points, all within 0.2 of one another"""
    body = np.array([sign * 0.58, 0.0, 0.0]) + rng.uniform(-0.03, 0.03, (7, 3))
    return np.concatenate([body, [[sign * 0.45, 0.01, 0.02]]])


def contested(order, exact=False):
    """Two clumps of 8 core points and the origin between them, which is within eps = 0.5 of ONE core point of each clump and has too
    few neighbours (3) to be core itself: a border point contested by two clusters, in three index orders.  exact=False: the origin
    sits 0.58 from each clump's body and 0.45 from its arm point, no pair at exactly eps.  exact=True: every coordinate is a multiple
    of 1/8 and the origin is at EXACTLY eps from one point of each clump.  -> (points, eps, min_samples)"""
    rng = np.random.default_rng(5)
    if exact:
        g = np.array([[x, y, 0.0] for x in (0.0, 0.125) for y in (0.0, 0.125, 0.25, 0.375)])      # 8 points, the nearest (0.125, *, 0)
        a, b = g - [0.625, 0.0, 0.0], g * [-1.0, 1.0, 1.0] + [0.625, 0.0, 0.0]                        # nearest x: -0.5 and +0.5
        mid = np.array([[0.0, 0.0, 0.0]])
        min_samples = 6
    else:
        a, b = _clump(-1.0, rng), _clump(1.0, rng)
        mid = np.array([[0.0, 0.0, 0.0]])
        min_samples = 8
    parts = {"a_b_mid": [a, b, mid], "mid_b_a": [mid, b, a], "b_mid_a": [b[:3], mid, a, b[3:]]}[order]
    return np.concatenate(parts).astype(np.float32), 0.5, min_samples


ORDERS = ("a_b_mid", "mid_b_a", "b_mid_a")


def lattice():
    """9 x 9 x 9 points of pitch 0.25: every coordinate exact, many pairs at exactly eps = 0.25 and at exactly 0.5"""
    g = np.arange(9, dtype=np.float64) * 0.25
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


LATTICES = ((0.25, 7), (0.5, 5))


def dense_blobs(n=20000, seed=21):
    """three dense blobs (sigma 0.3, centres a few eps apart and one far away) and a thin halo: at eps 0.5 a point has thousands of
    neighbours -> float32 (n, 3)"""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 40.0, 5.0]])
    per = (n - 200) // 3
    parts = [c + 0.3 * rng.standard_normal((per, 3)) for c in centres]
    parts.append(rng.uniform(-4, 6, (n - 3 * per, 3)))
    P = np.concatenate(parts).astype(np.float32)
    return P[rng.permutation(n)]
