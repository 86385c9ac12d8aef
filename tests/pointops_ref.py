"""Numpy restatement of the library's point-set operations (csrc/pointops.hip, i2sdf_amd.mesh.voxel_down_sample /
nearest_neighbors / evaluate): open3d's voxel down-sampling rule with the library's pinned arithmetic, a chunked fp64 brute-force
nearest neighbour with the smallest index on ties, and the five metrics of utils/mesh_util.py:evaluate.  Shared by the CPU and
GPU tests and by scripts/mesh_eval_timing.py."""
import numpy as np

VOXEL_BITS = 21
SEQ_LIMIT = 64          # runs up to this length are summed by a vectorised loop over the rank inside the run


def voxel_indices(points, voxel_size):
    """(N, 3) int64 voxel indices: floor((p - lo) / voxel_size) in fp64, lo = min(points) - voxel_size / 2 per axis."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    v = float(voxel_size)
    if not v > 0.0 or not np.isfinite(v):
        raise ValueError("voxel_size must be positive and finite")
    if not np.isfinite(p).all():
        raise ValueError("non-finite coordinate")
    lo = p.min(axis=0) - 0.5 * v
    idx = np.floor((p - lo) / v)
    if (idx >= float(1 << VOXEL_BITS)).any():
        raise ValueError("voxel index does not fit 21 bits")
    return idx.astype(np.int64)


def voxel_down_sample(points, voxel_size):
    """-> (means (M, 3) fp32, counts (M,) int32), voxels in ascending (ix, iy, iz) order.  Every mean is the fp64 sum of the
    voxel's points in original index order (a sequential, left-to-right sum), divided by their number, rounded to fp32."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    if pts.shape[0] == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    idx = voxel_indices(pts, voxel_size)
    keys = (idx[:, 0] << (2 * VOXEL_BITS)) | (idx[:, 1] << VOXEL_BITS) | idx[:, 2]
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    head = np.concatenate([[True], sk[1:] != sk[:-1]])
    start = np.nonzero(head)[0]
    counts = np.diff(np.concatenate([start, [sk.shape[0]]]))
    sp = pts[order].astype(np.float64)
    sums = np.zeros((start.shape[0], 3), np.float64)
    for r in range(int(min(counts.max(), SEQ_LIMIT))):         # the r-th point of every run that has one, runs side by side
        has = counts > r
        sums[has] = sums[has] + sp[start[has] + r]
    for m in np.nonzero(counts > SEQ_LIMIT)[0]:                # long runs one by one (np.cumsum adds left to right)
        sums[m] = np.cumsum(sp[start[m]:start[m] + counts[m]], axis=0)[-1]
    return (sums / counts[:, None].astype(np.float64)).astype(np.float32), counts.astype(np.int32)


def nearest_neighbors(query, ref, chunk=2048):
    """Brute force in fp64 -> (dist (Q,) fp64, index (Q,) int64): the exact nearest reference point of every query, the
    smallest index among equal distances (np.argmin returns the first minimum)."""
    q = np.asarray(query, np.float64).reshape(-1, 3)
    r = np.asarray(ref, np.float64).reshape(-1, 3)
    if r.shape[0] == 0:
        raise ValueError("ref is empty")
    dist = np.zeros(q.shape[0], np.float64)
    index = np.zeros(q.shape[0], np.int64)
    for a in range(0, q.shape[0], chunk):
        d = q[a:a + chunk, None, :] - r[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        j = np.argmin(d2, axis=1)
        index[a:a + chunk] = j
        dist[a:a + chunk] = np.sqrt(d2[np.arange(j.shape[0]), j])
    return dist, index


def metrics(dist1, dist2, threshold):
    """The dict of utils/mesh_util.py:42-51 from dist1 (trgt -> pred) and dist2 (pred -> trgt)."""
    prec = float(np.mean((np.asarray(dist2) < threshold).astype("float")))
    recal = float(np.mean((np.asarray(dist1) < threshold).astype("float")))
    with np.errstate(invalid="ignore", divide="ignore"):
        fscore = float(np.float64(2 * prec * recal) / np.float64(prec + recal))
    return {"Acc": float(np.mean(dist2)), "Comp": float(np.mean(dist1)), "Prec": prec, "Recal": recal, "F-score": fscore}


def evaluate(pred, trgt, threshold=0.05, down_sample=0.02, nn=nearest_neighbors):
    """utils/mesh_util.py:evaluate on two vertex arrays; `nn(query, ref) -> (dist, index)` may be swapped for a k-d tree."""
    p = np.asarray(pred, np.float32).reshape(-1, 3)
    t = np.asarray(trgt, np.float32).reshape(-1, 3)
    if down_sample:
        p, _ = voxel_down_sample(p, down_sample)
        t, _ = voxel_down_sample(t, down_sample)
    if p.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError("an empty point set")
    dist1, _ = nn(t, p)
    dist2, _ = nn(p, t)
    return metrics(dist1, dist2, threshold)
