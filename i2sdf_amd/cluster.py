"""Clustering of the emitter point cloud (the reference's `I2SDFNetwork.init_emission_groups`, model/network/__init__.py:49-75):
`kmeans_pp_centroid` (utils/__init__.py:111-123) and `KMeans` (the part of fast_pytorch_kmeans.KMeans the reference uses) on the device,
and the DBSCAN seeding the reference offers as an alternative: on the host with scikit-learn as there, or on the device (`DBSCAN`,
csrc/dbscan.hip: the library's labels for the whole cloud, no scikit-learn).

The k-means routes are HIP (csrc/kmeans.hip; include/i2sdf.h states the laws): stream-ordered, without a host read, seeded and bitwise
reproducible.  Imitated: the seeding law (probability proportional to the distance to the nearest centroid so far), Lloyd's iteration with
the library's stopping rule, empty-cluster rule and returned labels.  Not imitated: numpy's random stream, minibatch k-means, cosine
mode, dimensions other than 3, and the library's default initialisation (see `KMeans.fit_predict`).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import lib as L_

MAX_K = L_.KMEANS_MAX_K


def _points(t, name, dev=None):
    """(n, 3) float32 on a ROCm device, contiguous and detached; refuses anything else with the reason"""
    ok = isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == 3 and t.dtype == torch.float32
    if ok and t.device.type != "cuda":
        raise L_.I2SDFError(f"{name}: expected a tensor on a ROCm device, got one on {t.device} (there is no CPU path)")
    if not ok or (dev is not None and t.device != dev):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name}: expected (n, 3) float32 on {dev if dev is not None else 'a ROCm device'}, got {got}")
    return t.detach().contiguous()


def _sizes(n, k, what):
    if not (1 <= k <= MAX_K):
        raise ValueError(f"{what}: k = {k} is outside 1 .. {MAX_K} (I2SDF_KMEANS_MAX_K)")
    if k > n or n >= 2 ** 31:
        raise ValueError(f"{what}: needs k <= n < 2^31, got n = {n}, k = {k}")


def _workspace(lib, n, k, dev):
    return torch.empty(int(lib.i2sdf_kmeans_workspace_bytes(n, k)), dtype=torch.uint8, device=dev)


def _new_seed():
    # 62 bits from torch's CPU generator: torch.manual_seed decides the run (as in RenderingLayer)
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def kmeans_pp_centroid(points: torch.Tensor, k: int, seed: Optional[int] = None, return_index: bool = False):
    """utils.kmeans_pp_centroid: k rows of `points` (n, 3), the first uniform, each next one drawn with probability proportional to its
    distance to the nearest row chosen so far.  -> centroids (k, 3), and the indices (k,) int64 with return_index.  k launches on the
    current stream, no host read.  seed: 64 bits; None takes 62 bits from torch's CPU generator.  The stream is Philox, not numpy's."""
    pts = _points(points, "points")
    n, k = int(pts.shape[0]), int(k)
    _sizes(n, k, "kmeans_pp_centroid")
    seed = _new_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    lib, dev = L_.load(), pts.device
    idx = torch.empty(k, dtype=torch.int64, device=dev)
    cent = torch.empty(k, 3, dtype=torch.float32, device=dev)
    ws = _workspace(lib, n, k, dev)
    with torch.cuda.device(dev):
        L_.check(lib.i2sdf_kmeans_pp(L_.ptr(pts), n, k, seed, L_.ptr(ws), L_.ptr(idx), L_.ptr(cent), L_.stream_ptr()), "i2sdf_kmeans_pp")
    return (cent, idx) if return_index else cent


class KMeans:
    """fast_pytorch_kmeans.KMeans(n_clusters, max_iter=100, tol=1e-4) as the reference uses it: euclidean, full batch, 3 dimensions."""

    def __init__(self, n_clusters: int, max_iter: int = 100, tol: float = 1e-4):
        if not (1 <= int(n_clusters) <= MAX_K):
            raise ValueError(f"KMeans: n_clusters = {n_clusters} is outside 1 .. {MAX_K} (I2SDF_KMEANS_MAX_K)")
        if int(max_iter) < 1 or not (float(tol) >= 0):
            raise ValueError(f"KMeans: needs max_iter >= 1 and tol >= 0, got {max_iter}, {tol}")
        self.n_clusters, self.max_iter, self.tol = int(n_clusters), int(max_iter), float(tol)
        self._centroids: Optional[torch.Tensor] = None
        self.n_iter: Optional[torch.Tensor] = None          # device int32 (1,): iterations the last fit_predict ran

    @property
    def centroids(self) -> Optional[torch.Tensor]:
        return self._centroids

    @centroids.setter
    def centroids(self, value):
        """Restore a saved clustering: (n_clusters, 3) float32 on a ROCm device."""
        if value is not None:
            value = _points(value, "centroids").clone()
            if value.shape[0] != self.n_clusters:
                raise ValueError(f"centroids: expected ({self.n_clusters}, 3), got {tuple(value.shape)}")
        self._centroids = value

    def fit_predict(self, X: torch.Tensor, centroids: Optional[torch.Tensor] = None, seed: Optional[int] = None) -> torch.Tensor:
        """Lloyd's iteration from `centroids` (n_clusters, 3) until the centroids move by error <= tol or max_iter iterations ran.
        -> labels (n,) int64 of the last iteration (they belong to the centroids before the final update, as in the library);
        self.centroids, self.n_iter (device) are set.  No host read: 2 max_iter launches are enqueued and those after the stop return at once.

        centroids=None seeds with kmeans_pp_centroid(X, n_clusters, seed).  This DIFFERS from the library, whose default initialisation is
        a random subset of X; the reference always passes centroids."""
        X = _points(X, "X")
        n, k, dev = int(X.shape[0]), self.n_clusters, X.device
        _sizes(n, k, "KMeans.fit_predict")
        if centroids is None:
            cent = kmeans_pp_centroid(X, k, seed)
        else:
            cent = _points(centroids, "centroids", dev).clone()
            if cent.shape[0] != k:
                raise ValueError(f"centroids: expected ({k}, 3), got {tuple(cent.shape)}")
        lib = L_.load()
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        n_iter = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(lib, n, k, dev)
        with torch.cuda.device(dev):
            L_.check(lib.i2sdf_kmeans_fit(L_.ptr(X), n, k, L_.ptr(cent), self.max_iter, self.tol, L_.ptr(ws), L_.ptr(labels), L_.ptr(n_iter),
                                          L_.stream_ptr()), "i2sdf_kmeans_fit")
        self._centroids, self.n_iter = cent, n_iter
        return labels

    def predict(self, X: torch.Tensor, return_dist2: bool = False):
        """labels (n,) int64 of the nearest of self.centroids (lowest index on ties); with return_dist2 also the squared distances."""
        if self._centroids is None:
            raise RuntimeError("KMeans.predict: no centroids yet (call fit_predict or assign .centroids)")
        X = _points(X, "X", self._centroids.device)
        n, dev = int(X.shape[0]), X.device
        if n >= 2 ** 31:
            raise ValueError(f"KMeans.predict: needs n < 2^31, got {n}")
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        d2 = torch.empty(n, dtype=torch.float32, device=dev) if return_dist2 else None
        with torch.cuda.device(dev):
            L_.check(L_.load().i2sdf_kmeans_assign(L_.ptr(X), n, L_.ptr(self._centroids), self.n_clusters, L_.ptr(labels), L_.ptr(d2),
                                                   L_.stream_ptr()), "i2sdf_kmeans_assign")
        return (labels, d2) if return_dist2 else labels


class DBSCAN:
    """sklearn.cluster.DBSCAN(eps=0.5, min_samples=5) on the device for (n, 3) float32 clouds: euclidean, no sample weights.  The law
    is stated in include/i2sdf.h ("Density clustering"): the library's labels and core points, with distances formed in fp64.  The whole
    cloud is clustered in a workspace linear in n (csrc/dbscan.hip); every result is bitwise reproducible."""

    def __init__(self, eps: float = 0.5, min_samples: int = 5):
        eps = float(eps)
        if not (eps > 0 and eps * eps > 0 and eps * eps < float("inf")):
            raise ValueError(f"DBSCAN: needs a finite eps > 0, got {eps}")
        if int(min_samples) != min_samples or not (1 <= int(min_samples) < 2 ** 31):
            raise ValueError(f"DBSCAN: needs an integer min_samples in 1 .. 2^31 - 1, got {min_samples}")
        self.eps, self.min_samples = eps, int(min_samples)
        self.labels_: Optional[torch.Tensor] = None              # device int64 (n,): cluster numbers, -1 = noise
        self.core_sample_mask_: Optional[torch.Tensor] = None    # device bool (n,)
        self.n_clusters_: Optional[torch.Tensor] = None          # device int32 (1,)
        self.status_: Optional[torch.Tensor] = None              # device int32 (1,): bit 0 non-finite points, bit 1 beyond 2^21 cells

    @property
    def core_sample_indices_(self) -> torch.Tensor:
        """indices of the core points, ascending (device int64; sized by the mask, so this waits for the device)"""
        if self.core_sample_mask_ is None:
            raise RuntimeError("DBSCAN.core_sample_indices_: nothing fitted yet (call fit_predict)")
        return torch.nonzero(self.core_sample_mask_).reshape(-1)

    def fit_predict(self, X: torch.Tensor, check: bool = True) -> torch.Tensor:
        """-> labels (n,) int64 on X's device; labels_, core_sample_mask_, n_clusters_, status_ are set.  Two library calls around one
        stable torch.sort of the cell keys, all on the current stream.  check=True reads status_ once and raises ValueError for
        non-finite points or a cloud beyond 2^21 cells of eps / 2 per axis; check=False only enqueues (such points end as -1 and
        status_ says why)."""
        X = _points(X, "X")
        n, dev = int(X.shape[0]), X.device
        if not (1 <= n < 2 ** 31):
            raise ValueError(f"DBSCAN.fit_predict: needs 1 <= n < 2^31, got n = {n}")
        lib = L_.load()
        ws = torch.empty(int(lib.i2sdf_dbscan_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        core = torch.empty(n, dtype=torch.uint8, device=dev)
        n_clusters = torch.zeros(1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            L_.check(lib.i2sdf_dbscan_cell_keys(L_.ptr(X), n, self.eps, L_.ptr(ws), L_.ptr(keys), L_.ptr(status), L_.stream_ptr()),
                     "i2sdf_dbscan_cell_keys")
            skeys, perm = torch.sort(keys, stable=True)
            L_.check(lib.i2sdf_dbscan_label(L_.ptr(X), n, self.eps, self.min_samples, L_.ptr(skeys), L_.ptr(perm), L_.ptr(ws), L_.ptr(labels),
                                            L_.ptr(core), L_.ptr(n_clusters), L_.ptr(status), L_.stream_ptr()), "i2sdf_dbscan_label")
        self.labels_, self.core_sample_mask_, self.n_clusters_, self.status_ = labels, core.bool(), n_clusters, status
        if check:
            _raise_status(int(status), self.eps)
        return labels


def _raise_status(status: int, eps: float):
    if status & L_.DBSCAN_NONFINITE:
        raise ValueError("DBSCAN: the points hold non-finite coordinates (such points are labelled -1)")
    if status & L_.DBSCAN_CELLS:
        raise ValueError(f"DBSCAN: the cloud spans more than 2^21 cells of eps / 2 = {0.5 * eps:g} along an axis (the 2^21-cell limit): "
                         "nothing was clustered")


def _device_seeds(points, n_emitters, n_samples, generator):
    pts = _points(points, "points")
    n, dev = int(pts.shape[0]), pts.device
    if n_samples is None:
        samples = pts                                            # the whole cloud in its own order
    else:
        pick = torch.randperm(n, generator=generator)[:n_samples]      # the host route's draw
        samples = pts[pick.to(dev)]
    db = DBSCAN()
    labels = db.fit_predict(samples, check=False)
    found, noise, status = torch.cat([db.n_clusters_.long(), (labels < 0).sum().reshape(1), db.status_.long()]).tolist()      # the one host read
    _raise_status(status, db.eps)
    if noise:
        raise ValueError(f"DBSCAN marked {noise} of {labels.numel()} sampled points as noise: no seed can be taken per cluster "
                         "(the reference would seed the last cluster with point 0)")
    if found != int(n_emitters):
        raise ValueError(f"inconsistent emitter count: n_emitters = {n_emitters}, DBSCAN found {found} clusters")
    m = labels.numel()
    first = torch.full((found,), m, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, labels, torch.arange(m, dtype=torch.int64, device=dev), "amin")      # first sampled point of every cluster
    return samples[first].contiguous()


def dbscan_seeds(points, n_emitters: int, n_samples: Optional[int] = 10000, generator: Optional[torch.Generator] = None,
                 route: str = "host") -> torch.Tensor:
    """The reference's DBSCAN seeding (model/network/__init__.py:50-65): torch.randperm takes n_samples points, DBSCAN with the library's
    defaults (eps 0.5, min_samples 5) labels them, and each cluster's seed is the first sampled point carrying its label.
    -> (n_emitters, 3) float32.

    route="host": sklearn's DBSCAN on the host whatever device `points` is on; the seeds are on the host; needs scikit-learn.
    route="device": the same pick labelled by `DBSCAN` above on the points' ROCm device; the seeds stay there; no scikit-learn, no
    download of the points.  n_samples=None takes the whole cloud in its own order.  One host read (the cluster count,
    the noise count and the status word together): it is a set-up call.

    Raises ValueError where the reference prints and exits (DBSCAN found another number of clusters than n_emitters), and also when
    DBSCAN reports noise points: the reference counts the noise label as a cluster and then seeds the last cluster with point 0."""
    if route == "device":
        return _device_seeds(points, n_emitters, n_samples, generator)
    if route != "host":
        raise ValueError(f"dbscan_seeds: route is 'host' or 'device', got {route!r}")
    try:
        from sklearn.cluster import DBSCAN
    except ImportError as e:
        raise ImportError("init_emission_groups(use_dbscan=True) needs the package scikit-learn (sklearn.cluster.DBSCAN), which is not "
                          "importable here") from e
    pts = torch.as_tensor(points).detach()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points: expected (n, 3), got {tuple(pts.shape)}")
    pick = torch.randperm(pts.shape[0], generator=generator)[:n_samples]
    samples = pts[pick.to(pts.device)].to("cpu", torch.float32)
    labels = torch.from_numpy(DBSCAN().fit_predict(samples.numpy()))
    noise = int((labels < 0).sum())
    if noise:
        raise ValueError(f"DBSCAN marked {noise} of {labels.numel()} sampled points as noise: no seed can be taken per cluster "
                         "(the reference would seed the last cluster with point 0)")
    found = int(torch.unique(labels).numel())
    if found != int(n_emitters):
        raise ValueError(f"inconsistent emitter count: n_emitters = {n_emitters}, DBSCAN found {found} clusters")
    first = [int(torch.nonzero(labels == c)[0, 0]) for c in range(found)]      # first sampled point of every cluster
    return samples[first].contiguous()
