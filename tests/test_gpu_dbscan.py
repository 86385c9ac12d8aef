"""GPU: the device density clustering (csrc/dbscan.hip: i2sdf_dbscan_cell_keys / _label, i2sdf_amd.cluster.DBSCAN) against the numpy
restatement of its law (tests/dbscan_ref.py, itself held to scikit-learn on the CPU by tests/test_dbscan_ref.py): labels, core mask and
cluster count EXACTLY -- the law is stated in fp64 on both sides, operation for operation, so there is no tolerance and no condition.
Then the invariants of the law at 20 000 dense points against fp64 torch, canaries around every buffer, reproducibility, and the
routes up to I2SDFNetwork.init_emission_groups(use_dbscan="device")."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbscan_ref as R

pytestmark = pytest.mark.gpu


def _rng_cloud(kind):
    rng = np.random.default_rng(31)
    if kind == "one":
        return np.array([[0.25, -1.0, 3.0]], dtype=np.float32)
    if kind == "identical":
        return np.tile(np.array([[0.3, 0.1, -0.7]], dtype=np.float32), (300, 1))
    if kind == "few":
        return rng.uniform(0, 0.2, (7, 3)).astype(np.float32)
    if kind == "ball":                                                     # 5000 points within 1e-3 of a centre: one or two dense cells
        d = rng.standard_normal((5000, 3))
        d *= (1e-3 * rng.uniform(0, 1, (5000, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        return (np.array([0.5, 0.5, 0.5]) + d).astype(np.float32)
    if kind == "far":                                                      # two blobs 10^4 apart at eps = 0.01: 2 000 000 cells along x
        a = 0.01 * rng.standard_normal((400, 3))
        b = np.array([1e4, 0.0, 0.0]) + 0.01 * rng.standard_normal((400, 3))
        return np.concatenate([a, b]).astype(np.float32)[rng.permutation(800)]
    raise KeyError(kind)


def _cases():
    """name -> (points, eps, min_samples)"""
    out = {name: R.cloud(name) for name in R.CLOUDS}
    for order in R.ORDERS:
        out[f"contested_{order}"] = R.contested(order)
    out["contested_exact_b_mid_a"] = R.contested("b_mid_a", exact=True)
    for eps, ms in R.LATTICES:
        out[f"lattice_{eps}_{ms}"] = (R.lattice(), eps, ms)
    P, eps, ms = R.cloud("blobs_0.12_5")
    out["permuted_blobs_0.12_5"] = (P[np.random.default_rng(8).permutation(P.shape[0])], eps, ms)
    out["one_point_1"] = (_rng_cloud("one"), 0.5, 1)
    out["one_point_2"] = (_rng_cloud("one"), 0.5, 2)
    out["identical_300"] = (_rng_cloud("identical"), 0.5, 5)
    out["min_samples_above_n"] = (_rng_cloud("few"), 0.5, 8)
    out["dense_ball_5000"] = (_rng_cloud("ball"), 0.5, 5)
    out["far_blobs"] = (_rng_cloud("far"), 0.01, 5)
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def reference():
    """the restatement's answers, computed once and left unchanged"""
    out = {}
    for name, (P, eps, ms) in CASES.items():
        labels, core, k = R.dbscan(P, eps, ms)
        labels.setflags(write=False); core.setflags(write=False)
        out[name] = (labels, core, k)
    return out


def _fit(P, eps, ms, check=True):
    from i2sdf_amd import DBSCAN
    db = DBSCAN(eps, ms)
    labels = db.fit_predict(torch.from_numpy(np.ascontiguousarray(P)).cuda(), check=check)
    assert labels is db.labels_ and labels.dtype == torch.int64 and labels.is_cuda
    assert db.core_sample_mask_.dtype == torch.bool and db.n_clusters_.dtype == torch.int32 and db.n_clusters_.is_cuda and db.status_.is_cuda
    assert torch.equal(db.core_sample_indices_, torch.nonzero(db.core_sample_mask_).reshape(-1))
    return db


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_equal_the_restatement(reference, name):
    P, eps, ms = CASES[name]
    want_labels, want_core, want_k = reference[name]
    db = _fit(P, eps, ms)
    got, core, k = db.labels_.cpu().numpy(), db.core_sample_mask_.cpu().numpy(), int(db.n_clusters_)
    print(f"{name}: n = {P.shape[0]}, {k} clusters (restatement {want_k}), {int(core.sum())} core, {int(((got >= 0) & ~core).sum())} border, "
          f"{int((got != want_labels).sum())} labels and {int((core != want_core).sum())} core flags differ")
    assert int(db.status_) == 0
    assert k == want_k
    assert np.array_equal(core, want_core)
    assert np.array_equal(got, want_labels)


def test_the_cases_take_the_paths_they_are_for(reference):
    assert reference["one_point_1"][2] == 1 and reference["one_point_2"][2] == 0
    assert reference["identical_300"][1].all() and reference["identical_300"][2] == 1
    assert not reference["min_samples_above_n"][1].any() and (reference["min_samples_above_n"][0] == -1).all()
    assert reference["dense_ball_5000"][1].all() and reference["dense_ball_5000"][2] == 1
    assert reference["far_blobs"][2] >= 2 and 2 <= np.unique(reference["far_blobs"][0][reference["far_blobs"][1]]).size
    P = CASES["far_blobs"][0]
    assert (P[:, 0].max() - P[:, 0].min()) / 0.005 > 1.9e6                  # nearly all of the 2^21 cells along x, 800 of them occupied
    assert reference["contested_exact_b_mid_a"][2] == 2 and (~reference["contested_exact_b_mid_a"][1]).sum() == 1
    assert reference["blobs_0.2_1"][2] > 100


def test_non_finite_points():
    from i2sdf_amd import DBSCAN
    P, eps, ms = R.cloud("blobs_0.15_12")
    P = P.copy()
    bad = [17, 903]
    P[bad[0]] = [np.nan, 0.0, 0.0]
    P[bad[1], 2] = np.inf
    keep = np.setdiff1d(np.arange(P.shape[0]), bad)
    want_labels, want_core, want_k = R.dbscan(P[keep], eps, ms)             # the restatement without those rows
    db = _fit(P, eps, ms, check=False)
    got, core = db.labels_.cpu().numpy(), db.core_sample_mask_.cpu().numpy()
    assert int(db.status_) == 1                                            # bit 0
    assert (got[bad] == -1).all() and not core[bad].any()
    assert np.array_equal(got[keep], want_labels) and np.array_equal(core[keep], want_core) and int(db.n_clusters_) == want_k
    full_labels, full_core, _ = R.dbscan(P, eps, ms)                       # and with them: nobody's neighbours
    assert np.array_equal(got, full_labels) and np.array_equal(core, full_core)
    with pytest.raises(ValueError, match="non-finite"):
        DBSCAN(eps, ms).fit_predict(torch.from_numpy(P).cuda())
    only = _fit(np.full((5, 3), np.nan, dtype=np.float32), 0.5, 1, check=False)      # no finite point at all
    assert int(only.status_) == 1 and int(only.n_clusters_) == 0 and (only.labels_ == -1).all() and not only.core_sample_mask_.any()


def test_more_than_2_21_cells():
    from i2sdf_amd import DBSCAN
    rng = np.random.default_rng(2)
    P = rng.uniform(0, 1, (200, 3)).astype(np.float32)
    P[150, 0] = 6.0e5                                                      # 2.4e6 cells of 0.25 away
    db = _fit(P, 0.5, 5, check=False)
    assert int(db.status_) == 2                                            # bit 1
    assert int(db.n_clusters_) == 0 and (db.labels_ == -1).all() and not db.core_sample_mask_.any()
    with pytest.raises(ValueError, match=r"2\^21"):
        DBSCAN(0.5, 5).fit_predict(torch.from_numpy(P).cuda())
    P[150, 0] = 5.0e5                                                      # 2.0e6 cells: inside the limit
    db = _fit(P, 0.5, 5)
    want_labels, want_core, want_k = R.dbscan(P, 0.5, 5)
    assert int(db.status_) == 0 and int(db.n_clusters_) == want_k and np.array_equal(db.labels_.cpu().numpy(), want_labels)
    assert np.array_equal(db.core_sample_mask_.cpu().numpy(), want_core)


def test_invariants_at_20000_dense_points():
    """three dense blobs, eps 0.5: a point has thousands of neighbours.  The arbiter is fp64 torch on the device over all 4e8 pairs."""
    P = R.dense_blobs()
    n, eps, ms = P.shape[0], 0.5, 5
    db = _fit(P, eps, ms)
    labels, core, k = db.labels_, db.core_sample_mask_, int(db.n_clusters_)
    X = torch.from_numpy(P).cuda().double()
    eps2 = torch.tensor(eps, dtype=torch.float64, device="cuda") ** 2
    rows = 2000
    count = torch.empty(n, dtype=torch.int64, device="cuda")
    big = torch.iinfo(torch.int64).max
    near_min = torch.empty(n, dtype=torch.int64, device="cuda")            # smallest label among a point's core neighbours
    split = 0                                                              # core pairs within eps that do not share a label
    for lo in range(0, n, rows):
        a = X[lo:lo + rows]
        dx, dy, dz = (a[:, None, c] - X[None, :, c] for c in range(3))
        A = ((dx * dx + dy * dy) + dz * dz) <= eps2
        count[lo:lo + rows] = A.sum(1)
        Ac = A & core[None, :]
        near_min[lo:lo + rows] = torch.where(Ac, labels[None, :], big).amin(1)
        split += int((Ac & core[lo:lo + rows, None] & (labels[lo:lo + rows, None] != labels[None, :])).sum())
    print(f"n = {n}: {k} clusters, {int(core.sum())} core, {int(((labels >= 0) & ~core).sum())} border, {int((labels < 0).sum())} noise, "
          f"neighbours per point: median {int(count.median())}, max {int(count.max())}")
    assert int(count.median()) > 1000
    assert torch.equal(core, count >= ms)                                  # the core mask is the brute-force count
    assert split == 0                                                      # every core pair within eps shares a label
    assert bool((labels[core] >= 0).all())
    border = ~core & (near_min != big)
    assert torch.equal(labels[border], near_min[border])                   # a border label is the minimum over its core neighbours
    assert bool((labels[~core & (near_min == big)] == -1).all())           # a noise point has no core neighbour
    assert k == int(labels.max()) + 1 and k >= 3
    first = torch.full((k,), n, dtype=torch.int64, device="cuda")
    first.scatter_reduce_(0, labels[core], torch.nonzero(core).reshape(-1), "amin")
    assert bool((first < n).all()) and bool((first[1:] > first[:-1]).all())      # cluster numbers ascend with their first core index
    try:
        from sklearn.cluster import DBSCAN as Library
    except ImportError:
        return
    fit = Library(eps=eps, min_samples=ms).fit(P)
    assert np.array_equal(labels.cpu().numpy(), fit.labels_.astype(np.int64))
    assert np.array_equal(torch.nonzero(core).reshape(-1).cpu().numpy(), fit.core_sample_indices_)


def test_nothing_is_written_outside_the_buffers():
    from i2sdf_amd import lib as L
    h = L.load()
    P, eps, ms = R.cloud("blobs_0.08_4")
    n = P.shape[0]
    X = torch.from_numpy(P).cuda()
    nbytes = int(h.i2sdf_dbscan_workspace_bytes(n))
    PAT = 0xA5

    def guarded(payload_bytes):
        buf = torch.full((64 + payload_bytes + 64,), PAT, dtype=torch.uint8, device="cuda")
        return buf, buf.data_ptr() + 64

    ws, ws_p = guarded(nbytes)
    keys, keys_p = guarded(8 * n)
    labels, labels_p = guarded(8 * n)
    core, core_p = guarded(n)
    nclu, nclu_p = guarded(4)
    status, status_p = guarded(4)
    assert ws_p % 16 == 0 and keys_p % 8 == 0
    rc = h.i2sdf_dbscan_cell_keys(L.ptr(X), n, eps, C.c_void_p(ws_p), C.c_void_p(keys_p), C.c_void_p(status_p), L.stream_ptr())
    assert rc == 0
    skeys, perm = torch.sort(keys[64:64 + 8 * n].view(torch.int64), stable=True)
    rc = h.i2sdf_dbscan_label(L.ptr(X), n, eps, ms, L.ptr(skeys), L.ptr(perm), C.c_void_p(ws_p), C.c_void_p(labels_p), C.c_void_p(core_p),
                              C.c_void_p(nclu_p), C.c_void_p(status_p), L.stream_ptr())
    assert rc == 0
    for name, (buf, size) in dict(workspace=(ws, nbytes), keys=(keys, 8 * n), labels=(labels, 8 * n), core=(core, n), n_clusters=(nclu, 4),
                                  status=(status, 4)).items():
        assert bool((buf[:64] == PAT).all()) and bool((buf[64 + size:] == PAT).all()), f"{name}: bytes outside the buffer were written"
    want_labels, want_core, want_k = R.dbscan(P, eps, ms)
    assert np.array_equal(labels[64:64 + 8 * n].view(torch.int64).cpu().numpy(), want_labels)       # on a workspace full of 0xA5
    assert np.array_equal(core[64:64 + n].cpu().numpy().astype(bool), want_core)
    assert int(nclu[64:68].view(torch.int32)) == want_k and int(status[64:68].view(torch.int32)) == 0
    # a perm that is no permutation is never dereferenced out of range: the call completes and the guards hold
    bad_perm = perm.clone()
    bad_perm[::7] = n + 5
    bad_perm[3::11] = -2
    rc = h.i2sdf_dbscan_label(L.ptr(X), n, eps, ms, L.ptr(skeys), L.ptr(bad_perm), C.c_void_p(ws_p), C.c_void_p(labels_p), C.c_void_p(core_p),
                              C.c_void_p(nclu_p), C.c_void_p(status_p), L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for name, (buf, size) in dict(workspace=(ws, nbytes), labels=(labels, 8 * n), core=(core, n), n_clusters=(nclu, 4)).items():
        assert bool((buf[:64] == PAT).all()) and bool((buf[64 + size:] == PAT).all()), f"{name}: bytes outside the buffer were written"
    lab = labels[64:64 + 8 * n].view(torch.int64)
    assert int(lab.min()) >= -1 and int(lab.max()) < n


def test_two_runs_are_bit_equal():
    P, eps, ms = R.cloud("blobs_0.2_1")
    a, b = _fit(P, eps, ms), _fit(P, eps, ms)
    assert int(a.n_clusters_) > 100
    assert torch.equal(a.labels_, b.labels_) and torch.equal(a.core_sample_mask_, b.core_sample_mask_)
    assert torch.equal(a.n_clusters_, b.n_clusters_) and torch.equal(a.status_, b.status_)
    P, eps, ms = R.cloud("blobs_0.15_12")
    a, b = _fit(P, eps, ms), _fit(P, eps, ms)
    assert torch.equal(a.labels_, b.labels_) and torch.equal(a.core_sample_mask_, b.core_sample_mask_) and torch.equal(a.n_clusters_, b.n_clusters_)


# ---- routes -------------------------------------------------------------------------------------------
CENTRES = torch.tensor([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]])


def _three_blobs():
    """the cloud of tests/test_gpu_kmeans.py::test_init_emission_groups_dbscan_wrong_count: three tight blobs, no noise points"""
    g = torch.Generator().manual_seed(0)
    return torch.cat([c + 0.05 * torch.randn(60, 3, generator=g) for c in CENTRES]).cuda()


def _seeds_from_the_restatement(samples):
    labels, _, k = R.dbscan(samples.cpu().numpy(), 0.5, 5)
    assert (labels >= 0).all()
    return samples[[int(np.flatnonzero(labels == c)[0]) for c in range(k)]]


def test_dbscan_seeds_on_the_device():
    from i2sdf_amd import dbscan_seeds
    cloud = _three_blobs()
    pick = torch.randperm(cloud.shape[0], generator=torch.Generator().manual_seed(3))[:10000]
    want = _seeds_from_the_restatement(cloud[pick.cuda()])
    got = dbscan_seeds(cloud, 3, generator=torch.Generator().manual_seed(3), route="device")
    assert got.is_cuda and got.shape == (3, 3) and got.dtype == torch.float32 and torch.equal(got, want)
    pick = torch.randperm(cloud.shape[0], generator=torch.Generator().manual_seed(4))[:100]
    got = dbscan_seeds(cloud, 3, n_samples=100, generator=torch.Generator().manual_seed(4), route="device")
    assert torch.equal(got, _seeds_from_the_restatement(cloud[pick.cuda()]))
    whole = dbscan_seeds(cloud, 3, n_samples=None, route="device")         # the whole cloud in its own order: the first point of every blob
    assert torch.equal(whole, cloud[[0, 60, 120]])
    try:
        import sklearn.cluster  # noqa: F401
    except ImportError:
        return
    host = dbscan_seeds(cloud, 3, generator=torch.Generator().manual_seed(3))
    assert not host.is_cuda and torch.equal(host, dbscan_seeds(cloud, 3, generator=torch.Generator().manual_seed(3), route="device").cpu())


def test_init_emission_groups_on_the_device_route():
    from helpers import camera_inputs, make_gt
    from test_gpu_kmeans import _net, _step
    cloud = _three_blobs()
    net = _net()
    inp = {key: v.cuda() for key, v in camera_inputs(48, (0.0, 0.2, -1.8), W=32, H=32, f=30.0, seed=1).items()}
    gt = {key: v.cuda() for key, v in make_gt(48).items()}
    out0, g0, l0 = _step(net, inp, gt)
    with pytest.raises(ValueError, match="inconsistent emitter count: n_emitters = 4, DBSCAN found 3 clusters"):
        net.init_emission_groups(4, cloud, use_dbscan="device")
    lonely = torch.cat([cloud, torch.tensor([[50.0, 50.0, 50.0]], device="cuda")])
    with pytest.raises(ValueError, match="DBSCAN marked 1 of 181 sampled points as noise"):
        net.init_emission_groups(3, lonely, use_dbscan="device")
    with pytest.raises(ValueError, match="use_dbscan"):
        net.init_emission_groups(3, cloud, use_dbscan="nonsense")
    assert not hasattr(net, "emissions") and not hasattr(net, "emitter_clusters")       # a refused call leaves the module as it was
    labels, centroids = net.init_emission_groups(3, cloud, use_dbscan="device")         # the right count: one group per blob
    assert sorted(torch.cdist(centroids.cpu(), CENTRES).argmin(1).tolist()) == [0, 1, 2] and torch.bincount(labels).tolist() == [60, 60, 60]
    assert net.emissions.shape == (3, 3) and net.emissions.is_cuda and centroids.is_cuda
    out1, g1, l1 = _step(net, inp, gt)                                     # no render or loss route reads it: bit-equal
    assert out0.keys() == out1.keys() and all(torch.equal(out0[key], out1[key]) for key in out0)
    assert torch.equal(g0, g1) and torch.equal(l0, l1)
