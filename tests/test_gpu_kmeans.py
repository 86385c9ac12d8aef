"""GPU: the device clustering (csrc/kmeans.hip: i2sdf_kmeans_pp / _fit / _assign, i2sdf_amd/cluster.py) against the numpy restatement of
its two laws (tests/cluster_ref.py, itself checked on the CPU by tests/test_cluster_ref.py), and I2SDFNetwork.init_emission_groups.

Exact comparisons come with a CONDITION asserted on the restatement's side, not with a tolerance: fp32 log1pf / sqrtf and the fp32 distance
may differ from numpy's fp64 in the last bits, so the seeding indices are compared where every round's two smallest keys differ by more
than 1e-4 relative, labels where a point's two nearest squared distances do, and iteration counts where the error is a factor 2 away from
tol.  The seeds below were chosen (on the restatement) to meet the conditions."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_ref as R

pytestmark = pytest.mark.gpu

SEEDS = {"A": (1, 4, 6, 9, 11), "B": (1, 2, 3, 4, 77)}
LLOYD_SEED = {"A": 1, "B": 77}              # (the restatement's iteration count is decided by a factor 2 for these)
ULP = 2.0 ** -23                            # fp32 ulp of a value in [1, 2): ulp(m) <= m 2^-23


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for name, fx in (("A", R.fixture_a), ("B", R.fixture_b)):
        P, k = fx()
        out[name] = (P, k, torch.from_numpy(P).cuda())
    return out


@pytest.fixture(scope="module")
def seeding_ref(fixtures):
    """the restatement's draws, computed once: (fixture, seed) -> (idx, gaps)"""
    return {(name, seed): R.kmeans_pp(fixtures[name][0], fixtures[name][1], seed) for name in SEEDS for seed in SEEDS[name]}


def _centroid_bar(P):
    return 8 * ULP * float(np.abs(P).max())


# ---- seeding ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_seeding_indices_equal_the_restatement(fixtures, seeding_ref, name):
    from i2sdf_amd import kmeans_pp_centroid
    P, k, X = fixtures[name]
    for seed in SEEDS[name]:
        idx_ref, gaps = seeding_ref[(name, seed)]
        assert gaps.min() > 1e-4, (name, seed, gaps)                       # the condition, on the restatement's side
        cent, idx = kmeans_pp_centroid(X, k, seed=seed, return_index=True)
        assert idx.dtype == torch.int64 and idx.tolist() == idx_ref.tolist(), (name, seed, idx.tolist(), idx_ref.tolist(), gaps)
        assert torch.equal(cent, X[idx])
        cent2, idx2 = kmeans_pp_centroid(X, k, seed=seed, return_index=True)
        assert torch.equal(idx, idx2) and torch.equal(cent, cent2)         # one seed, one draw
    assert kmeans_pp_centroid(X, k, seed=5).shape == (k, 3)


def test_seeding_edges():
    from i2sdf_amd import kmeans_pp_centroid
    same = torch.ones(3, 3, device="cuda")
    for seed in range(6):
        _, idx = kmeans_pp_centroid(same, 2, seed=seed, return_index=True)
        assert idx.tolist() == [R.first_index(3, seed), 0]                # every distance 0: the argmax of an all-false mask
    one = torch.rand(1, 3, device="cuda")
    cent, idx = kmeans_pp_centroid(one, 1, seed=3, return_index=True)
    assert idx.tolist() == [0] and torch.equal(cent, one)
    torch.manual_seed(7)
    a = kmeans_pp_centroid(torch.arange(300, device="cuda", dtype=torch.float32).reshape(100, 3), 4)
    torch.manual_seed(7)
    b = kmeans_pp_centroid(torch.arange(300, device="cuda", dtype=torch.float32).reshape(100, 3), 4)
    assert torch.equal(a, b)                                               # seed=None: torch's CPU generator decides


def test_seeding_law_on_the_device():
    """i2sdf_kmeans_pp itself on n = 8, k = 2 over 4000 seeds: chi^2 of the second picks against d / sum d, conditioned on the first."""
    from i2sdf_amd import lib as L
    h = L.load()
    P = R.law_points()
    X = torch.from_numpy(P).cuda()
    idx = torch.empty(R.LAW_SEEDS, R.LAW_K, dtype=torch.int64, device="cuda")
    cent = torch.empty(R.LAW_K, 3, device="cuda")
    ws = torch.empty(int(h.i2sdf_kmeans_workspace_bytes(R.LAW_N, R.LAW_K)), dtype=torch.uint8, device="cuda")
    for seed in range(R.LAW_SEEDS):
        rc = h.i2sdf_kmeans_pp(L.ptr(X), R.LAW_N, R.LAW_K, seed, L.ptr(ws), C.c_void_p(idx.data_ptr() + 16 * seed), L.ptr(cent), L.stream_ptr())
        assert rc == 0
    pairs = idx.cpu().numpy()
    assert (pairs[:, 0] != pairs[:, 1]).all() and pairs.min() >= 0 and pairs.max() < R.LAW_N
    assert pairs[:, 0].tolist() == [R.first_index(R.LAW_N, s) for s in range(R.LAW_SEEDS)]
    chi, dof = R.chi2_second_pick(P, pairs)
    print(f"device: chi^2 = {chi:.2f} on {dof} degrees of freedom (bar {R.LAW_BAR})")
    assert dof == 7 and chi < R.LAW_BAR


# ---- Lloyd ----------------------------------------------------------------------------------------
def _fit(X, k, seed, **kw):
    from i2sdf_amd import KMeans, kmeans_pp_centroid
    km = KMeans(k, **kw)
    labels = km.fit_predict(X, kmeans_pp_centroid(X, k, seed=seed))
    return km, labels


def test_lloyd_on_fixture_a(fixtures, seeding_ref):
    P, k, X = fixtures["A"]
    seed = LLOYD_SEED["A"]
    ref = R.lloyd(P, P[seeding_ref[("A", seed)][0]])
    assert R.n_iter_is_decided(ref["errors"], 1e-4, 100), ref["errors"]
    km, labels = _fit(X, k, seed)
    assert km.n_iter.dtype == torch.int32 and km.n_iter.is_cuda
    print(f"fixture A: {int(km.n_iter)} iterations (restatement {ref['n_iter']}), errors {ref['errors']}")
    assert int(km.n_iter) == ref["n_iter"]
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), ref["labels"])
    err = float(np.abs(km.centroids.cpu().numpy().astype(np.float64) - ref["means"]).max())
    print(f"fixture A: centroids off the fp64 means by {err:.3e} (bar {_centroid_bar(P):.3e})")
    assert err <= _centroid_bar(P)


@pytest.mark.parametrize("max_iter", [1, 100])
def test_lloyd_on_fixture_b(fixtures, seeding_ref, max_iter):
    P, k, X = fixtures["B"]
    seed = LLOYD_SEED["B"]
    ref = R.lloyd(P, P[seeding_ref[("B", seed)][0]], max_iter=max_iter)
    assert R.n_iter_is_decided(ref["errors"], 1e-4, max_iter), ref["errors"]
    km, labels = _fit(X, k, seed, max_iter=max_iter)
    assert int(km.n_iter) == ref["n_iter"] and (ref["n_iter"] == 1 if max_iter == 1 else ref["n_iter"] > 5)
    got = labels.cpu().numpy()
    close = ref["gap"] < 1e-4
    print(f"fixture B, max_iter {max_iter}: {ref['n_iter']} iterations, {int(close.sum())} points left out, "
          f"{int((got != ref['labels']).sum())} labels differ")
    assert close.mean() <= 0.01
    assert np.array_equal(got[~close], ref["labels"][~close])
    own = R.cluster_means(P, got, k)                                       # the fp64 means of the device's own labels
    err = float(np.abs(km.centroids.cpu().numpy().astype(np.float64) - own).max())
    print(f"fixture B: centroids off the fp64 means of the device's labels by {err:.3e} (bar {_centroid_bar(P):.3e})")
    assert err <= _centroid_bar(P)


def test_rules(fixtures, seeding_ref):
    from i2sdf_amd import KMeans
    P, k, X = fixtures["A"]
    init = X[torch.from_numpy(seeding_ref[("A", 1)][0]).cuda()].clone()
    far = init.clone()
    far[k - 1] = 100.0
    km = KMeans(k, max_iter=1)
    labels = km.fit_predict(X, far)
    assert not bool((labels == k - 1).any()) and km.centroids[k - 1].tolist() == [0.0, 0.0, 0.0]      # an empty cluster ends at the origin
    assert torch.equal(far[k - 1], torch.full((3,), 100.0, device="cuda"))                            # the caller's tensor is not written
    twin = init.clone()
    twin[3] = twin[1]
    labels = KMeans(k, max_iter=1).fit_predict(X, twin)
    assert bool((labels == 1).any()) and not bool((labels == 3).any())                                # ties go to the lower index
    # predict on new points: the fp64 argmin, where the two nearest squared distances are not within 1e-4 of each other
    km = KMeans(k)
    km.fit_predict(X, init)
    new = torch.from_numpy(np.random.default_rng(3).uniform(-1, 2, (1001, 3)).astype(np.float32)).cuda()
    got, d2 = km.predict(new, return_dist2=True)
    want, gap = R.assign(new.cpu().numpy(), km.centroids.cpu().numpy())
    close = gap < 1e-4
    assert close.mean() <= 0.01 and np.array_equal(got.cpu().numpy()[~close], want[~close])
    d2_ref = ((new.double() - km.centroids.double()[got]) ** 2).sum(1)
    assert torch.allclose(d2.double(), d2_ref, rtol=1e-5, atol=0)
    assert torch.equal(km.predict(new), got)
    few = km.predict(new[:2])                                              # fewer points than clusters: i2sdf_kmeans_assign alone takes k > n
    assert torch.equal(few, got[:2]) and km.predict(new[:0]).shape == (0,)
    from i2sdf_amd import lib as L
    lab2 = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert L.load().i2sdf_kmeans_assign(L.ptr(new[:2].contiguous()), 2, L.ptr(km.centroids), k, L.ptr(lab2), None, L.stream_ptr()) == 0
    assert torch.equal(lab2, got[:2])
    # a saved clustering restored through the setter predicts the same
    km2 = KMeans(k)
    km2.centroids = km.centroids
    assert torch.equal(km2.predict(new), got)
    with pytest.raises(ValueError):
        km2.centroids = km.centroids[:2]
    with pytest.raises(ValueError):
        km2.predict(new.double())
    # twice: bit-equal labels and centroids
    a, b = KMeans(k), KMeans(k)
    la, lb = a.fit_predict(X, init), b.fit_predict(X, init)
    assert torch.equal(la, lb) and torch.equal(a.centroids, b.centroids) and torch.equal(a.n_iter, b.n_iter)
    # centroids=None seeds with k-means++ from torch's CPU generator
    torch.manual_seed(3)
    lc = KMeans(k).fit_predict(X)
    torch.manual_seed(3)
    assert torch.equal(lc, KMeans(k).fit_predict(X))


def test_grid_stride_widest_k_and_poisoned_workspace():
    """n = 2^19 + 7 (more points than one sweep of the grid, no multiple of anything), k = 256, one iteration, against torch fp64 on the
    device; and the same call on a workspace full of NaN bytes."""
    from i2sdf_amd import KMeans, kmeans_pp_centroid
    from i2sdf_amd import lib as L
    n, k = (1 << 19) + 7, 256
    g = torch.Generator(device="cuda").manual_seed(4)
    X = torch.rand(n, 3, device="cuda", generator=g) * 2 - 1
    init = X[torch.randperm(n, device="cuda", generator=g)[:k]].clone()
    km = KMeans(k, max_iter=1)
    labels = km.fit_predict(X, init)
    assert int(km.n_iter) == 1
    c64 = init.double()
    want = torch.empty(n, dtype=torch.int64, device="cuda")
    gap = torch.empty(n, dtype=torch.float64, device="cuda")
    for lo in range(0, n, 1 << 16):
        d2 = ((X[lo:lo + (1 << 16)].double()[:, None, :] - c64[None, :, :]) ** 2).sum(-1)
        two, arg = torch.topk(d2, 2, dim=1, largest=False, sorted=True)
        want[lo:lo + (1 << 16)] = arg[:, 0]                                # (an exact tie has gap 0 and is left out below)
        gap[lo:lo + (1 << 16)] = (two[:, 1] - two[:, 0]) / two[:, 1]
    close = gap < 1e-4
    print(f"n = {n}, k = {k}: {int(close.sum())} points left out, {int((labels != want).sum())} labels differ")
    assert float(close.double().mean()) <= 0.01 and torch.equal(labels[~close], want[~close])
    sums = torch.zeros(k, 3, dtype=torch.float64, device="cuda").index_add_(0, labels, X.double())
    cnt = torch.bincount(labels, minlength=k).double()
    own = torch.where(cnt[:, None] > 0, sums / cnt.clamp_min(1)[:, None], torch.zeros_like(sums))
    err = float((km.centroids.double() - own).abs().max())
    bar = 8 * ULP * float(X.abs().max())
    print(f"centroids off the fp64 means of the device's labels by {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    # the same through the C ABI on a poisoned workspace: nothing is read before the call has written it
    h = L.load()
    ws = torch.full((int(h.i2sdf_kmeans_workspace_bytes(n, k)),), 0xFF, dtype=torch.uint8, device="cuda")
    cent, lab2, it2 = init.clone(), torch.empty_like(labels), torch.full((1,), -5, dtype=torch.int32, device="cuda")
    L.check(h.i2sdf_kmeans_fit(L.ptr(X), n, k, L.ptr(cent), 1, 1e-4, L.ptr(ws), L.ptr(lab2), L.ptr(it2), L.stream_ptr()), "i2sdf_kmeans_fit")
    assert torch.equal(lab2, labels) and torch.equal(cent, km.centroids) and int(it2) == 1
    ws.fill_(0xFF)
    idx, seeds = torch.empty(k, dtype=torch.int64, device="cuda"), torch.empty(k, 3, device="cuda")
    L.check(h.i2sdf_kmeans_pp(L.ptr(X), n, k, 9, L.ptr(ws), L.ptr(idx), L.ptr(seeds), L.stream_ptr()), "i2sdf_kmeans_pp")
    seeds2, idx2 = kmeans_pp_centroid(X, k, seed=9, return_index=True)
    assert torch.equal(idx, idx2) and torch.equal(seeds, seeds2) and idx.unique().numel() == k and int(idx.min()) >= 0 and int(idx.max()) < n


# ---- init_emission_groups -------------------------------------------------------------------------
def _net(seed=0):
    from i2sdf_amd import I2SDFNetwork, plumbing_conf
    conf = plumbing_conf(skip=True)
    conf["use_normal"] = True
    torch.manual_seed(seed)
    return I2SDFNetwork(conf).cuda().train()


def _step(net, inp, gt):
    """one seeded training forward and backward -> (outputs, flat gradient)"""
    from i2sdf_amd import I2SDFLoss
    net.force_iters = 1
    for p in net.parameters():
        p.grad = None
    torch.manual_seed(100)
    out = net(inp)
    loss = I2SDFLoss(eikonal_weight=0.1, depth_weight=0.1, normal_weight=0.05)(out, gt, 0)["loss"]
    loss.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in net._param_list()]).clone()
    keep = {key: v.detach().clone() for key, v in out.items() if isinstance(v, torch.Tensor)}
    return keep, grads, loss.detach().clone()


def test_init_emission_groups(fixtures):
    from helpers import camera_inputs, make_gt
    from i2sdf_amd import FusedAdam, KMeans, kmeans_pp_centroid
    P, k, X = fixtures["A"]
    net = _net()
    inp = {key: v.cuda() for key, v in camera_inputs(48, (0.0, 0.2, -1.8), W=32, H=32, f=30.0, seed=1).items()}
    gt = {key: v.cuda() for key, v in make_gt(48).items()}
    out0, g0, l0 = _step(net, inp, gt)
    n_before = len(list(net.parameters()))

    labels, centroids = net.init_emission_groups(k, X, init_emission=2.5, seed=6)
    km = KMeans(k)
    by_hand = km.fit_predict(X, kmeans_pp_centroid(X, k, seed=6))
    assert torch.equal(labels, by_hand) and torch.equal(centroids, km.centroids)
    assert net.emitter_clusters.centroids is centroids and torch.equal(net.emitter_clusters.predict(X[:64]), km.predict(X[:64]))
    em = net.emissions
    assert isinstance(em, torch.nn.Parameter) and em.is_leaf and em.requires_grad and em.is_cuda and em.device == net._flat.device
    assert em.shape == (k, 3) and em.dtype == torch.float32 and bool((em == 2.5).all())
    assert "emissions" in net.state_dict() and torch.equal(net.state_dict()["emissions"], em.detach())
    assert not any("emitter" in key or "centroid" in key for key in net.state_dict())                  # as in the reference: not saved
    group = list(net.get_param_groups(1e-3)[0]["params"])
    assert len(group) == n_before + 1 and any(p is em for p in group)
    assert not any(p is em for p in net._param_list())                                                 # not part of the flat buffer

    out1, g1, l1 = _step(net, inp, gt)                                     # no render or loss route reads it: bit-equal
    assert out0.keys() == out1.keys() and all(torch.equal(out0[key], out1[key]) for key in out0), [key for key in out0 if not torch.equal(out0[key], out1[key])]
    assert torch.equal(g0, g1) and torch.equal(l0, l1) and em.grad is None

    # one optimizer step with a hand-set gradient: FusedAdam updates the tensor outside the flat run like torch.optim.Adam
    twin = torch.nn.Parameter(em.detach().clone())
    grad = torch.linspace(0.1, 1.0, 3 * k, device="cuda").reshape(k, 3) * torch.tensor([1.0, -1.0, 1.0], device="cuda")
    em.grad, twin.grad = grad.clone(), grad.clone()
    flat_before = net._flat.clone()
    for p in net._param_list():
        p.grad = None
    FusedAdam(net.get_param_groups(1e-2), eps=1e-15).step()
    torch.optim.Adam([twin], lr=1e-2, eps=1e-15).step()
    assert torch.equal(net._flat, flat_before)                             # (no gradient there: untouched)
    assert float((em.detach() - twin.detach()).abs().max()) <= 1e-6 * 2.5 and float((em.detach() - 2.5).abs().min()) > 5e-3

    # a refused call leaves the module as it was: the clustering too
    clusters = net.emitter_clusters
    with pytest.raises(ValueError):
        net.init_emission_groups(k, X.double())
    assert net.emissions is em and net.emitter_clusters is clusters and clusters.centroids is centroids


def test_init_emission_groups_dbscan_wrong_count():
    pytest.importorskip("sklearn")
    g = torch.Generator().manual_seed(0)
    centres = torch.tensor([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]])
    cloud = torch.cat([c + 0.05 * torch.randn(60, 3, generator=g) for c in centres]).cuda()      # three tight blobs: no noise points
    net = _net()
    with pytest.raises(ValueError, match="inconsistent emitter count"):
        net.init_emission_groups(4, cloud, use_dbscan=True)
    assert not hasattr(net, "emissions") and not hasattr(net, "emitter_clusters")
    labels, centroids = net.init_emission_groups(3, cloud, use_dbscan=True)                       # the right count: one group per blob
    assert sorted(torch.cdist(centroids.cpu(), centres).argmin(1).tolist()) == [0, 1, 2] and torch.bincount(labels).tolist() == [60, 60, 60]
    assert net.emissions.shape == (3, 3) and net.emissions.is_cuda
