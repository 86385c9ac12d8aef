"""CPU: the numpy restatement the GPU tests of the clustering compare against (tests/cluster_ref.py) is itself right: its seeding law is
utils.kmeans_pp_centroid's, its Lloyd iteration is the library's loop, it follows the empty-cluster and tie rules -- and the host-side
DBSCAN seeding of init_emission_groups (i2sdf_amd.cluster.dbscan_seeds) picks, and refuses, what the reference's does."""
import numpy as np
import pytest
import torch

import cluster_ref as R


def test_seeding_law_is_the_references():
    """utils.kmeans_pp_centroid draws point j with probability d_j / sum d.  n = 8, k = 2, 4000 seeds: chi^2 of the second picks,
    conditioned on the first, over 8 cells (the chosen point itself has probability 0 and must never come back)."""
    P = R.law_points()
    pairs = np.array([R.kmeans_pp(P, R.LAW_K, seed)[0] for seed in range(R.LAW_SEEDS)])
    assert (pairs[:, 0] != pairs[:, 1]).all()
    firsts = np.bincount(pairs[:, 0], minlength=R.LAW_N)
    assert firsts.min() > 0.7 * R.LAW_SEEDS / R.LAW_N, firsts          # the first pick is uniform: 500 each, sigma 21
    chi, dof = R.chi2_second_pick(P, pairs)
    print(f"restatement: chi^2 = {chi:.2f} on {dof} degrees of freedom (bar {R.LAW_BAR})")
    assert dof == 7 and chi < R.LAW_BAR


def _library_loop(X, centroids, max_iter=100, tol=1e-4):
    """fast_pytorch_kmeans.KMeans.fit_predict (0.1.9, euclidean, no minibatch) transcribed to plain torch fp64: the similarity
    2ab - a^2 - b^2 and its argmax, the dense (k, n) mask, nan_to_num for empty clusters, error <= tol."""
    X, c = X.double(), centroids.double().clone()
    k = c.shape[0]
    errors = []
    for _ in range(max_iter):
        sim = 2 * X @ c.T - (X ** 2).sum(1)[:, None] - (c ** 2).sum(1)[None, :]
        closest = sim.argmax(1)
        mask = (closest[None, :] == torch.arange(k)[:, None]).double()
        c_grad = torch.nan_to_num(mask @ X / mask.sum(1)[:, None])
        errors.append(float((c_grad - c).pow(2).sum()))
        c = c_grad
        if errors[-1] <= tol:
            break
    return closest, c, errors


@pytest.mark.parametrize("fixture, seed", [(R.fixture_a, 1), (R.fixture_b, 77)])
def test_lloyd_is_the_librarys_loop(fixture, seed):
    P, k = fixture()
    idx, _ = R.kmeans_pp(P, k, seed)
    got = R.lloyd(P, P[idx], keep_fp32=False)
    labels, c, errors = _library_loop(torch.from_numpy(P), torch.from_numpy(P[idx]))
    assert got["n_iter"] == len(errors) and got["n_iter"] >= 2
    # the two distance forms may order a near tie differently: none of these points is one
    assert float(got["gap"].min()) > 1e-9
    assert np.array_equal(got["labels"], labels.numpy())
    assert np.allclose(got["errors"], errors, rtol=1e-9, atol=1e-18)
    assert np.allclose(got["centroids"], c.numpy(), rtol=0, atol=1e-13)
    # the labels belong to the centroids BEFORE the final update: they are the assignment from the centroids one iteration short
    before = R.lloyd(P, P[idx], max_iter=got["n_iter"] - 1, keep_fp32=False)["centroids"]
    assert np.array_equal(R.assign(P, before)[0], got["labels"])
    if got["errors"][-1] > 0:                              # (the last update moved the centroids: the two are different questions)
        assert not np.array_equal(before, got["centroids"])


def test_empty_cluster_and_tie_rules():
    P, k = R.fixture_a()
    idx, _ = R.kmeans_pp(P, k, 1)
    far = np.concatenate([P[idx[:-1]], [[100.0, 100.0, 100.0]]]).astype(np.float32)
    r = R.lloyd(P, far, max_iter=1)
    assert not (r["labels"] == k - 1).any() and np.array_equal(r["centroids"][k - 1], np.zeros(3))      # the library's nan_to_num
    twin = P[idx].copy()
    twin[3] = twin[1]
    r = R.lloyd(P, twin, max_iter=1)
    assert (r["labels"] == 1).any() and not (r["labels"] == 3).any()                                    # ties go to the lower index
    assert np.array_equal(r["centroids"][3], np.zeros(3))
    # seeding: every distance 0 -> index 0; a single eligible point wins whatever its key
    same = np.ones((3, 3), np.float32)
    for seed in range(8):
        idx, gaps = R.kmeans_pp(same, 2, seed)
        assert idx[1] == 0 and np.isinf(gaps[0])
    two = np.array([[1, 1, 1], [1, 1, 1], [2, 2, 2], [1, 1, 1]], np.float32)
    for seed in range(8):
        idx, _ = R.kmeans_pp(two, 2, seed)
        assert idx[1] == 2 if idx[0] != 2 else idx[1] in (0, 1, 3)


def test_n_iter_condition():
    assert R.n_iter_is_decided([1.0, 3e-4, 4e-5], 1e-4, 100)
    assert not R.n_iter_is_decided([1.0, 1.5e-4, 4e-5], 1e-4, 100)          # an fp32 rounding could have stopped one iteration earlier
    assert not R.n_iter_is_decided([1.0, 3e-4, 8e-5], 1e-4, 100)
    assert R.n_iter_is_decided([1.0], 1e-4, 1) and not R.n_iter_is_decided([1.5e-4], 1e-4, 1)


def _blobs(n_each=60, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.tensor([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]])
    pts = torch.cat([c + 0.05 * torch.randn(n_each, 3, generator=g) for c in centres])
    return pts[torch.randperm(pts.shape[0], generator=g)], centres


def test_dbscan_seeds_one_per_blob_and_refusals():
    pytest.importorskip("sklearn")
    from i2sdf_amd.cluster import dbscan_seeds
    pts, centres = _blobs()
    seeds = dbscan_seeds(pts, 3, generator=torch.Generator().manual_seed(1))
    assert seeds.shape == (3, 3) and seeds.dtype == torch.float32
    nearest = torch.cdist(seeds, centres).argmin(1)
    assert sorted(nearest.tolist()) == [0, 1, 2]                                   # one seed in every blob
    assert all(bool((pts == s).all(1).any()) for s in seeds)                       # ... and each is a point of the cloud
    with pytest.raises(ValueError, match="inconsistent emitter count"):
        dbscan_seeds(pts, 4, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="inconsistent emitter count"):
        dbscan_seeds(pts, 2, generator=torch.Generator().manual_seed(1))
    lonely = torch.cat([pts, torch.tensor([[50.0, 50.0, 50.0]])])                  # no neighbour within eps: DBSCAN calls it noise
    with pytest.raises(ValueError, match="noise"):
        dbscan_seeds(lonely, 3, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="expected"):
        dbscan_seeds(torch.zeros(5, 2), 1)
