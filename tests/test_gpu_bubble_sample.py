"""GPU: the device bubble sampler (i2sdf_bubble_sample, csrc/bubble.hip; BubblePDF(sampler="device")): its keys against the numpy
restatement (tests/bubble_ref.py), the selection EXACTLY against a sort of the device's own keys, shortfall, reproducibility, the exact
successive-sampling law (the chi-square pair of tests/test_bubble_ref.py with the same inputs and bars), more than 2^24 eligible entries,
no blocking call, and a training step fed by it."""
import ctypes as C

import numpy as np
import pytest
import torch

import bubble_ref as R

pytestmark = pytest.mark.gpu

NOT_ELIGIBLE = 0x7F800000


def _lib():
    from i2sdf_amd import lib as L
    return L, L.load()


def device_keys(w, n, seed, draw):
    L, h = _lib()
    out = torch.full((n,), -1.0, device="cuda")
    L.check(h.i2sdf_bubble_keys(L.ptr(w), n, seed, draw, L.ptr(out), L.stream_ptr()), "i2sdf_bubble_keys")
    return out


def device_sample(w, n, k, seed, draw, cloud=None, count=None, status=None, idx=None, passes=None):
    """`passes`: a list that gets the number of passes over the weights the call made (read from its workspace)."""
    L, h = _lib()
    ws = torch.empty(int(h.i2sdf_bubble_sample_workspace_bytes(k)), dtype=torch.uint8, device="cuda")
    idx = torch.full((k,), -7, dtype=torch.int64, device="cuda") if idx is None else idx
    pts = None if cloud is None else torch.full((k, 3), -7.0, device="cuda")
    L.check(h.i2sdf_bubble_sample(L.ptr(w), n, L.ptr(cloud), k, seed, draw, L.ptr(ws), L.ptr(idx), L.ptr(pts), L.ptr(count), L.ptr(status),
                                  L.stream_ptr()), "i2sdf_bubble_sample")
    if passes is not None:
        passes.append(int(ws[L.BUBBLE_WS_PASSES_OFFSET:L.BUBBLE_WS_PASSES_OFFSET + 4].view(torch.int32).item()))
    return idx, pts


def first_k_of(keys, k):
    """The first k eligible entries of fp32 device keys in ascending (bits, index) order, by a device sort of the composites."""
    bits = keys.view(torch.int32).to(torch.int64)
    comp = (bits << 32) | torch.arange(keys.numel(), device=keys.device)
    comp = torch.sort(comp[bits < NOT_ELIGIBLE]).values
    return comp[:k] & 0xFFFFFFFF


def _weights(case, n):
    g = torch.Generator().manual_seed(n)
    if case == "sparse":                                   # 30 % eligible, the rest zero with a few NaN / negative / inf entries
        w = torch.rand(n, generator=g) * 0.15 + 0.05
        w[torch.rand(n, generator=g) >= 0.3] = 0.0
        w[5::1001], w[7::1003], w[11::1007] = float("nan"), -0.1, float("inf")
    elif case == "wide":                                   # 1e-30 .. 1e30: every top-digit bin of the select is populated
        w = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 60 - 30)
    elif case == "equal":                                  # equal weights: the keys are E / 0.1, still evenly spread at the small end, so
                                                           # the first digit decides here too (test_selection_when_the_keys_cluster is
                                                           # the one that makes the second and third histogram passes work)
        w = torch.full((n,), 0.1)
    else:
        raise KeyError(case)
    return w.to(torch.float32).cuda()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 200003])
def test_keys_match_the_restatement(n):
    """rtol 1e-6 = 8 ulp: log1pf (<= 2), a correctly rounded divide and the restatement's own rounding; a wrong counter or lane mapping
    is off by O(1)."""
    w = torch.rand(n, generator=torch.Generator().manual_seed(n)) * 0.15 + 0.05
    w[::7] = 0.0
    if n > 5:
        w[1], w[2], w[3], w[9], w[10] = float("nan"), -1.0, float("inf"), 1e-30, 1e30
    seed, draw = (0x1234 << 32) | 77, 3
    got = device_keys(w.cuda(), n, seed, draw).cpu().numpy()
    want = R.bubble_keys(w.numpy(), n, seed, draw)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok]) / want[ok]
    print(f"n = {n}: max relative key error {err.max() if ok.any() else 0:.2e}")
    assert (err <= 1e-6).all()
    uni = device_keys(None, n, seed, draw).cpu().numpy()                # weights == NULL: all ones
    assert np.allclose(uni, R.bubble_keys(None, n, seed, draw), rtol=1e-6, atol=0)


@pytest.mark.parametrize("case,n,k", [("sparse", 200003, 1), ("sparse", 200003, 1600), ("sparse", 200003, 4096), ("sparse", 1027, 1024),
                                      ("wide", 50001, 1600), ("equal", 200003, 1600), ("null", 200003, 1600), ("null", 1027, 1024)])
def test_selection_is_exactly_the_k_smallest_composites(case, n, k):
    w = None if case == "null" else _weights(case, n)
    if case == "sparse" and n == 1027:
        w = torch.where(torch.isfinite(w) & (w > 0), w, torch.full_like(w, 0.07))      # all 1027 eligible, k = 1024
    seed, draw = 99, 12
    cloud = torch.rand(n, 3, device="cuda")
    count = torch.zeros(n, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, pts = device_sample(w, n, k, seed, draw, cloud, count, status)
    want = first_k_of(device_keys(w, n, seed, draw), k)
    assert want.numel() == k
    assert torch.equal(idx, want)
    assert torch.equal(pts, cloud[idx])
    mark = torch.zeros(n, device="cuda")
    mark[idx] = 1.0
    assert torch.equal(count, mark) and float(count.sum()) == k
    assert int(status.item()) == 0
    if w is not None:
        wi = w[idx]
        assert bool(((wi > 0) & torch.isfinite(wi)).all())


@pytest.mark.parametrize("span", ["one top bin", "one middle bin"])
def test_selection_when_the_keys_cluster(span):
    """Keys made to order: with weights = E / c the keys are c up to rounding, so they can be packed into one bin of the first digit
    (the second pass has to decide) or into one bin of the second (the third decides, and many keys are equal: the index breaks ties)."""
    n, k, seed, draw = 200003, 1600, 5, 2
    E = device_keys(None, n, seed, draw).double()                           # all weights 1: the keys are E itself
    u = torch.rand(n, generator=torch.Generator().manual_seed(1), dtype=torch.float64).cuda()
    c = 1.01 + 0.04 * u if span == "one top bin" else 1.03 + 2.0 ** -15 * u     # inside [1, 1.0625) / inside a 2^-14 wide bin of it
    w = (E / c).float()
    keys = device_keys(w, n, seed, draw)
    bits = keys.view(torch.int32)
    assert bits.min() >> 19 == bits.max() >> 19                             # one bin of the 12-bit first digit holds every key
    if span == "one middle bin":
        assert keys.unique().numel() < 600 and (bits.max() - bits.min()) < 1024      # massive ties
    cloud = torch.rand(n, 3, device="cuda")
    count = torch.zeros(n, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    passes = []
    idx, pts = device_sample(w, n, k, seed, draw, cloud, count, status, passes=passes)
    assert torch.equal(idx, first_k_of(keys, k)) and torch.equal(pts, cloud[idx])
    assert float(count.sum()) == k and int(status.item()) == 0
    # every key in one first-digit bin: that bin holds n > 2k entries, so the second histogram pass must run; packed into one
    # second-digit bin as well, the third must too (plus the collect pass)
    assert passes == [3 if span == "one top bin" else 4]


def test_evenly_spread_keys_take_two_passes_and_the_count_is_exported():
    """Weights in [0.05, 0.2] on 30 % of 200 003 entries, k = 1600: a first-digit bin is 1/16 octave wide, so about k (1 + 2^(1/16) - 1)
    entries lie at or below the bin of the k-th key -- far fewer than 2k: one histogram pass and the collect pass.  BubblePDF.last_passes
    reads the same word."""
    n, k = 200003, 1600
    w = _weights("sparse", n)
    passes = []
    device_sample(w, n, k, 99, 12, passes=passes)
    assert passes == [2]
    bp = _pdf(seed=5)
    assert bp.last_passes() == 0
    bp.sample_bubble(64)
    assert bp.last_passes() == 2


@pytest.mark.parametrize("n", [5, 1027, 200003])
def test_weights_that_are_not_16_byte_aligned(n):
    """The C ABI takes any float pointer: a view that starts 4 bytes into an allocation goes through the scalar loads of every quad.  The
    keys must be bit-equal to those of an aligned copy and match the restatement; the selection stays exact."""
    k, seed, draw = min(n, 1024) if n < 2000 else 1600, 99, 12
    base = _weights("sparse", n + 1) if n > 5 else torch.tensor([9.0, 0.1, 0.0, 0.2, 0.05, 0.15]).cuda()
    w = base[1:]
    assert w.data_ptr() % 16 == 4 and w.is_contiguous()
    keys = device_keys(w, n, seed, draw)
    assert torch.equal(keys.view(torch.int32), device_keys(w.clone(), n, seed, draw).view(torch.int32))
    want = R.bubble_keys(w.cpu().numpy(), n, seed, draw)
    got = keys.cpu().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= 1e-6 * want[ok]).all()
    m = int(ok.sum())
    cloud = torch.rand(n, 3, device="cuda")
    count = torch.zeros(n, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, pts = device_sample(w, n, k, seed, draw, cloud, count, status)
    real = min(k, m)
    assert torch.equal(idx[:real], first_k_of(keys, real)) and torch.equal(pts, cloud[idx])
    assert float(count.sum()) == real and int(status.item()) == k - real


def test_an_empty_pdf_is_a_shortfall_of_every_row():
    """n = 0 is inside the limits: no entry is eligible, so every index is -1, every point zero, and the counter grows by k."""
    k = 16
    w = torch.empty(0, device="cuda")
    cloud = torch.rand(1, 3, device="cuda")                                 # (an empty tensor has no pointer: NULL would skip `points`)
    count = torch.zeros(1, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for weights in (w, None):
        idx, pts = device_sample(weights, 0, k, 1, 0, cloud, count, status)
        assert bool((idx == -1).all()) and bool((pts == 0).all()) and float(count.sum()) == 0
    assert int(status.item()) == 2 * k
    assert device_keys(w, 0, 1, 0).numel() == 0


def test_more_equal_keys_than_the_buffer_holds_is_counted_and_stays_in_bounds():
    """Every key overflows and is clamped to FLT_MAX, so all n keys equal the k-th smallest: more than 2k records.  The call returns k
    distinct eligible entries out of those it captured, counts the event and writes nothing out of bounds."""
    n, k = 50001, 64
    w = torch.full((n,), 1e-44).cuda()                                      # (a subnormal weight: E / w overflows for all but tiny E)
    w[::3] = 0.0
    keys = device_keys(w, n, 9, 0)
    assert int((keys == torch.finfo(torch.float32).max).sum()) > 2 * k
    guard = torch.full((k + 16,), -7, dtype=torch.int64, device="cuda")
    count = torch.zeros(n, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, _ = device_sample(w, n, k, 9, 0, None, count, status, idx=guard[:k])
    assert bool((guard[k:] == -7).all())
    assert idx.unique().numel() == k and bool((w[idx] > 0).all()) and int(idx.min()) >= 0 and int(idx.max()) < n
    assert float(count.sum()) == k and int(status.item()) == 1


@pytest.mark.parametrize("m", [5, 0])
def test_shortfall_repeats_the_draw_and_counts_it(m):
    n, k = 1000, 16
    w = torch.zeros(n)
    w[1], w[2] = float("nan"), float("inf")
    where = torch.tensor([3, 250, 251, 640, 999])[:m]
    w[where] = torch.tensor([0.3, 0.1, 0.2, 0.05, 0.4])[:m]
    w = w.cuda()
    cloud = torch.rand(n, 3, device="cuda") + 1.0
    count = torch.zeros(n, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, pts = device_sample(w, n, k, 4, 0, cloud, count, status)
    if m == 0:
        assert bool((idx == -1).all()) and bool((pts == 0).all()) and float(count.sum()) == 0
    else:
        assert sorted(idx[:m].tolist()) == where.tolist()
        assert torch.equal(idx[:m], first_k_of(device_keys(w, n, 4, 0), m))
        assert torch.equal(idx, idx[:m][torch.arange(k, device="cuda") % m])
        assert torch.equal(pts, cloud[idx])
        assert float(count.sum()) == m and bool((count[where.cuda()] == 1).all())      # only the m real draws are counted
    assert int(status.item()) == k - m
    device_sample(w, n, k, 4, 1, cloud, count, status)
    assert int(status.item()) == 2 * (k - m)                                # the counter accumulates


def _pdf(n=5000, **kw):
    from i2sdf_amd import BubblePDF
    g = torch.Generator().manual_seed(8)
    bp = BubblePDF(torch.rand(n, 3, generator=g), torch.zeros(1, dtype=torch.int64), sampler="device", **kw)
    bp.pdf.copy_((torch.rand(n, generator=g) * 0.15 + 0.05) * (torch.rand(n, generator=g) < 0.5))
    return bp


def test_reproducible_by_seed_and_draw_and_state_round_trips():
    a, b = _pdf(seed=31), _pdf(seed=31)
    i0, p0 = a.sample_bubble_device(64)
    j0, q0 = b.sample_bubble_device(64)
    assert torch.equal(i0, j0) and torch.equal(p0, q0)                      # same (seed, draw): bit-identical
    i1, _ = a.sample_bubble_device(64)
    assert not torch.equal(i0, i1) and a.sampler_state() == (31, 2)          # the next draw differs
    state = a.sampler_state()
    i2 = a.sample_bubble(64)
    c = _pdf(seed=1)
    c.load_sampler_state(state)
    assert torch.equal(c.sample_bubble(64), i2) and c.sampler_state() == a.sampler_state() == (31, 3)
    assert not torch.equal(_pdf(seed=32).sample_bubble_device(64)[0], i0)    # another seed (another rank) draws other points
    assert float(a.sample_count.sum()) == 3 * 64 and a.shortfall() == 0
    # uniform_bubble passes no weights: zero-PDF entries are drawn too
    u = _pdf(seed=31, uniform_bubble=True)
    iu, _ = u.sample_bubble_device(512)
    assert iu.unique().numel() == 512 and bool((u.pdf[iu] == 0).any())
    assert torch.equal(iu, first_k_of(device_keys(None, 5000, 31, 0), 512))
    from i2sdf_amd import BubblePDF
    assert BubblePDF(torch.zeros(4, 3), torch.zeros(1, dtype=torch.int64)).sampler == "multinomial"      # the default is unchanged


def _device_rows(w, k, draws, seed):
    n = w.numel()
    rows = torch.empty(draws, k, dtype=torch.int64, device="cuda")
    wd = w.cuda()
    for d in range(draws):
        device_sample(wd, n, k, seed, d, idx=rows[d])
    return rows.cpu().numpy()


def test_first_draw_frequencies_follow_the_weights_on_the_device():
    from scipy.stats import chi2
    w = R.first_draw_weights()
    rows = _device_rows(torch.from_numpy(w), R.FIRST_K, R.FIRST_DRAWS, R.STAT_SEED)
    assert (w[rows] > 0).all() and all(np.unique(r).shape[0] == R.FIRST_K for r in rows)
    stat, dof, on_zero = R.chi2_first_draw(w, rows[:, 0])
    print(f"device first-draw chi^2 {stat:.1f} (dof {dof}, bar {chi2.ppf(0.9999, dof):.1f})")
    assert dof == 50 and on_zero == 0 and stat < chi2.ppf(0.9999, 50)


def test_ordered_pairs_follow_successive_sampling_on_the_device():
    from scipy.stats import chi2
    w = np.array(R.PAIR_W, np.float32)
    pairs = _device_rows(torch.from_numpy(w), R.PAIR_K, R.PAIR_DRAWS, R.STAT_SEED)
    stat, dof, off_law = R.chi2_pairs(w, pairs)
    print(f"device ordered-pairs chi^2 {stat:.1f} (dof {dof}, bar {chi2.ppf(0.9999, dof):.1f})")
    assert dof == 41 and off_law == 0 and stat < chi2.ppf(0.9999, 41)


def test_more_than_2_to_24_eligible_entries():
    """n = 2^24 + 4099, every entry eligible: torch.multinomial's category limit makes the default sampler raise (as the reference exits);
    the device sampler returns the exact selection."""
    from i2sdf_amd import BubblePDF
    n, k = (1 << 24) + 4099, 1600
    cloud = torch.rand(n, 3, device="cuda")
    links = torch.zeros(1, dtype=torch.int64)
    eager = BubblePDF(cloud, links)
    eager.pdf.uniform_(0.05, 0.2)
    with pytest.raises(RuntimeError):
        eager.sample_bubble(k)
    bp = BubblePDF(cloud, links, sampler="device", seed=2024)
    bp.pdf.copy_(eager.pdf)
    del eager
    idx, pts = bp.sample_bubble_device(k)
    want = first_k_of(device_keys(bp.pdf, n, 2024, 0), k)
    assert torch.equal(idx, want) and torch.equal(pts, cloud[idx])
    assert float(bp.sample_count.sum()) == k and bp.shortfall() == 0
    tail = torch.zeros(n, device="cuda")
    tail[-3:] = 1.0                                                         # only the last three entries eligible: index n - 1 > 2^24 is returned
    i2, _ = device_sample(tail, n, 3, 1, 0)
    assert sorted(i2.tolist()) == [n - 3, n - 2, n - 1]


def test_device_route_issues_no_blocking_call():
    bp = _pdf(seed=3)
    bp.sample_bubble(64)                                                    # (first call: allocates the workspace)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.where(bp.pdf > 0)
            enforced = False
        except RuntimeError:
            enforced = True
        if enforced:
            pts = bp.sample_bubble(64)                                      # must not raise
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("this torch build does not enforce set_sync_debug_mode('error') (torch.where did not raise): the no-blocking "
                    "assertion cannot be made")
    assert pts.shape == (64, 3) and bool(torch.isfinite(pts).all())


def test_training_step_with_device_bubble_points():
    from i2sdf_amd import I2SDFLoss
    from helpers import camera_inputs, make_gt
    from test_gpu_edge_cases import _net
    net, _, _ = _net(True)
    B = 33
    inp = {k: v.cuda() for k, v in camera_inputs(B, (0.0, 0.2, -1.8), W=32, H=32, f=30.0, seed=3).items()}
    gt = {k: v.cuda() for k, v in make_gt(B).items()}
    bp = _pdf(seed=6)
    bp.pointcloud.mul_(1.4).sub_(0.7)
    inp["pointcloud"] = bp.sample_bubble(64)
    out = net(inp)
    assert out["surface_sdf"].shape == (64, 1)
    res = I2SDFLoss(eikonal_weight=0.1, depth_weight=0.1, normal_weight=0.05, bubble_weight=0.5, min_bubble_iter=50000,
                    max_bubble_iter=150000, smooth_iter=150000)(out, gt, 60000)
    res["loss"].backward()
    assert torch.isfinite(res["bubble_loss"]) and float(res["bubble_loss"]) > 0 and torch.isfinite(res["loss"])
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
