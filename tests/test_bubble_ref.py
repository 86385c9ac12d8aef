"""CPU: the numpy restatement of the device bubble sampler (tests/bubble_ref.py) against what is known independently of it: Random123's
known answers for Philox4x32-10, the composite tie-break, the exact successive-sampling law (chi-square), and the un-projection against
the reference's own cloud and links (tests/golden/g17_bubble_cloud.npz)."""
import numpy as np
import pytest

import bubble_ref as R


def test_philox_reproduces_random123_known_answers():
    got = [int(x) for x in R.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    got = [int(x) for x in R.philox4x32_10(f, f, f, f, f, f)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # the sampler's counter layout: entries 4q .. 4q+3 are the four words of counter (q, 0, 7, draw)
    x = R.bubble_words(11, seed=(5 << 32) | 9, draw=3)
    want = np.stack(R.philox4x32_10(np.arange(3), 0, 7, 3, 9, 5), 1).reshape(-1)[:11]
    assert np.array_equal(x, want)


def test_composite_tie_break_and_shortfall_fill():
    inf = np.float32(np.inf)
    keys = np.array([0.5, 0.25, inf, 0.25, 0.125, 0.25, inf, 0.5], np.float32)
    idx, m = R.select(keys, 4)
    assert m == 4 and idx.tolist() == [4, 1, 3, 5]                  # equal keys: the lower index first
    idx, m = R.select(keys, 6)
    assert m == 6 and idx.tolist() == [4, 1, 3, 5, 0, 7]
    idx, m = R.select(keys, 8)                                      # six eligible: rows 6, 7 repeat rows 0, 1
    assert m == 6 and idx.tolist() == [4, 1, 3, 5, 0, 7, 4, 1]
    idx, m = R.select(np.full(5, inf, np.float32), 3)
    assert m == 0 and idx.tolist() == [-1, -1, -1]


def test_keys_eligibility_and_precision():
    w = np.array([0.1, 0.0, -1.0, np.nan, np.inf, 1e-30, 1e30, 0.2, 3e-39], np.float32)
    keys = R.bubble_keys(w, w.shape[0], seed=1, draw=0)
    assert np.isinf(keys[1:5]).all() and np.isfinite(keys[[0, 5, 6, 7, 8]]).all() and (keys[[0, 5, 6, 7]] > 0).all()
    assert keys[8] <= R.FLT_MAX                                     # an overflowing quotient stays in front of the not-eligible ones
    # the small end of E keeps the low bits of x: neighbouring small words give different keys
    x = np.arange(1, 200, dtype=np.uint32)
    v = (x.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    assert np.unique(-np.log1p(-v.astype(np.float64))).shape[0] == x.shape[0]
    assert np.array_equal(R.bubble_keys(None, 9, 4, 2), R.bubble_keys(np.ones(9, np.float32), 9, 4, 2))


@pytest.mark.parametrize("seed", [R.STAT_SEED, 7, 99])
def test_first_draw_frequencies_follow_the_weights(seed):
    from scipy.stats import chi2
    w = R.first_draw_weights()
    assert int((w > 0).sum()) == 51
    rows = np.stack([R.sample(w, R.FIRST_N, R.FIRST_K, seed, d)[0] for d in range(R.FIRST_DRAWS)])
    assert (w[rows] > 0).all()                                      # zero-weight entries are never drawn, in any of the k rows
    assert all(np.unique(r).shape[0] == R.FIRST_K for r in rows)    # without replacement
    stat, dof, on_zero = R.chi2_first_draw(w, rows[:, 0])
    print(f"seed {seed}: first-draw chi^2 {stat:.1f} (dof {dof}, bar {chi2.ppf(0.9999, dof):.1f})")
    assert dof == 50 and on_zero == 0 and stat < chi2.ppf(0.9999, 50)


@pytest.mark.parametrize("seed", [R.STAT_SEED, 7, 99])
def test_ordered_pairs_follow_successive_sampling(seed):
    from scipy.stats import chi2
    w = np.array(R.PAIR_W, np.float32)
    pairs = np.stack([R.sample(w, 8, R.PAIR_K, seed, d)[0] for d in range(R.PAIR_DRAWS)])
    stat, dof, off_law = R.chi2_pairs(w, pairs)
    print(f"seed {seed}: ordered-pairs chi^2 {stat:.1f} (dof {dof}, bar {chi2.ppf(0.9999, dof):.1f})")
    assert dof == 41 and off_law == 0 and stat < chi2.ppf(0.9999, 41)


def test_unprojection_matches_the_references_cloud_and_links(golden):
    z = golden("g17_bubble_cloud")
    H, W = int(z["H"]), int(z["W"])
    masks, pointlinks, pixlinks, cloud = R.depth_unproject(z["depth"], z["intrinsics"], z["pose"], H, W)
    assert np.array_equal(masks, z["depth_masks"]) and np.array_equal(pointlinks, z["pointlinks"]) and np.array_equal(pixlinks, z["pixlinks"])
    assert not masks.all() and masks.any()
    assert np.abs(cloud - z["pointcloud"]).max() <= 1e-5 * np.abs(z["pointcloud"]).max()
