"""CPU: the stage checkers of tests/sampler_ref.py on the fp32 oracle's own loop (they must pass, and the printed figures are the
oracle column of the table in tests/test_gpu_sampler_stages.py), their teeth (every mutation of a passing snapshot must fail the
intended checker), and the workspace layout constants against the library."""
import pytest
import torch

import sampler_ref as R
from oracle import i2sdf_oracle as orc

_RUNS = {}


def oracle_case(name, training=False):
    """-> dict(ocfg, sd, snaps {k: Snap}, priors {k: prior beta}, init_beta, draws, u_more, u_final, cam, dirs); computed once."""
    key = (name, training)
    if key in _RUNS:
        return _RUNS[key]
    ocfg, sd = R.case_oracle(name)
    inp = R.case_inputs(name)
    cam, dirs, _ = orc.prepare_rays(inp["uv"], inp["pose"], inp["intrinsics"])
    sc = ocfg.sampler
    dr = R.case_draws(ocfg, R.B_RAYS) if training else None
    forces = R.CASES[name]["force"]
    free = None
    if forces == (0,):
        free, _, _ = R.oracle_snap(sd, ocfg, cam, dirs, training, dr)
        forces = tuple(range(1, free.iters + 1))
    snaps, priors, ib = {}, {}, None
    for k in forces:
        snaps[k], priors[k], ib = R.oracle_snap(sd, ocfg, cam, dirs, training, dr, force=k)
    c = dict(ocfg=ocfg, sd=sd, snaps=snaps, priors=priors, init_beta=ib, draws=dr, free=free, cam=cam, dirs=dirs,
             u_more=torch.linspace(0.0, 1.0, sc.N_samples_eval), u_final=dr.cdf_u if training else torch.linspace(0.0, 1.0, sc.N_samples))
    _RUNS[key] = c
    return c


def run_checks(c, training=False, snaps=None, priors=None, only=None, sdf=True):
    dr = c["draws"]
    return R.check_run(snaps or c["snaps"], priors or c["priors"], c["sd"], c["ocfg"], training, c["u_more"], c["u_final"],
                       extra_idx=dr.extra_idx if dr else None, eik_idx=dr.eik_idx if dr else None, strat_u=dr.strat_u if dr else None,
                       sdf64=R.sdf64_fn(c["sd"], c["ocfg"], c["cam"], c["dirs"]) if sdf else None, init_beta=c["init_beta"], only=only)


@pytest.mark.parametrize("name", list(R.CASES))
def test_checkers_pass_on_the_fp32_oracle(name):
    """Measured (torch 2.x CPU, fp32 oracle vs the fp64 checkers, eval mode, 37 rays), case: largest used fraction of tol more / final,
    beta deviation in bracket widths, flattened share, smallest share of rays with tol < 1e-4 over the stages:
        A  0.094 / 0.044   0.00   2.25 %   0.46        D  0.086 / 0.091   0.00   2.96 %   0.49
        B  0.080 / 0.028   0.00   1.56 %   0.49        E  0.082 / 0.000   0.00   3.67 %   1.00
        C  0.092 / 0.066   0.00   2.56 %   0.38
    row 0 at most 1.05 ulp of far, the Lemma-2 beta 1.7e-7, SDF values 5.3e-7 (max-norm relative).  The final stage is checked after every
    forced count; the largest fractions come from the FIRST row of rays that hit nothing (tol 0.012).  At the loop's natural end
    (D, 5 iterations) the final stage uses 0.023."""
    c = oracle_case(name)
    fig = run_checks(c)
    print(fig.line(f"oracle fp32, case {name}"))
    fig.assert_not_soft(name)
    assert fig.used["more"] <= 0.2 and fig.used["final"] <= 0.2      # torch's own fp32 needs a small part of tol (the device gets all of it)
    assert fig.widths <= 0.5 and fig.exempt == 0
    if name == "D":
        free = c["free"]
        assert free.iters == max(c["snaps"]) and torch.equal(free.row, c["snaps"][free.iters].row) and torch.equal(free.z_out, c["snaps"][free.iters].z_out)


def test_checkers_pass_on_the_fp32_oracle_in_training_mode():
    c = oracle_case("D", training=True)
    fig = run_checks(c, training=True)
    print(fig.line("oracle fp32, case D (training draws)"))
    fig.assert_not_soft("D/train")


# ---- teeth -----------------------------------------------------------------------------------------------------------------------
def failing(c, training, snaps, priors=None):
    """The checkers that fail on these snapshots -> {name: message}."""
    out = {}
    for chk in R.CHECKERS:
        try:
            run_checks(c, training, snaps=snaps, priors=priors, only={chk}, sdf=False)
        except AssertionError as e:
            out[chk] = str(e)
    return out


def _recompose(s, c, training):
    dr = c["draws"]
    s.z_out = R.compose_final(s, c["ocfg"], training, dr.extra_idx if dr else None)
    if s.z_eik is not None:
        e = dr.eik_idx.long().reshape(-1, 1) if training else torch.zeros(s.B, 1, dtype=torch.long)
        s.z_eik = torch.gather(s.z_out, 1, e)
    return s


def _with(c, k, s):
    snaps = dict(c["snaps"])
    snaps[k] = s
    return snaps


def test_teeth_sample_in_the_neighbouring_bracket():
    c = oracle_case("E")                                       # every ray hits: all tolerances small
    k = 4
    s = c["snaps"][k].copy()
    N = c["ocfg"].sampler.N_samples
    for r in range(s.B):
        j = int(torch.searchsorted(s.row[r], s.samples[r, N // 2], right=True))       # bracket (j-1, j) -> the middle of (j, j+1)
        j = min(j, s.n - 2)
        s.samples[r, N // 2] = 0.5 * (s.row[r, j] + s.row[r, j + 1])
    s.samples[:, :N] = torch.sort(s.samples[:, :N], -1)[0]
    f = failing(c, False, _with(c, k, _recompose(s, c, False)))
    assert set(f) == {"resample"} and "check_resample/final/cdf" in f["resample"], f


def test_teeth_largest_u_replaced_by_far():
    c = oracle_case("D", training=True)                        # (eval rows end AT far and their largest u is 1: no mutation there)
    k = 3
    s = c["snaps"][k].copy()
    N = c["ocfg"].sampler.N_samples
    s.samples[torch.arange(s.B), c["u_final"].argmax(-1)] = 2.0 * c["ocfg"].scene_bounding_sphere
    assert N == c["u_final"].shape[1]
    f = failing(c, True, _with(c, k, _recompose(s, c, True)))
    assert set(f) == {"resample"} and "check_resample/final" in f["resample"], f


@pytest.mark.parametrize("name,k", [("B", 3), ("A", 1)])
def test_teeth_last_lane_block_shifted_by_one(name, k):
    """Row entries j >= 64 (E - 1) shifted by one position.  In a merged row that is the merge's finding (values no longer where idx says);
    in row 0 it is the initial row's.  The checkers that read the row as their INPUT (beta, resample, final) may notice too; none other may."""
    c = oracle_case(name)
    s = c["snaps"][k].copy()
    E = -(-s.n // 64)
    j0 = 64 * (E - 1)
    s.row[:, j0:s.n - 1] = c["snaps"][k].row[:, j0 + 1:]
    f = failing(c, False, _with(c, k, s))
    want = "merge" if k > 1 else "init"
    assert want in f and set(f) <= {want, "beta", "resample", "final"}, f
    if k > 1:
        assert "check_merge/carry" in f["merge"], f


def test_teeth_two_idx_entries_swapped():
    c = oracle_case("A")
    k = 5
    s = c["snaps"][k].copy()
    n_old = s.n - s.N_eval
    for r in range(s.B):
        j = (s.idx[r] < n_old).nonzero().reshape(-1)
        a, b = int(j[10]), int(j[40])
        s.idx[r, a], s.idx[r, b] = c["snaps"][k].idx[r, b], c["snaps"][k].idx[r, a]
    f = failing(c, False, _with(c, k, s))
    assert set(f) == {"merge"} and "check_merge/carry" in f["merge"], f


def test_teeth_new_sdf_values_rotated():
    c = oracle_case("C")
    for k in (1, 7):
        s = c["snaps"][k].copy()
        s.sdf_new = torch.roll(s.sdf_new, 1, dims=1)
        f = failing(c, False, _with(c, k, s))
        assert set(f) == {"merge"} and "check_merge/sdf" in f["merge"], f


def test_teeth_beta_raised_by_four_bracket_widths():
    """(check_resample reads beta as an input of the final pdf; no other checker may notice)"""
    c = oracle_case("A")
    k = 2
    s = c["snaps"][k].copy()
    w = (c["priors"][k] - R._beta0(c["sd"], c["ocfg"])) / 2.0 ** c["ocfg"].sampler.beta_iters
    s.beta = s.beta + 4.0 * w
    f = failing(c, False, _with(c, k, s))
    assert "beta" in f and set(f) <= {"beta", "resample"} and "check_beta/bar" in f["beta"], f
    s.beta = c["snaps"][k].beta + 1.0 * w                     # one width is inside the bar
    assert "beta" not in failing(c, False, _with(c, k, s))


@pytest.mark.parametrize("training", [False, True])
def test_teeth_extra_slot_replaced_by_its_row_neighbour(training):
    c = oracle_case("D", training)
    k = 2
    s = c["snaps"][k].copy()
    ex = R.extra_index(s, c["ocfg"], training, c["draws"].extra_idx if training else None)
    e = int(ex[3])
    other = s.row[:, e + 1] if e + 1 < s.n else s.row[:, e - 1]
    assert bool((other != s.row[:, e]).any())
    for r in range(s.B):
        slot = int((s.z_out[r] == s.row[r, e]).nonzero()[0])
        s.z_out[r, slot] = other[r]
    s.z_out = torch.sort(s.z_out, -1)[0]
    if s.z_eik is not None:
        eik = c["draws"].eik_idx.long().reshape(-1, 1) if training else torch.zeros(s.B, 1, dtype=torch.long)
        s.z_eik = torch.gather(s.z_out, 1, eik)
    f = failing(c, training, _with(c, k, s))
    assert set(f) == {"final"} and "check_final/z_out" in f["final"], f


def test_teeth_tie_ordered_new_before_old():
    c = oracle_case("A")                                       # eval: u = 0 puts a new sample AT row[0] = near in every merge
    k = 3
    s = c["snaps"][k].copy()
    n_old = s.n - s.N_eval
    done = 0
    for r in range(s.B):
        for j in range(s.n - 1):
            if s.row[r, j] == s.row[r, j + 1] and s.idx[r, j] < n_old <= s.idx[r, j + 1]:
                s.idx[r, j], s.idx[r, j + 1] = c["snaps"][k].idx[r, j + 1], c["snaps"][k].idx[r, j]
                s.sdf_row[r, j], s.sdf_row[r, j + 1] = c["snaps"][k].sdf_row[r, j + 1], c["snaps"][k].sdf_row[r, j]
                done += 1
                break
    assert done >= s.B // 2
    f = failing(c, False, _with(c, k, s))
    assert set(f) == {"merge"} and "check_merge/tie" in f["merge"], f


def test_iteration_count_mismatch_is_caught():
    c = oracle_case("D")
    k = 2
    s = c["snaps"][k].copy()
    s.iters_out = k + 1
    f = failing(c, False, _with(c, k, s))
    assert set(f) == {"final"} and "check_final/iters" in f["final"], f


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def test_layout_constants_match_the_library():
    from i2sdf_amd import lib as L                 # the host library, loaded (and built when missing) as tests/test_cabi.py does
    import os
    import subprocess
    import sys
    if not os.path.exists(L.LIB_PATH):
        subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       check=True)
    h = L.load()
    for B in (1, 4, 37, 1024, 3 * 10 ** 6):
        assert h.i2sdf_sampler_workspace_floats(B) == R.workspace_floats(B)
        lay = R.layout(B)
        off, _, width = lay["state"]
        assert off + width + R.ST_TAIL == R.workspace_floats(B)
        assert lay["samples"][0] == 6 * B * R.NMAX and lay["beta"][0] == lay["samples"][0] + 2 * B * R.NNEW
    assert R.ST_CNT0 + 12 <= R.ST_WORDS and R.ST_FLAG0 + 12 <= R.ST_CNT0       # one flag and one counter per possible iteration


def test_snapshot_slices_by_parity():
    B, N = 3, 36
    ws = torch.arange(R.workspace_floats(B), dtype=torch.float32)
    lay = R.layout(B)
    for iters in (1, 2, 5):
        s = R.snapshot(ws, B, N, iters)
        cur, prev = ("zA", "zB") if iters % 2 else ("zB", "zA")
        assert s.row.shape == (B, N * iters) and float(s.row[1, 2]) == lay[cur][0] + R.NMAX + 2
        assert float(s.sdf_row[2, 0]) == lay["sA" if iters % 2 else "sB"][0] + 2 * R.NMAX
        if iters > 1:
            assert s.prev_row.shape == (B, N * (iters - 1)) and float(s.prev_row[0, 1]) == lay[prev][0] + 1
            assert s.idx.shape == (B, N * iters)
        assert float(s.samples[1, 0]) == lay["samples"][0] + R.NNEW and float(s.beta[2]) == lay["beta"][0] + 2
        assert s.state.numel() == R.ST_WORDS
