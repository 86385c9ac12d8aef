"""GPU: every stage of the error-bounded sampler (csrc/sampler.hip) against fp64, on the device's own inputs to that stage.

tests/test_gpu_sampler.py compares the END of the loop with a criterion that tolerates 2 % of the depths being anywhere; a kernel that
gets one position per row wrong passes it.  Here the loop's workspace is read after every call (tests/sampler_ref.py: snapshot) and each
stage -- initial row and Lemma-2 beta, SDF merge, beta line search, the "more" pdf and the final pdf with their inverse CDFs, the stable
sorted merge with its idx map, the sorting epilogue -- is repeated in fp64 from what the device fed it.  The run with force_iters = k
shows row k, its SDF row, beta_k, the final-pdf samples, the merge k-1 -> k and the "more" samples of iteration k-1; the prior beta of
iteration k is the beta of the run with k-1.  Cases (tests/sampler_ref.py: CASES) reach every row-length instantiation E = 1..10 of the
three iteration kernels, rows that are no multiple of 32 or 64, twelve iterations, the split (data-dependent) and the fused (forced)
kernels, eval and training draws, B = 1, 4 and 37 (one live wave in the last workgroup), the 64-wide and the 256-wide SDF passes with
three and with two planes.  (The two-plane option exists for 256-wide nets only -- i2sdf_plan_set_option refuses it on a 64-wide plan
-- so the two plane counts run on the 256-wide net, with the sampler sizes of cases A and D.)

Measured on an MI355X / by the fp32 oracle on the CPU (tests/test_sampler_ref.py), 37 rays, eval mode:
(device / oracle; "used" = largest used fraction of check_resample's derived tol; beta = largest deviation of the line search in final
bracket widths, rays exempted; flat = share of samples in flattened brackets; small = smallest share, over the stages, of rays with
tol < 1e-4; row 0 in ulp of far; sdf = max-norm relative error of the SDF row (64-wide fp32 pass), bar 2e-5)

    case        used "more"     used final      beta        flat %        small        row 0        sdf
    A           0.114 / 0.094   0.023 / 0.044   0.00, 0     2.25 / 2.25   0.46 / 0.46  1.05 / 1.05  2.1e-7 / 3.6e-7
    B           0.100 / 0.080   0.015 / 0.028   0.00, 0     1.56 / 1.56   0.49 / 0.49  0.85 / 0.85  2.6e-7 / 4.1e-7
    C           0.103 / 0.092   0.066 / 0.066   0.00, 0     2.56 / 2.56   0.38 / 0.38  0.63 / 0.63  2.1e-7 / 3.6e-7
    D eval      0.090 / 0.086   0.077 / 0.091   0.00, 0     3.08 / 2.96   0.49 / 0.49  0.84 / 0.84  2.1e-7 / 3.6e-7
    D training  0.098 / 0.098   0.079 / 0.103   0.00, 0     1.07 / 0.99   0.49 / 0.49  1.49 / 1.49  2.6e-7 / 3.6e-7
    E           0.060 / 0.082   0.000 / 0.000   0.00, 0     3.67 / 3.67   1.00 / 1.00  1.05 / 1.05  3.0e-7 / 5.3e-7

(The final stage is checked after EVERY forced count, not only where the loop would end; its largest fractions come from the first row
of rays that hit nothing, tol = 0.012.  At the loop's natural end the oracle uses 0.023 on D.  The D rows of the device include the
data-dependent snapshot beside the forced ones, hence the slightly different shares.)  Initial beta vs Lemma 2: device 7.2e-8 ... 1.6e-7,
oracle 9.6e-8 ... 2.0e-7 (bar 1e-6).  256-wide net: used 0.094 / 0.031 at most, SDF row 4.8e-7 under three planes, the same figures to
two digits under two planes.  No ray needed the line search's exemption.  The data-dependent snapshot of D (split kernels) was bit-equal
to the forced run of equal count (fused kernel) in every mode and batch size, and so were the 256-wide ones.  No stage check failed: the
DPP scans, the E-blocked row code, the LDS searches and the epilogue are as the reference computes them at every E and in both loops.
"""
import pytest
import torch

import sampler_ref as R
from oracle import i2sdf_oracle as orc
from test_gpu_train_forward import make_engine, TOL

pytestmark = pytest.mark.gpu

assert R.SDF_TOL == TOL          # check_merge holds single SDF values to the project's bar for that kernel

PATTERN = 0x4B4B4B4B          # 13323083.0f: finite, no depth, no sdf value, no index < 640


class Device:
    """One engine on one case's rays; run(force) -> Snap of that call."""

    def __init__(self, conf, ocfg, sd, inp, B, training=False, planes=None):
        self.ocfg, self.sd, self.B, self.training = ocfg, sd, B, training
        self.eng = make_engine(conf, sd)
        if planes is not None:
            self.eng.set_sampler_bf16x2(planes == 2)
        self.flat = self.eng.layout.flat_from_state_dict(sd).cuda()
        self.cam, self.dirs, _ = self.eng.ray_setup(inp["uv"].cuda(), inp["pose"].cuda(), inp["intrinsics"].cuda())
        self.draws = R.case_draws(ocfg, B) if training else None
        sc = ocfg.sampler
        self.u_more = self.eng.u_more.cpu()
        self.u_final = self.draws.cdf_u if training else self.eng.u_final.cpu()
        self.beta0 = R._beta0(sd, ocfg)
        self.grid = (B + 3) // 4
        assert sc.N_samples_eval == self.eng.cfg.sampler.N_samples_eval and sc.max_total_iters == self.eng.cfg.sampler.max_total_iters

    def run(self, force=0, workspace=None):
        kw = {}
        if self.training:
            d = self.draws
            kw = dict(strat_u=d.strat_u.cuda(), cdf_u=d.cdf_u.cuda(), extra_idx=d.extra_idx.cuda(), eik_idx=d.eik_idx.cuda())
        zo, zeik, iters = self.eng.sample_rays(self.flat, self.cam, self.dirs, training=self.training, force_iters=force, workspace=workspace, **kw)
        torch.cuda.synchronize()
        it = int(iters.item())
        assert 1 <= it <= self.ocfg.sampler.max_total_iters
        s = R.snapshot(self.eng._last_sampler_ws, self.B, self.ocfg.sampler.N_samples_eval, it)
        s.z_out, s.z_eik, s.iters_out = zo.cpu(), zeik.cpu(), it
        return s

    def lemma2(self, s1):
        """Prior beta of iteration 1 (overwritten by the line search; test_initial_row_and_beta reads it from a run without a line
        search and holds it to 1e-6 of this formula)."""
        z = s1.row.double()
        return torch.sqrt((1.0 / (4.0 * torch.log(torch.tensor(self.ocfg.sampler.eps + 1.0, dtype=torch.float64)))) * ((z[:, 1:] - z[:, :-1]) ** 2).sum(-1))

    def check(self, snaps, priors, sdf=True, fig=None):
        d = self.draws
        return R.check_run(snaps, priors, self.sd, self.ocfg, self.training, self.u_more, self.u_final,
                           extra_idx=d.extra_idx if d else None, eik_idx=d.eik_idx if d else None, strat_u=d.strat_u if d else None,
                           sdf64=R.sdf64_fn(self.sd, self.ocfg, self.cam, self.dirs) if sdf else None, sdf_last_only=True, fig=fig)

    def forced(self, ks):
        snaps, priors = {}, {}
        for k in ks:
            snaps[k] = self.run(force=k)
            assert snaps[k].iters == k, f"force_iters={k}: the loop reports {snaps[k].iters} iterations"
            priors[k] = snaps[k - 1].beta if k - 1 in snaps else (self.lemma2(snaps[k]) if k == 1 else None)
        return snaps, priors

    def check_state(self, s, free):
        """The state words after a call: done, the count, one workgroup counter per iteration run; data-dependent runs: the batch flag of
        every iteration but the last is up, and the loop ended where no ray's beta was above beta0 (or at max_total_iters)."""
        st, it, mx = s.state, s.iters, self.ocfg.sampler.max_total_iters
        assert int(st[R.ST_DONE]) == 1 and int(st[R.ST_ITERS]) == it
        assert st[R.ST_CNT0:R.ST_CNT0 + it].tolist() == [self.grid] * it and not bool(st[R.ST_CNT0 + it:R.ST_WORDS].any())
        if free:
            assert st[R.ST_FLAG0:R.ST_FLAG0 + it - 1].tolist() == [1] * (it - 1) and not bool(st[R.ST_FLAG0 + it:R.ST_CNT0].any())
            above = bool((s.beta > torch.tensor(self.beta0)).any())
            assert int(st[R.ST_FLAG0 + it - 1]) == int(above) and (not above or it == mx)
        else:
            assert not bool(st[R.ST_FLAG0:R.ST_CNT0].any())


def bit_equal(a, b, N):
    """Two snapshots of the same loop, bit for bit (of `samples` the N columns the last step wrote; the rest of a fresh workspace is not set)."""
    a, b = a.copy(samples=a.samples[:, :N]), b.copy(samples=b.samples[:, :N])
    return all(torch.equal(getattr(a, f).float().view(torch.int32), getattr(b, f).float().view(torch.int32))
               for f in ("row", "sdf_row", "sdf_new", "samples", "beta", "z_out", "z_eik")) and (a.idx is None or torch.equal(a.idx, b.idx))


def plumbing_device(name, B=R.B_RAYS, training=False):
    ocfg, sd = R.case_oracle(name)
    return Device(R.case_conf(name), ocfg, sd, R.case_inputs(name, B), B, training)


def wide_device(N_eval, max_iters, planes, B=R.B_RAYS):
    """The 256-wide net (synthetic_conf) with the sampler sizes given."""
    from i2sdf_amd.config import synthetic_conf
    ocfg = orc.synthetic_cfg()
    ocfg.sampler.N_samples_eval, ocfg.sampler.max_total_iters = N_eval, max_iters
    sd = orc.perturb_params(orc.init_params(ocfg, seed=23), 0.05, seed=24)
    sd["density.beta"] = torch.tensor(0.02)
    conf = synthetic_conf()
    conf["ray_sampler"].update({"N_samples_eval": N_eval, "max_total_iters": max_iters})
    return Device(conf, ocfg, sd, R.case_inputs("A", B), B, planes=planes)


# ---- forced iteration counts: the fused A+B kernel, every E ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_forced_iteration_counts(name):
    dev = plumbing_device(name)
    snaps, priors = dev.forced(R.CASES[name]["force"])
    for s in snaps.values():
        dev.check_state(s, free=False)
    fig = dev.check(snaps, priors)
    print(fig.line(f"device, case {name}"))
    fig.assert_not_soft(name)
    assert fig.exempt == 0


# ---- data-dependent loop: the split beta / resample kernels, ST_DONE ----------------------------------------------------------------
@pytest.mark.parametrize("B", [R.B_RAYS, 1, 4])
@pytest.mark.parametrize("training", [False, True])
def test_data_dependent_loop(training, B):
    dev = plumbing_device("D", B, training)
    free = dev.run(force=0)
    dev.check_state(free, free=True)
    it = free.iters
    snaps, priors = dev.forced(range(1, it + 1))
    for k in range(1, it):                                       # the loop went on exactly while some ray's beta was above beta0
        assert bool((snaps[k].beta > torch.tensor(dev.beta0)).any()), f"the loop ran {it} iterations although every ray had beta0 after {k}"
    fig = dev.check(snaps, priors)
    fig = dev.check({it: free}, {it: priors[it]}, fig=fig)
    print(fig.line(f"device, case D (B={B}, {'training' if training else 'eval'}), {it} iterations"),
          "| data-dependent and forced snapshots bit-equal:", bit_equal(free, snaps[it], dev.ocfg.sampler.N_samples))
    if B == R.B_RAYS:
        fig.assert_not_soft("D")
    assert fig.exempt == 0


# ---- the 256-wide SDF passes, three and two planes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [3, 2])
@pytest.mark.parametrize("sizes", ["A", "D", "synthetic"])
def test_wide_net_both_plane_counts(sizes, planes):
    """sizes A: N_samples_eval 64 x 10 forced iterations; D: 32 x 5 data-dependent; synthetic: the shipped 128 x 5, data-dependent.  With two
    planes the project has no bar for single SDF values and none is invented: the bookkeeping is still bitwise, and every other stage
    is checked on the device's own SDF row."""
    N_eval, mx = {"A": (64, 10), "D": (32, 5), "synthetic": (128, 5)}[sizes]
    dev = wide_device(N_eval, mx, planes)
    assert dev.eng.sampler_bf16x2 == (planes == 2)
    if sizes == "A":
        snaps, priors = dev.forced(range(1, mx + 1))
        fig = dev.check(snaps, priors, sdf=planes == 3)
    else:
        free = dev.run(force=0)
        dev.check_state(free, free=True)
        it = free.iters
        snaps, priors = dev.forced(range(max(1, it - 1), it + 1))
        fig = dev.check({it: snaps[it]}, {it: priors[it]}, sdf=planes == 3)
        fig = dev.check({it: free}, {it: priors[it]}, sdf=planes == 3, fig=fig)
        print("data-dependent and forced snapshots bit-equal:", bit_equal(free, snaps[it], dev.ocfg.sampler.N_samples))
    print(fig.line(f"device, 256-wide net, sizes {sizes}, {planes} planes"))
    assert fig.exempt == 0


# ---- the initial row and the Lemma-2 beta ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
@pytest.mark.parametrize("training", [False, True])
def test_initial_row_and_beta(name, training):
    """Without a line search (beta_iters = 0) one iteration leaves the initial beta in place wherever the bound at beta0 exceeds eps."""
    ocfg, sd = R.case_oracle(name)
    ocfg.sampler.beta_iters = 0
    conf = R.case_conf(name)
    conf["ray_sampler"]["beta_iters"] = 0
    dev = Device(conf, ocfg, sd, R.case_inputs(name), R.B_RAYS, training)
    s = dev.run(force=1)
    mask = s.beta != torch.tensor(dev.beta0)
    assert int(mask.sum()) >= R.B_RAYS // 3
    fig = R.check_init(s.row, s.beta, ocfg, training, dev.draws.strat_u if training else None, mask)
    print(f"device, case {name} ({'training' if training else 'eval'}): row 0 {fig['row_ulp']:.2f} ulp of far, initial beta {fig['beta_rel']:.1e} "
          f"({int(mask.sum())} of {R.B_RAYS} rays show it)")


# ---- what the loop has no business writing --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,force", [("A", 3), ("A", 10), ("B", 4), ("D", 0)])
def test_workspace_outside_the_rows_is_untouched(name, force):
    dev = plumbing_device(name, training=(name == "D"))
    B, sc = dev.B, dev.ocfg.sampler
    n_ws, guard = R.workspace_floats(B), 64
    ws = torch.full((n_ws + guard,), PATTERN, dtype=torch.int32).view(torch.float32).cuda()
    s = dev.run(force=force, workspace=ws)
    assert dev.eng._last_sampler_ws.data_ptr() == ws.data_ptr()
    w = ws.cpu().view(torch.int32)
    lay = R.layout(B)
    it, N = s.iters, sc.N_samples_eval
    written = {}                                                  # buffer -> longest row it ever held
    for k in range(1, it + 1):
        a = "A" if k % 2 else "B"
        written["z" + a] = written["s" + a] = N * k
        if k > 1:
            written["iB" if k % 2 else "iA"] = N * k
    for name_, (off, rows, width) in lay.items():
        v = w[off:off + rows * width].reshape(rows, width)
        if name_ in ("zA", "zB", "sA", "sB", "iA", "iB"):
            n = written.get(name_, 0)
            assert bool((v[:, n:] == PATTERN).all()), f"{name_}: written past its row of {n}"
            assert not bool((v[:, :n] == PATTERN).any()), f"{name_}: a row of {n} is not fully written"
        elif name_ == "samples":
            n = max(N, sc.N_samples)
            assert bool((v[:, n:] == PATTERN).all()) and not bool((v[:, :n] == PATTERN).any()), "samples"
        elif name_ == "sdf_new":
            assert bool((v.reshape(-1)[B * N:] == PATTERN).all()) and not bool((v.reshape(-1)[:B * N] == PATTERN).any()), "sdf_new"
        elif name_ == "beta":
            assert not bool((v == PATTERN).any())
    end = lay["state"][0] + R.ST_WORDS
    assert bool((w[end:] == PATTERN).all()), "the spare floats behind the state words or the guard behind the workspace were written"
    fig = dev.check({it: s}, {}, sdf=False)                       # and the pattern did not leak into what the loop returned
    assert bool(torch.isfinite(s.z_out).all()) and float(s.z_out.max()) <= 6.0
