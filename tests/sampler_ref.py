"""The error-bounded sampler stage by stage: a reader for the workspace of i2sdf_sample_rays and fp64 checkers, one per stage.

Every checker takes the stage's OWN inputs as the device (or the fp32 oracle) had them -- its row, its SDF row, its prior beta, its
uniforms -- and repeats that one stage in fp64 through oracle.i2sdf_oracle.  Given those inputs a stage is a well-posed function, so no
outlier allowance is needed (tests/test_gpu_sampler.py needs one because it compares the END of the loop, which is ill-conditioned).
Every checker asserts and returns the figures it measured.  Assertion messages start with the checker's name and the sub-check.

The workspace layout is restated here once (csrc/sampler.hip: i2sdf_sampler_workspace_floats and the carve-up at the top of
i2sdf_sample_rays; include/i2sdf.h); tests/test_sampler_ref.py ties the constants to the library."""
from dataclasses import dataclass, replace
from typing import Optional

import torch

from oracle import i2sdf_oracle as orc

NMAX = 640            # capacity of a row (zA, zB, sA, sB, iA, iB), floats / ints per ray
NNEW = 128            # capacity of `samples` and `sdf_new` per ray (`samples` has rows of 128; `sdf_new` is packed, rows of N_eval)
ST_WORDS = 32         # state words, followed by 64 spare floats
ST_TAIL = 64
ST_DONE, ST_ITERS, ST_FLAG0, ST_CNT0 = 0, 1, 2, 16

FAR_ULP = 2.0 ** -21  # ulp of far = 6 (2 * scene_bounding_sphere = 3)
SDF_TOL = 2e-5        # TOL of tests/test_gpu_train_forward.py: the bar of the fp32-equivalent SDF kernels


def workspace_floats(B):
    return B * (NMAX * 6 + NNEW * 2 + 1) + ST_WORDS + ST_TAIL


def layout(B):
    """name -> (offset, rows, width) in floats."""
    out, off = {}, 0
    for name, width in (("zA", NMAX), ("zB", NMAX), ("sA", NMAX), ("sB", NMAX), ("iA", NMAX), ("iB", NMAX), ("samples", NNEW), ("sdf_new", NNEW),
                        ("beta", 1)):
        out[name] = (off, B, width)
        off += B * width
    out["state"] = (off, 1, ST_WORDS)
    return out


@dataclass
class Snap:
    B: int
    N_eval: int
    iters: int
    n: int
    row: torch.Tensor                   # (B, n) the row of the last iteration
    sdf_row: torch.Tensor               # (B, n)
    prev_row: Optional[torch.Tensor]    # (B, n - N_eval) | None (iters == 1)
    prev_sdf: Optional[torch.Tensor]
    idx: Optional[torch.Tensor]         # (B, n) int64: source index of row position in cat([prev_row, new samples])
    samples: torch.Tensor               # (B, >= N_samples) the last inverse-CDF output
    sdf_new: torch.Tensor               # (B, N_eval) sdf at the newest samples of the row
    beta: torch.Tensor                  # (B,)
    state: torch.Tensor                 # (ST_WORDS,) int32
    z_out: Optional[torch.Tensor] = None
    z_eik: Optional[torch.Tensor] = None
    iters_out: Optional[int] = None

    def new_samples(self):
        """The "more" samples of the previous iteration: the row entries with idx >= n_old, in idx order (B, N_eval)."""
        n_old = self.n - self.N_eval
        pos = torch.argsort(self.idx, dim=1, stable=True)[:, n_old:]
        return torch.gather(self.row, 1, pos)

    def copy(self, **kw):
        c = replace(self, **kw)
        for f in ("row", "sdf_row", "prev_row", "prev_sdf", "idx", "samples", "sdf_new", "beta", "state", "z_out", "z_eik"):
            if f not in kw and getattr(c, f) is not None:
                setattr(c, f, getattr(c, f).clone())
        return c


def snapshot(ws, B, N_eval, iters):
    ws = ws.detach().cpu().contiguous()
    assert ws.numel() >= workspace_floats(B)
    lay = layout(B)

    def buf(name, as_int=False):
        off, rows, width = lay[name]
        v = ws[off:off + rows * width]
        if as_int:
            v = v.view(torch.int32)
        return v.reshape(rows, width)

    odd = iters % 2 == 1
    n, n_old = N_eval * iters, N_eval * (iters - 1)
    z_cur, z_prev = (buf("zA"), buf("zB")) if odd else (buf("zB"), buf("zA"))
    s_cur, s_prev = (buf("sA"), buf("sB")) if odd else (buf("sB"), buf("sA"))
    ix = buf("iB" if odd else "iA", True)
    return Snap(B=B, N_eval=N_eval, iters=iters, n=n, row=z_cur[:, :n].clone(), sdf_row=s_cur[:, :n].clone(),
                prev_row=z_prev[:, :n_old].clone() if iters > 1 else None, prev_sdf=s_prev[:, :n_old].clone() if iters > 1 else None,
                idx=ix[:, :n].long() if iters > 1 else None, samples=buf("samples").clone(),
                sdf_new=buf("sdf_new").reshape(-1)[:B * N_eval].reshape(B, N_eval).clone(),     # (packed: the SDF pass writes rows of N_eval)
                beta=buf("beta")[:, 0].clone(), state=buf("state", True)[0].clone())


def snap_from_trace(tr, z_out=None, z_eik=None):
    """The same view of the fp32 oracle's own loop (a SamplerTrace of a run with tr.iters iterations)."""
    k = tr.iters
    B, n = tr.z_rows[-1].shape
    state = torch.zeros(ST_WORDS, dtype=torch.int32)
    state[ST_DONE], state[ST_ITERS] = 1, k
    return Snap(B=B, N_eval=tr.z_rows[0].shape[1], iters=k, n=n, row=tr.z_rows[-1].clone(), sdf_row=tr.sdf_rows[-1].clone(),
                prev_row=tr.z_rows[-2].clone() if k > 1 else None, prev_sdf=tr.sdf_rows[-2].clone() if k > 1 else None,
                idx=tr.sort_idx[-1].clone() if k > 1 else None, samples=tr.new_samples[-1].clone(), sdf_new=tr.sdf_new[-1].clone(),
                beta=tr.betas[-1].clone(), state=state, z_out=z_out, z_eik=z_eik, iters_out=k)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.float()), _bits(b.float()))


# ------------------------------------------------------------------------------------------------------------------------------
def check_init(row0, init_beta, cfg, training, strat_u=None, mask=None):
    """Row 0 vs uniform_z_vals in fp64 (<= 2 ulp of far); the initial beta vs Lemma 2 on that row (relative 1e-6).  `mask` (B,) selects
    the rays whose initial beta is observable."""
    B = row0.shape[0]
    ref = orc.uniform_z_vals(B, cfg, training, None if strat_u is None else strat_u.double(), torch.float64)
    assert row0.shape == ref.shape, f"check_init/row: shape {tuple(row0.shape)} vs {tuple(ref.shape)}"
    row_ulp = float((row0.double() - ref).abs().max()) / FAR_ULP
    assert row_ulp <= 2.0, f"check_init/row: {row_ulp:.2f} ulp of far"
    beta_rel = None
    if init_beta is not None:
        z = row0.double()
        d = z[:, 1:] - z[:, :-1]
        b64 = torch.sqrt((1.0 / (4.0 * torch.log(torch.tensor(cfg.sampler.eps + 1.0, dtype=torch.float64)))) * (d ** 2).sum(-1))
        rel = (init_beta.double() - b64).abs() / b64
        if mask is not None:
            assert bool(mask.any()), "check_init/beta: no ray shows its initial beta"
            rel = rel[mask]
        beta_rel = float(rel.max())
        assert beta_rel <= 1e-6, f"check_init/beta: relative {beta_rel:.2e}"
    return {"row_ulp": row_ulp, "beta_rel": beta_rel}


def check_merge(s: Snap, sdf64=None, tol=SDF_TOL):
    """Sorted, a permutation, old values carried bitwise, ties old-first / new in order, SDF bookkeeping bitwise; with `sdf64`
    (callable: row (B,n) fp64 depths -> fp64 SDF at the device's own points) also the SDF values, max-norm relative `tol`."""
    from helpers import assert_close
    fig = {"sdf_err": None, "ties": 0}
    assert bool((s.row[:, 1:] >= s.row[:, :-1]).all()), "check_merge/sorted: the row decreases somewhere"
    if s.iters > 1:
        n_old = s.n - s.N_eval
        want = torch.arange(s.n).unsqueeze(0).expand(s.B, -1)
        assert torch.equal(torch.sort(s.idx, dim=1)[0], want), "check_merge/perm: idx is not a permutation of 0..n-1"
        old = s.idx < n_old
        src = torch.gather(s.prev_row, 1, s.idx.clamp_max(n_old - 1))
        assert torch.equal(_bits(s.row)[old], _bits(src)[old]), "check_merge/carry: row[j] != prev_row[idx[j]] bitwise"
        tie = s.row[:, 1:] == s.row[:, :-1]
        fig["ties"] = int(tie.sum())
        assert bool((s.idx[:, 1:] > s.idx[:, :-1])[tie].all()), "check_merge/tie: equal depths not ordered old first, new in order"
        both = torch.cat([s.prev_sdf, s.sdf_new], 1)
        assert torch.equal(_bits(s.sdf_row), _bits(torch.gather(both, 1, s.idx))), "check_merge/sdf: sdf_row[j] != source[idx[j]] bitwise"
    else:
        assert torch.equal(_bits(s.sdf_row), _bits(s.sdf_new)), "check_merge/sdf: sdf row 0 is not sdf_new bitwise"
    if sdf64 is not None:
        fig["sdf_err"] = assert_close(s.sdf_row, sdf64(s.row.double()).float(), tol, "check_merge/value: sdf row")
    return fig


def _beta0(sd, cfg):
    return float(orc.get_beta({"density.beta": sd["density.beta"].float()}, cfg))


def check_beta(s: Snap, prior_beta, sd, cfg):
    """The line search in fp64 from the device's prior beta on the device's row: |beta - beta64| <= 2 w + 1e-6 beta64 with
    w = (beta_start - beta0) / 2^beta_iters.  A ray over the bar is exempt only where fp64 met a midpoint (or beta0) whose error is
    within 1e-5 eps of eps; at most 1 % of the rays."""
    sc = cfg.sampler
    z, d = s.row.double(), s.sdf_row.double()
    dists = z[:, 1:] - z[:, :-1]
    ds = orc.d_star_bound(z, d)
    b0 = torch.full((s.B,), _beta0(sd, cfg), dtype=torch.float64)
    err = orc.error_bound(b0.unsqueeze(-1), d, dists, ds)
    near = (err - sc.eps).abs() <= 1e-5 * sc.eps
    ok = err <= sc.eps
    b_max = torch.where(ok, b0, prior_beta.double())
    b_min = b0.clone()
    w = (b_max - b0) / 2.0 ** sc.beta_iters
    for _ in range(sc.beta_iters):
        b_mid = (b_min + b_max) / 2.0
        err = orc.error_bound(b_mid.unsqueeze(-1), d, dists, ds)
        near |= (err - sc.eps).abs() <= 1e-5 * sc.eps
        ok = err <= sc.eps
        b_max = torch.where(ok, b_mid, b_max)
        b_min = torch.where(ok, b_min, b_mid)
    dev = (s.beta.double() - b_max).abs()
    over = dev > 2.0 * w + 1e-6 * b_max
    bad = over & ~near
    widths = torch.where(w > 0, dev / w.clamp_min(1e-300), torch.zeros_like(dev))
    fig = {"widths": float(widths[~over].max()) if bool((~over).any()) else 0.0, "exempt": int((over & near).sum()), "rays": s.B,
           "beta0_rays": int((b_max == b0).sum())}
    assert not bool(bad.any()), (f"check_beta/bar: {int(bad.sum())} rays over the bar, worst {float((dev / w.clamp_min(1e-300))[bad].max()):.2f} "
                                 f"bracket widths (ray {int(bad.nonzero()[0])})")
    assert fig["exempt"] <= 0.01 * s.B, f"check_beta/exempt: {fig['exempt']} of {s.B} rays exempted"
    return fig


def _F(z, cdf, x, right):
    """The piecewise-linear CDF through (z, cdf) at x; duplicate knots: left-continuous (right=False) / right-continuous value."""
    n = z.shape[1]
    j = torch.searchsorted(z, x.contiguous(), right=right)
    lo, hi = (j - 1).clamp(0, n - 1), j.clamp(0, n - 1)
    z0, z1 = torch.gather(z, 1, lo), torch.gather(z, 1, hi)
    c0, c1 = torch.gather(cdf, 1, lo), torch.gather(cdf, 1, hi)
    t = torch.where(z1 > z0, (x - z0) / (z1 - z0).clamp_min(1e-300), torch.zeros_like(x))
    return c0 + t * (c1 - c0)


def pdf64(row, sdf_row, beta, which, add_tiny):
    """The pdf that ran, in fp64 -> (cdf (B,n), tol (B,))."""
    z, d, b = row.double(), sdf_row.double(), beta.double().unsqueeze(-1)
    dists = z[:, 1:] - z[:, :-1]
    fe = dists * orc.laplace_density(d, b)[:, :-1]
    T = torch.exp(-(torch.cumsum(fe, -1) - fe))
    if which == "more":
        ds = orc.d_star_bound(z, d)
        g = torch.clamp(torch.exp(torch.cumsum(torch.exp(-ds / b) * dists ** 2 / (4 * b ** 2), -1)), max=1.0e6)
        pdf, num = (g - 1.0) * T + add_tiny, (g * T).sum(-1)
    else:
        pdf, num = (1.0 - torch.exp(-fe)) * T + 1e-5, T.sum(-1)
    tot = pdf.sum(-1)
    cdf = torch.cat([torch.zeros_like(tot).unsqueeze(-1), torch.cumsum(pdf, -1) / tot.unsqueeze(-1)], -1)
    return cdf, 2.0 ** -23 * num / tot + 2e-6


def check_resample(row, sdf_row, beta, smp, u, which, add_tiny):
    """Inverse-CDF samples `smp` (B,N) for uniforms `u` (N,) | (B,N) against the fp64 CDF of the pdf that ran on (row, sdf_row, beta),
    in CDF space: F(s - delta, left) - tol <= u <= F(s + delta, right) + tol, delta = 4 ulp(far).  Brackets that the reference's
    `denom < 1e-5 -> 1` rule flattens (fp64 test: 2e-5) only need z[below] - delta <= s <= z[above] + delta."""
    assert which in ("more", "final")
    B, n = row.shape
    z, s = row.double(), smp.double()
    u = u.double().expand(B, -1) if u.dim() == 2 else u.double().unsqueeze(0).expand(B, -1)
    assert s.shape == u.shape, f"check_resample/{which}: {tuple(s.shape)} samples for {tuple(u.shape)} uniforms"
    assert bool(torch.isfinite(s).all()), f"check_resample/{which}: non-finite samples"
    cdf, tol = pdf64(row, sdf_row, beta, which, add_tiny)
    delta = 4.0 * FAR_ULP
    inds = torch.searchsorted(cdf, u.contiguous(), right=True)
    below = (inds - 1).clamp(0, n - 2)          # (u = 0 or 1 can land past either end by rounding: the end bracket is the proper one)
    above = below + 1
    flat = (torch.gather(cdf, 1, above) - torch.gather(cdf, 1, below)) < 2e-5
    zb, za = torch.gather(z, 1, below), torch.gather(z, 1, above)
    bad_flat = flat & ((s < zb - delta) | (s > za + delta))
    assert not bool(bad_flat.any()), (f"check_resample/{which}/flat: {int(bad_flat.sum())} samples of flattened brackets outside their bracket "
                                      f"(first: ray, k = {bad_flat.nonzero()[0].tolist()})")
    over = torch.maximum(_F(z, cdf, s - delta, False) - u, u - _F(z, cdf, s + delta, True)).clamp_min(0.0) / tol.unsqueeze(-1)
    over = torch.where(flat, torch.zeros_like(over), over)
    fig = {"used": float(over.max()), "flat": int(flat.sum()), "samples": int(flat.numel()), "tol_small": float((tol < 1e-4).double().mean()),
           "tol_max": float(tol.max())}
    assert fig["used"] <= 1.0, (f"check_resample/{which}/cdf: a sample is {fig['used']:.2f} tol from its uniform in CDF space "
                                f"(ray, k = {(over == over.max()).nonzero()[0].tolist()})")
    return fig


def extra_index(s: Snap, cfg, training, extra_idx):
    sc = cfg.sampler
    if sc.N_samples_extra <= 0:
        return None
    if training:
        idx = extra_idx.long()
        return idx[s.iters - 1] if idx.dim() == 2 else idx
    return torch.linspace(0, s.n - 1, sc.N_samples_extra).long()


def compose_final(s: Snap, cfg, training, extra_idx):
    sc = cfg.sampler
    parts = [s.samples[:, :sc.N_samples], torch.full((s.B, 1), sc.near), torch.full((s.B, 1), 2.0 * cfg.scene_bounding_sphere)]
    idx = extra_index(s, cfg, training, extra_idx)
    if idx is not None:
        parts.append(s.row[:, idx.clamp(0, s.n - 1)])
    return torch.sort(torch.cat(parts, -1).float(), -1)[0]


def check_final(s: Snap, cfg, training, extra_idx=None, eik_idx=None):
    """z_out bitwise sort(samples U {near, far} U row[extra]); z_eik = z_out[eik_idx]; the reported iteration count."""
    want = compose_final(s, cfg, training, extra_idx)
    assert s.z_out.shape == want.shape, f"check_final/z_out: shape {tuple(s.z_out.shape)} vs {tuple(want.shape)}"
    same = _bits(s.z_out.float()) == _bits(want)
    assert bool(same.all()), f"check_final/z_out: {int((~same).sum())} depths differ bitwise (first: ray, k = {(~same).nonzero()[0].tolist()})"
    if s.z_eik is not None:
        e = eik_idx.long().reshape(-1, 1) if (training and eik_idx is not None) else torch.zeros(s.B, 1, dtype=torch.long)
        assert _same_bits(s.z_eik.reshape(-1, 1), torch.gather(s.z_out, 1, e)), "check_final/z_eik: z_eik != z_out[eik_idx]"
    assert int(s.state[ST_ITERS]) == s.iters and int(s.iters_out) == int(s.state[ST_ITERS]), \
        f"check_final/iters: reported {s.iters_out}, state word {int(s.state[ST_ITERS])}, snapshot {s.iters}"
    return {}


# ------------------------------------------------------------------------------------------------------------------------------
class Figures:
    """What a case measured, merged over its iterations; `assert_not_soft` holds the two conditions that keep check_resample honest."""

    def __init__(self):
        self.used = {"more": 0.0, "final": 0.0}
        self.flat = {"more": [0, 0], "final": [0, 0]}
        self.tol_small = {"more": [], "final": []}
        self.widths, self.exempt, self.rays = 0.0, 0, 0
        self.sdf_err, self.row_ulp, self.beta_rel = None, None, None

    def resample(self, which, fig):
        self.used[which] = max(self.used[which], fig["used"])
        self.flat[which][0] += fig["flat"]; self.flat[which][1] += fig["samples"]
        self.tol_small[which].append(fig["tol_small"])

    def beta(self, fig):
        self.widths = max(self.widths, fig["widths"]); self.exempt += fig["exempt"]; self.rays += fig["rays"]

    def merge(self, fig):
        if fig.get("sdf_err") is not None:
            self.sdf_err = max(self.sdf_err or 0.0, fig["sdf_err"])

    def init(self, fig):
        self.row_ulp = max(self.row_ulp or 0.0, fig["row_ulp"])
        if fig["beta_rel"] is not None:
            self.beta_rel = max(self.beta_rel or 0.0, fig["beta_rel"])

    def flat_share(self):
        f = sum(v[0] for v in self.flat.values()); t = sum(v[1] for v in self.flat.values())
        return f / max(t, 1)

    def tol_share(self):
        return min((min(v) for v in self.tol_small.values() if v), default=1.0)

    def assert_not_soft(self, what=""):
        assert self.flat_share() <= 0.10, f"{what}: {self.flat_share() * 100:.1f}% of the samples sit in flattened brackets"
        assert self.tol_share() >= 1.0 / 3.0, f"{what}: only {self.tol_share() * 100:.0f}% of the rays of some stage have tol < 1e-4"

    def line(self, what):
        o = lambda v, f: "-" if v is None else format(v, f)
        return (f"{what}: used tol more {self.used['more']:.3f} final {self.used['final']:.3f} | beta {self.widths:.2f} widths, {self.exempt} exempt of "
                f"{self.rays} | flat {self.flat_share() * 100:.2f}% | tol<1e-4 {self.tol_share():.2f} | row0 {o(self.row_ulp, '.2f')} ulp, "
                f"beta_init {o(self.beta_rel, '.1e')} | sdf {o(self.sdf_err, '.2e')}")


CHECKERS = ("init", "merge", "beta", "resample", "final")


def check_run(snaps, priors, sd, cfg, training, u_more, u_final, extra_idx=None, eik_idx=None, strat_u=None, sdf64=None, init_beta=None,
              init_mask=None, fig=None, only=None, sdf_last_only=False):
    """Every checker on the snapshots of one case.  snaps: {k: Snap of the run with k iterations}; priors: {k: prior beta of iteration k}
    (k = 1: the initial beta where it is known).  `only`: a set of checker names to run (teeth tests).  `sdf_last_only`: SDF values of the
    longest row only (every earlier value is in it, carried bitwise -- which check_merge asserts)."""
    fig = fig or Figures()
    sc = cfg.sampler
    want = lambda c: only is None or c in only
    for k in sorted(snaps):
        s = snaps[k]
        if k == 1 and want("init"):
            fig.init(check_init(s.row, init_beta, cfg, training, strat_u, init_mask))
        if want("merge"):
            fig.merge(check_merge(s, sdf64 if (not sdf_last_only or k == max(snaps)) else None))
        if want("beta") and priors.get(k) is not None:
            fig.beta(check_beta(s, priors[k], sd, cfg))
        if want("resample"):
            fig.resample("final", check_resample(s.row, s.sdf_row, s.beta, s.samples[:, :sc.N_samples], u_final, "final", sc.add_tiny))
            if k > 1 and priors.get(k) is not None:     # the "more" step of iteration k-1 ran on the previous row with beta_{k-1} = this prior
                fig.resample("more", check_resample(s.prev_row, s.prev_sdf, priors[k], s.new_samples(), u_more, "more", sc.add_tiny))
        if want("final") and s.z_out is not None:
            check_final(s, cfg, training, extra_idx, eik_idx)
    return fig


# ------------------------------------------------------------------------------------------------------------------------------
# the cases both test modules run (plumbing-skip net, 37 rays)
CASES = {
    "A": dict(N_eval=64, max_iters=10, force=tuple(range(1, 11)), beta=0.03, cam=(0.0, 0.2, -1.8)),    # every E 1..10, full lanes
    "B": dict(N_eval=100, max_iters=6, force=tuple(range(1, 7)), beta=0.03, cam=(0.0, 0.2, -1.8)),     # E 2,4,5,7,8,10, ragged last lane
    "C": dict(N_eval=36, max_iters=12, force=tuple(range(1, 13)), beta=0.01, cam=(0.0, 0.2, -1.8)),    # state words up to it = 11, n = 432
    "D": dict(N_eval=32, max_iters=5, force=(0,), beta=0.03, cam=(0.0, 0.2, -1.8)),                    # data-dependent: split kernels, ST_DONE
    "E": dict(N_eval=64, max_iters=10, force=tuple(range(1, 11)), beta=0.1, cam=(0.1, -0.2, 0.3)),     # inside: every ray hits
}
B_RAYS = 37


def case_oracle(name):
    c = CASES[name]
    ocfg = orc.plumbing_cfg(skip=True)
    ocfg.sampler.N_samples_eval, ocfg.sampler.max_total_iters = c["N_eval"], c["max_iters"]
    sd = orc.perturb_params(orc.init_params(ocfg, seed=23), 0.05, seed=24)
    sd["density.beta"] = torch.tensor(c["beta"])
    return ocfg, sd


def case_conf(name):
    from i2sdf_amd.config import plumbing_conf
    conf = plumbing_conf(skip=True)
    conf["ray_sampler"].update({"N_samples_eval": CASES[name]["N_eval"], "max_total_iters": CASES[name]["max_iters"]})
    return conf


def case_inputs(name, B=B_RAYS):
    from helpers import camera_inputs
    return camera_inputs(B, CASES[name]["cam"], W=32, H=32, f=30.0, seed=3, train_layout=False)


def case_draws(ocfg, B, seed=1):
    """Per-ray strat_u / cdf_u, eik_idx and a 2-D extra_idx: one randperm row per possible loop length."""
    from helpers import make_draws
    sc = ocfg.sampler
    rows = [make_draws(ocfg, B, n_row=sc.N_samples_eval * (it + 1), seed=seed + 10 * it).extra_idx for it in range(sc.max_total_iters)]
    dr = make_draws(ocfg, B, n_row=sc.N_samples_eval, seed=seed)
    dr.extra_idx = torch.stack(rows)
    return dr


def sdf64_fn(sd, ocfg, cam, dirs):
    sd64 = {k: v.double() for k, v in sd.items()}
    cam, dirs = cam.double().cpu(), dirs.double().cpu()

    def f(row):
        pts = (cam.unsqueeze(1) + row.unsqueeze(2) * dirs.unsqueeze(1)).reshape(-1, 3)
        with torch.no_grad():
            return orc.sdf_forward(sd64, ocfg.sdf, pts)[:, :1].reshape(row.shape)
    return f


def oracle_snap(sd, ocfg, cam, dirs, training, draws=None, force=None):
    """One run of the fp32 oracle -> (Snap, prior beta of its last iteration, initial beta)."""
    tr = orc.SamplerTrace(stable_sort=True)
    z_out, z_eik = orc.sample_z_vals(sd, ocfg, dirs, cam, training=training, draws=draws, force_iters=force, trace=tr)
    return snap_from_trace(tr, z_out, z_eik), tr.prior_betas[-1], tr.prior_betas[0]
