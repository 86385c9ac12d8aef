"""The marching rule of i2sdf_trace_rays (include/i2sdf.h, "Sphere tracing") restated with numpy, in fp32 or fp64, over any sdf(x) callable.
numpy rounds every fp32 operation once and contracts nothing, so in fp32 this IS the arithmetic of the device rule: given the f the
device saw at every step (`replay`), it must reproduce t, status and steps bit for bit.  Test infrastructure, not a product path."""
import numpy as np
import torch

ACTIVE, HIT, MISS, UNRESOLVED, INSIDE = 0, 1, 2, 3, 4
MUTATIONS = ("no_bracket", "gt_at_t1", "collapse_lo", "first_negative_brackets", "steps_off_by_one")


def points(o, d, t):
    """o + (t * d): the multiply and the add each rounded once, as fetch_point forms a ray point"""
    return o + t[:, None] * d


def trace(sdf, o, d, t0, t1, eps=1e-4, max_steps=64, step_scale=1.0, dtype=np.float32, mutate=None, replay=None, return_f=False, return_t=False):
    """sdf: (n, 3) array of `dtype` -> (n,) values (called on the ACTIVE rays only), or None with replay = (max_steps, N) array: the f of
    every step is then read from there.  o, d (N, 3); t0, t1 numbers or (N,).  mutate: one of MUTATIONS, a deliberately wrong rule (the
    tests show that each one is caught).  -> t (N,) dtype, status (N,) int32, steps (N,) int32 [, f_trace (max_steps, N), NaN where no step] [, t_trace (max_steps, N): the depth each
    step was evaluated at, NaN where no step]."""
    assert mutate is None or mutate in MUTATIONS
    o, d = np.ascontiguousarray(o, dtype=dtype), np.ascontiguousarray(d, dtype=dtype)
    N = o.shape[0]
    t0 = np.broadcast_to(np.asarray(t0, dtype=dtype), (N,)).copy()
    t1 = np.broadcast_to(np.asarray(t1, dtype=dtype), (N,)).copy()
    eps_, scale_, half = dtype(eps), dtype(step_scale), dtype(0.5)
    with np.errstate(invalid="ignore"):
        status = np.where(t1 > t0, ACTIVE, MISS).astype(np.int32)
    t, lo, hi = t0.copy(), t0.copy(), t0.copy()
    bracketed = np.zeros(N, dtype=bool)
    steps = np.zeros(N, dtype=np.int32)
    f_trace = np.full((max_steps, N), np.nan, dtype=dtype)
    t_trace = np.full((max_steps, N), np.nan, dtype=dtype)
    for s in range(max_steps):
        a = np.nonzero(status == ACTIVE)[0]
        if a.size == 0:
            break
        f = np.asarray(replay[s, a], dtype=dtype) if sdf is None else np.asarray(sdf(points(o[a], d[a], t[a])), dtype=dtype).reshape(-1)
        f_trace[s, a] = f
        t_trace[s, a] = t[a]
        steps[a] += 1
        with np.errstate(invalid="ignore", over="ignore"):
            for i, r in enumerate(a):                      # per ray, in the order the rule is written
                fi = f[i]
                if not np.isfinite(fi):
                    status[r] = UNRESOLVED
                    continue
                if abs(fi) <= eps_:
                    status[r] = HIT
                    continue
                if fi < 0 and steps[r] == 1 and mutate != "first_negative_brackets":
                    status[r], t[r] = INSIDE, t0[r]
                    continue
                if fi < 0 and mutate != "no_bracket":
                    hi[r], bracketed[r] = t[r], True
                else:
                    lo[r] = t[r]
                if bracketed[r]:
                    tn = dtype(lo[r] + dtype(half * dtype(hi[r] - lo[r])))
                    if tn == lo[r] or tn == hi[r]:
                        status[r], t[r] = HIT, (lo[r] if mutate == "collapse_lo" else hi[r])
                        continue
                else:
                    tn = dtype(t[r] + dtype(scale_ * fi))
                    if (tn > t1[r]) if mutate == "gt_at_t1" else (tn >= t1[r]):
                        status[r], t[r] = MISS, t1[r]
                        continue
                t[r] = tn
    status[status == ACTIVE] = UNRESOLVED
    if mutate == "steps_off_by_one":
        steps = np.maximum(steps - 1, 0).astype(np.int32)
    return (t, status, steps) + ((f_trace,) if return_f else ()) + ((t_trace,) if return_t else ())


def oracle_sdf(sd, cfg, dtype):
    """sdf(x) of the oracle's network in torch on the CPU, as a numpy callable for trace(); dtype np.float32 / np.float64"""
    from oracle import i2sdf_oracle as orc
    td = torch.float32 if dtype == np.float32 else torch.float64
    sd_ = {k: v.to(td) for k, v in sd.items()}

    def f(x):
        with torch.no_grad():
            return orc.sdf_forward(sd_, cfg.sdf, torch.from_numpy(np.ascontiguousarray(x)).to(td))[:, 0].numpy()
    return f


def make_rays(n, seed, radius=3.0, r_lo=1.5, r_hi=2.5, box=0.9):
    """n rays with origins on radii r_lo..r_hi aimed into the cube of +-box, and the interval [0, exit of the sphere of `radius`]: fp32
    arrays o, d (unit to fp32 rounding), t0, t1.  (The origins lie inside the bounding sphere, so the clipped interval starts at 0.)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    o = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(r_lo, r_hi, (n, 1))
    target = rng.uniform(-box, box, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = (o * d).sum(1)
    t1 = -b + np.sqrt(b * b - ((o * o).sum(1) - radius * radius))
    return o.astype(np.float32), d.astype(np.float32), np.zeros(n, np.float32), t1.astype(np.float32)

