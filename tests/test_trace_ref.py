"""CPU: tests/trace_ref.py, the restatement of the sphere-tracing rule (include/i2sdf.h), against closed forms (a sphere and a plane: hit,
graze, miss, origin inside), fp32 against fp64 on the oracle's networks, and against five wrong rules, each of which one checker below
must catch -- so the restatement the GPU tests replay the device against is itself pinned down."""
import numpy as np
import pytest

import trace_ref as TR
from oracle import i2sdf_oracle as orc

F32, F64 = np.float32, np.float64


def sphere(slope=1.0, radius=1.0):
    return lambda x: (slope * (np.sqrt((x * x).sum(1)) - radius)).astype(x.dtype)


def plane(x):          # the half space z < 0 is inside
    return x[:, 2].copy()


def _one(o, d):
    return np.array([o], dtype=F64), np.array([d], dtype=F64)


# ---- the checkers: each takes the tracer (trace_ref.trace with or without a mutation bound in) -----------------------------------------
def check_sphere_hits(trace, dtype):
    """rays through a unit sphere, on and off its axis: HIT within eps of the closed-form depth, in a handful of steps"""
    rng = np.random.default_rng(0)
    n = 64
    o = np.tile(np.array([[0.0, 0.0, -3.0]]), (n, 1))
    target = np.concatenate([np.zeros((1, 3)), rng.uniform(-0.4, 0.4, (n - 1, 3))])
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = (o * d).sum(1)
    t_exact = -b - np.sqrt(b * b - ((o * o).sum(1) - 1.0))
    t, status, steps = trace(sphere(), o, d, 0.0, 6.0, dtype=dtype)
    assert (status == TR.HIT).all()
    # f is convex along a ray and 0 <= f <= eps where the march stops, so the tangent at the crossing bounds the distance to it:
    # 0 <= t_exact - t <= eps / |d . grad f(x_exact)|, grad f = x / |x|  (+ the fp32 rounding of points and depths of size ~3)
    slope = np.abs(((o + t_exact[:, None] * d) * d).sum(1))
    err = t_exact - t.astype(F64)
    tol = 4e-6 if dtype == F32 else 1e-12
    assert (err >= -tol).all() and (err <= 1e-4 / slope + tol).all(), (err.min(), (err * slope).max())
    assert steps.min() >= 2 and steps.max() <= 40
    assert steps[0] == 2            # on the axis: f(0) = 2 exactly, t = 2, f = 0


def check_steep_sphere(trace, dtype):
    """|grad| = 2.5: every step overshoots by 1.5 times the distance, and only the bracket brings the ray back"""
    o, d = _one([0.0, 0.0, -2.0], [0.0, 0.0, 1.0])
    t, status, steps = trace(sphere(2.5), o, d, 0.0, 5.0, dtype=dtype)
    assert status[0] == TR.HIT and abs(float(t[0]) - 1.0) <= 1e-4 / 2.5 + 1e-6 and steps[0] <= 24


def check_miss_at_t1(trace, dtype):
    """moving away from a plane: f = 1 + t, so the first step lands exactly on t1 = 1: MISS there, after one step (tn >= t1)"""
    o, d = _one([0.0, 0.0, 1.0], [0.0, 0.0, 1.0])
    t, status, steps = trace(plane, o, d, 0.0, 1.0, dtype=dtype)
    assert status[0] == TR.MISS and t[0] == 1.0 and steps[0] == 1


def check_collapse(trace, dtype):
    """eps far below the resolution of t: the bracket collapses and the HIT is reported on its inside end, f(t) < 0"""
    o, d = _one([0.3, -0.2, -3.0], [0.0, 0.0, 1.0])
    o, d = np.tile(o, (4, 1)), np.tile(d, (4, 1))
    o[:, 0] += np.arange(4) * 0.1
    f = sphere(1.7)
    t, status, steps = trace(f, o, d, 0.0, 6.0, eps=1e-30, max_steps=200, dtype=dtype)
    assert (status == TR.HIT).all()
    ft = f(TR.points(o.astype(dtype), d.astype(dtype), t))
    assert ((ft < 0) | (np.abs(ft) <= 1e-30)).all(), ft
    prev = np.nextafter(t, dtype(0))
    assert (f(TR.points(o.astype(dtype), d.astype(dtype), prev)) >= 0).all()      # one step of t back is outside: the crossing is bracketed


def check_inside(trace, dtype):
    """an origin behind the surface: INSIDE after one step, t = t0"""
    o, d = _one([0.0, 0.1, 0.2], [0.0, 0.0, 1.0])
    t, status, steps = trace(sphere(), o, d, 0.25, 5.0, dtype=dtype)
    assert status[0] == TR.INSIDE and t[0] == dtype(0.25) and steps[0] == 1


def check_steps_count(trace, dtype):
    """steps = the number of sdf evaluations of the ray"""
    calls = []

    def counting(x):
        calls.append(x.shape[0])
        return sphere()(x)
    o, d = _one([0.0, 0.5, -3.0], [0.0, 0.0, 1.0])
    t, status, steps = trace(counting, o, d, 0.0, 6.0, dtype=dtype)
    assert status[0] == TR.HIT and steps[0] == len(calls) == sum(calls)
    t, status, steps = trace(sphere(), o, d, 0.0, 6.0, max_steps=3, dtype=dtype)
    assert status[0] == TR.UNRESOLVED and steps[0] == 3


CHECKERS = {"no_bracket": check_steep_sphere, "gt_at_t1": check_miss_at_t1, "collapse_lo": check_collapse,
            "first_negative_brackets": check_inside, "steps_off_by_one": check_steps_count}


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_closed_forms(dtype):
    check_sphere_hits(TR.trace, dtype)
    for chk in CHECKERS.values():
        chk(TR.trace, dtype)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_graze_miss_and_degenerate_intervals(dtype):
    d = np.array([[0.0, 0.0, 1.0]] * 2)
    o = np.array([[1.0 - 1e-3, 0.0, -3.0], [1.0 + 1e-3, 0.0, -3.0]])           # impact parameters either side of the radius
    t, status, steps = TR.trace(sphere(), o, d, 0.0, 6.0, max_steps=512, dtype=dtype)
    assert status[0] == TR.HIT and status[1] == TR.MISS and t[1] == dtype(6.0)
    t_exact = 3.0 - np.sqrt(1.0 - (1.0 - 1e-3) ** 2)
    # |d . grad| = sqrt(1 - b^2) = 0.0447 at this graze: eps / that, doubled for the curvature over the last step
    assert abs(float(t[0]) - t_exact) <= 2 * 1e-4 / 0.0447
    assert steps[1] > steps[0] > 8                                               # the near miss crawls past the sphere
    # a plain miss costs few steps; an empty, reversed or NaN interval none
    o2, d2 = _one([0.0, 2.0, -3.0], [0.0, 0.0, 1.0])
    t, status, steps = TR.trace(sphere(), o2, d2, 0.0, 6.0, dtype=dtype)
    assert status[0] == TR.MISS and t[0] == dtype(6.0) and steps[0] <= 6
    o3, d3 = np.tile(o2, (3, 1)), np.tile(d2, (3, 1))
    t, status, steps = TR.trace(sphere(), o3, d3, np.array([1.0, 2.0, 0.0]), np.array([1.0, 1.0, np.nan]), dtype=dtype)
    assert (status == TR.MISS).all() and (steps == 0).all() and (t == np.array([1.0, 2.0, 0.0], dtype=dtype)).all()
    # a non-finite sdf value: UNRESOLVED where it stands
    t, status, steps = TR.trace(lambda x: np.full(x.shape[0], np.inf, x.dtype), o2, d2, 0.5, 6.0, dtype=dtype)
    assert status[0] == TR.UNRESOLVED and t[0] == dtype(0.5) and steps[0] == 1


@pytest.mark.parametrize("mutation", TR.MUTATIONS)
def test_each_wrong_rule_is_caught(mutation):
    from functools import partial
    for dtype in (F32, F64):
        with pytest.raises(AssertionError):
            CHECKERS[mutation](partial(TR.trace, mutate=mutation), dtype)


def test_replay_reproduces_the_march():
    o, d, t0, t1 = TR.make_rays(200, seed=5)
    f = sphere(1.4, 0.8)
    t, status, steps, ftr = TR.trace(f, o, d, t0, t1, return_f=True)
    t2, status2, steps2 = TR.trace(None, o, d, t0, t1, replay=ftr)
    assert t.tobytes() == t2.tobytes() and (status == status2).all() and (steps == steps2).all()
    assert len(set(status.tolist())) >= 2


@pytest.mark.parametrize("which", ["plumbing", "plumbing_skip", "synthetic"])
def test_fp32_against_fp64_on_the_oracle_nets(which):
    """The nets of the GPU tests (tests/test_gpu_trace.py).  The two marches see sdf values ~1e-7 apart; they may take different steps, but they
    end on the same surface: the same status except where it is decided within rounding (a graze), and on a hit that is well posed
    (|d . grad sdf| >= 0.2) depths within 2 eps / |d . grad sdf| (each stops within eps of zero)."""
    ocfg = orc.synthetic_cfg() if which == "synthetic" else orc.plumbing_cfg(skip=which.endswith("skip"))
    sd = orc.perturb_params(orc.init_params(ocfg, seed=3), 0.05)
    n = 96 if which == "synthetic" else 384
    o, d, t0, t1 = TR.make_rays(n, seed=11)
    t32, s32, n32 = TR.trace(TR.oracle_sdf(sd, ocfg, F32), o, d, t0, t1, dtype=F32)
    t64, s64, n64 = TR.trace(TR.oracle_sdf(sd, ocfg, F64), o, d, t0, t1, dtype=F64)
    assert (s32 != s64).mean() <= 0.01
    both = (s32 == TR.HIT) & (s64 == TR.HIT)
    assert both.sum() >= n // 4
    import torch
    x = torch.from_numpy(TR.points(o.astype(F64), d.astype(F64), t64)[both])
    g = orc.sdf_gradient({k: v.double() for k, v in sd.items()}, ocfg.sdf, x).numpy()
    slope = np.abs((g * d[both].astype(F64)).sum(1))
    well = slope >= 0.2
    assert well.mean() >= 0.9
    used = np.abs(t32[both].astype(F64) - t64[both])[well] * slope[well] / 2e-4
    print(f"{which}: {both.sum()} common hits, {well.mean() * 100:.1f} % well posed, largest used fraction of 2 eps / slope {used.max():.3f}, "
          f"steps at most {n32[both].max()}")
    assert used.max() <= 1.0
