"""CPU: the frontier of the network shapes `NetConfig.from_conf` accepts.

a. Python and the C API agree on every conf of a grid around the two base confs: either `from_conf` refuses it with a
   NotImplementedError that names the key and the value, or the descriptor builds and `i2sdf_plan_create` accepts it -- never one
   without the other, never another exception, never a refusal at the first launch (config.py: "refused HERE, with the reason").
b. Every weight stream an accepted shape's kernels walk is a whole number of stages; every stream whose absence tells the library that
   the shape has no such kernel is empty (shapes_ref.span_rule restates the launch sites' conditions; the C++ is not parsed).
c. The inputs of tests/test_gpu_shapes.py leave the oracle's own fp32-vs-fp64 difference at most a quarter of that module's bars and
   keep every ReLU of the radiance net away from zero, so a miss there is the kernel's.

The probe (tests/plan_probe.cpp with csrc/plan.cpp, host code only) and its build recipe are those of tests/test_plan_spans.py."""
import os
import subprocess

import pytest
import torch

import shapes_ref as S
from helpers import rel_max
from test_plan_spans import probe  # noqa: F401  (the module-scoped fixture: one compile for this module)


def _grid():
    """(id, conf, key and value a refusal must name) -- one factor at a time from each base conf, then the twelve cases"""
    out = []
    for width in (256, 64):
        base = S.base_conf(width)
        nh0 = len(base["implicit_network"]["dims"])
        skip0 = base["implicit_network"]["skip_in"]
        nr0 = len(base["rendering_network"]["dims"])
        for nh in (1, 2, 3, 4, 8, 11, 12):
            # (the base skip where the depth has room for it: the factor varied is the depth)
            skip = skip0 if skip0 and skip0[0] < nh else []
            out.append((f"w{width}-sdf{nh}", S.make_conf(width, nh, skip, nr0, None), ("implicit_network.dims", str(nh))))
        for name, skip in (("none", []), ("0", [0]), ("1", [1]), ("nh-1", [nh0 - 1]), ("nh", [nh0])):
            out.append((f"w{width}-skip_{name}", S.make_conf(width, nh0, skip, nr0, None), ("implicit_network.skip_in", str(skip))))
        for nr in (1, 2, 3, 11, 12):
            out.append((f"w{width}-rgb{nr}", S.make_conf(width, nh0, skip0, nr, None), ("rendering_network.dims", str(nr))))
        for light in (None, [32], [64], [96], [100], [128], [256], [512], [64, 64]):
            tag = "none" if light is None else "x".join(map(str, light))
            out.append((f"w{width}-light_{tag}", S.make_conf(width, nh0, skip0, nr0, light), ("light_network.dims", str(light))))
    for c in S.CASES:
        out.append((c.id, S.case_conf(c), None))
    return out


GRID = _grid()
# what the grid must hold whatever the code under test answers: the shapes the issue lists as unrunnable are REFUSED, the cases ACCEPTED
MUST_REFUSE = {f"w{w}-{k}" for w in (256, 64) for k in ("sdf12", "skip_0", "skip_nh", "rgb12", "light_100", "light_512", "light_64x64", "light_64",
                                                         "light_96", "light_256")} | {"w256-light_32", "w64-light_128"}
MUST_ACCEPT = {c.id for c in S.CASES} | {f"w{w}-{k}" for w in (256, 64) for k in ("sdf1", "sdf2", "sdf3", "sdf4", "sdf8", "sdf11", "skip_none", "skip_1",
                                                                                  "skip_nh-1", "rgb1", "rgb2", "rgb3", "rgb11", "light_none")} \
    | {"w256-light_128", "w64-light_32"}


def test_grid_is_decided_in_advance():
    ids = [g[0] for g in GRID]
    assert len(set(ids)) == len(ids)
    assert MUST_REFUSE | MUST_ACCEPT == set(ids) and not (MUST_REFUSE & MUST_ACCEPT)


def _decide(probe_exe, conf, tmp_path):
    """-> ("refused", message) from Python, or ("accepted", probe stdout lines); anything else fails here"""
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.params import ParamLayout
    try:
        cfg = NetConfig.from_conf(conf)
    except NotImplementedError as e:
        return "refused", str(e)
    desc = os.path.join(str(tmp_path), "net.desc")
    with open(desc, "wb") as f:
        f.write(bytes(ParamLayout(cfg).net_desc()))          # (an exception here: accepted in one place, refused in the other)
    r = subprocess.run([probe_exe, desc], capture_output=True, text=True)
    assert r.returncode == 0, f"from_conf accepted what i2sdf_plan_create refuses (probe exit {r.returncode}): {r.stderr[-400:]}"
    return "accepted", r.stdout.splitlines()


@pytest.mark.parametrize("gid", [g[0] for g in GRID])
def test_python_and_c_agree_and_refusals_say_why(probe, tmp_path, gid):  # noqa: F811
    _, conf, names = next(g for g in GRID if g[0] == gid)
    verdict, what = _decide(probe, conf, tmp_path)
    assert verdict == ("refused" if gid in MUST_REFUSE else "accepted"), what if verdict == "refused" else ""
    if verdict == "refused":
        key, value = names
        assert key in what and value in what, f"the refusal names neither {key} nor {value}: {what}"
        assert "instantiated" in what or "kernels" in what, what      # ... and what the kernels exist for


def _desc_of(conf):
    """a descriptor `from_conf` would refuse, built behind its back: what a C caller can hand to i2sdf_plan_create"""
    from i2sdf_amd.params import ParamLayout
    return bytes(ParamLayout(S.unchecked_cfg(conf)).net_desc())


@pytest.mark.parametrize("gid,names", [("w256-light_64", ("light.hidden 64", "128")), ("w64-light_128", ("light.hidden 128", "32")),
                                       ("w256-light_64x64", ("light.n_lin 3", "one hidden layer")), ("w256-light_512", ("light.hidden 512", "128")),
                                       ("w256-skip_nh", ("sdf.skip_layer 8", "n_lin 9")), ("w64-skip_0", ("sdf.skip_layer 0", "n_lin 3"))])
def test_plan_create_refuses_with_a_reason(probe, tmp_path, gid, names):  # noqa: F811
    """the C API on its own: the descriptors of refused confs reach i2sdf_plan_create, which refuses each with its own reason text
    (i2sdf_last_hip_error), before any launch"""
    _, conf, _ = next(g for g in GRID if g[0] == gid)
    desc = os.path.join(str(tmp_path), "net.desc")
    with open(desc, "wb") as f:
        f.write(_desc_of(conf))
    r = subprocess.run([probe, desc], capture_output=True, text=True)
    assert r.returncode == 3 and r.stdout == "", (r.returncode, r.stdout[:200])
    for s in names:
        assert s in r.stderr, r.stderr


@pytest.mark.parametrize("gid", sorted(MUST_ACCEPT))
def test_every_launch_site_of_an_accepted_shape_has_a_whole_span(probe, tmp_path, gid):  # noqa: F811
    from i2sdf_amd.config import NetConfig
    _, conf, _ = next(g for g in GRID if g[0] == gid)
    verdict, lines = _decide(probe, conf, tmp_path)
    assert verdict == "accepted"
    spans = {l.split()[1]: l.split()[2:] for l in lines if l.startswith("span ")}
    cfg = NetConfig.from_conf(conf)
    used, absent = S.span_rule(cfg.sdf.hidden, cfg.sdf.n_lin, cfg.sdf.skip_layer, cfg.rgb.n_lin, cfg.light.hidden if cfg.light else None)
    assert set(used) | set(absent) <= set(spans), sorted((set(used) | set(absent)) - set(spans))
    for k in used:
        assert spans[k] != ["refused"] and int(spans[k][1]) > 0, f"{k}: the shape's kernels walk this stream, the plan has none (or a ragged one)"
    for k in absent:
        assert spans[k] == ["refused"], f"{k}: the shape has no kernel for this stream, the plan emits {spans[k]}"
    chk = dict(l.split()[1:] for l in lines if l.startswith("check "))
    assert chk == {"empty": "0", "backwards": "0", "ragged": "0", "whole": "1"}


@pytest.mark.parametrize("cid", [c.id for c in S.CASES])
def test_oracle_fp32_is_well_inside_the_bars(cid):
    """conditions on the inputs (seeds, points), not measurements of the library: fp32 vs fp64 oracle at most a quarter of each bar, and
    no ReLU of the radiance net so close to zero that fp32 rounding decides its backward mask (shapes_ref.relu_margin)"""
    case = S.BY_ID[cid]
    margin = S.relu_margin(case)
    assert margin >= S.RELU_MARGIN, f"a radiance pre-activation is {margin:.2e} of its layer's scale: closer to zero than {S.RELU_MARGIN:.1e}"
    lo, hi = S.oracle_run(case, torch.float32), S.reference(case)
    assert set(lo) == set(hi)
    worst = {}
    for k in hi:
        e = rel_max(lo[k], hi[k]) if float(hi[k].abs().max()) > 0 else float(lo[k].abs().max())
        kind = "grad" if k.startswith("grad.") else "out"
        if e >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (e, k)
        assert e <= 0.25 * S.bar(k), f"{k}: the oracle's fp32 and fp64 runs differ by {e:.2e}, more than a quarter of the bar {S.bar(k):.0e}"
    print(f"{cid}: fp32 vs fp64 oracle, worst output {worst['out'][0]:.2e} ({worst['out'][1]}), worst gradient {worst['grad'][0]:.2e} ({worst['grad'][1]})")
