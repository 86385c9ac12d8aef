"""CPU: i2sdf_weight_grads enqueues the launches it enqueued before its driver became data.

csrc/wgrad_plan.h turns (plan, training buffers) into a list of passes -- kernel, threads, LDS bytes, stream, WgLaunch batches -- and
wgrad.hip only enqueues them.  A task in the wrong launch, or one wrong field of a WgTask, is not a failing assertion on the device but a
wrong or missing block of a gradient (or a read past a tensor), so the whole list is pinned here, on the CPU.

tests/wgrad_probe.cpp is compiled together with csrc/plan.cpp (host code only, no GPU: a plan without a device keeps its host-side table)
and prints every pass with every WgTask / WgJob field, operand pointers as offsets from fake bases, and the table of the final reduction.

tests/golden/wgrad_plan/<case>.txt were recorded from the logic of commit 2fb3451, the last one whose driver was the tail of wgrad.hip, not
from the code under test: a throwaway header with the probe's interface that held that commit's `Src`, `TaskList`, `fill_wn`, the task
building, the `variant` rule, the three selections (`sel_narrow`, `sel_blocks`, `sel_all`), the `merged` rule and the launch sequence of
both shapes as verbatim line ranges of its wgrad.hip, with the body of its `launch` lambda recording (kernel, threads, LDS bytes, stream,
the WgLaunch it had filled) where it launched; this probe was compiled against that header and run over the cases below, with
I2SDF_WGRAD_MERGED and I2SDF_WGRAD_BLOCKS_FIRST unset."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i2sdf_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_plan")

X3, BLOCKED, X2, PARTS, SAVES24 = 2, 128, 256, 512, 2048        # include/i2sdf.h: I2SDF_OPT_*
M_SDF, M_MAIN = 2 * 2048 + 200, 2048 + 300                     # three chunks, the last partly filled; the radiance points end inside the second


def _confs():
    from i2sdf_amd.config import synthetic_conf, plumbing_conf
    deep = synthetic_conf()                                     # twelve layers per net: more split-arithmetic tasks than one WgLaunch holds
    deep["implicit_network"]["dims"] = [256] * 11
    deep["implicit_network"]["skip_in"] = [5]
    deep["rendering_network"]["dims"] = [256] * 11
    return {"synthetic": synthetic_conf(), "synthetic_light": synthetic_conf(True), "plumbing": plumbing_conf(),
            "plumbing_skip_light": plumbing_conf(True, True), "deep": deep}


# name -> (configuration, M_sdf, M_main, fbar present, {option: value} on top of the plan's defaults)
CASES = {
    "synthetic": ("synthetic", M_SDF, M_MAIN, 1, {}),
    "synthetic_light": ("synthetic_light", M_SDF, M_MAIN, 1, {}),
    "plumbing": ("plumbing", M_SDF, M_MAIN, 1, {}),
    "plumbing_skip_light": ("plumbing_skip_light", M_SDF, M_MAIN, 1, {}),
    "plumbing_skip_light_x3": ("plumbing_skip_light", M_SDF, M_MAIN, 1, {X3: 1}),
    "synthetic_fp32": ("synthetic", M_SDF, M_MAIN, 1, {X3: 0}),
    "synthetic_light_fp32": ("synthetic_light", M_SDF, M_MAIN, 1, {X3: 0}),
    "synthetic_x2": ("synthetic", M_SDF, M_MAIN, 1, {X2: 1}),
    "synthetic_pointmajor": ("synthetic", M_SDF, M_MAIN, 1, {BLOCKED: 0}),
    "synthetic_tail": ("synthetic", 256 * 128 + 5000, 256 * 128 + 3000, 1, {}),          # bulk + split-K tail: a blocked prefix
    "synthetic_no_main": ("synthetic", M_SDF, 0, 1, {}),
    "synthetic_no_fbar": ("synthetic", M_SDF, M_MAIN, 0, {}),
    "synthetic_light_no_main": ("synthetic_light", M_SDF, 0, 0, {}),
    "synthetic_parts": ("synthetic", M_SDF, M_MAIN, 1, {PARTS: 2}),
    "synthetic_light_parts": ("synthetic_light", M_SDF, M_MAIN, 1, {PARTS: 2}),
    "synthetic_parts_fp32": ("synthetic", M_SDF, M_MAIN, 1, {PARTS: 2, X3: 0}),
    "synthetic_parts_x2": ("synthetic", M_SDF, M_MAIN, 1, {PARTS: 2, X2: 1}),
    "synthetic_parts_x2_saves24": ("synthetic", M_SDF, M_MAIN, 1, {PARTS: 2, X2: 1, SAVES24: 1}),
    "synthetic_parts_saves24_only": ("synthetic", M_SDF, M_MAIN, 1, {PARTS: 2, SAVES24: 1}),       # without X2 the tensors stay fp32
    "synthetic_saves24_no_parts": ("synthetic", M_SDF, M_MAIN, 1, {X2: 1, SAVES24: 1}),
    "synthetic_parts_pointmajor": ("synthetic", M_SDF, M_MAIN, 1, {PARTS: 2, BLOCKED: 0}),
    "synthetic_parts_no_main": ("synthetic", M_SDF, 0, 0, {PARTS: 3}),
    "deep": ("deep", M_SDF, M_MAIN, 1, {}),
    "deep_parts": ("deep", M_SDF, M_MAIN, 1, {PARTS: 2}),                                  # 32 tasks > MAX_TASKS: two launches per range
}


def run_case(probe, name, tmp):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.params import ParamLayout
    conf, m_sdf, m_main, fbar, opts = CASES[name]
    desc = os.path.join(str(tmp), "net.desc")
    with open(desc, "wb") as f:
        f.write(bytes(ParamLayout(NetConfig.from_conf(_confs()[conf])).net_desc()))
    env = {k: v for k, v in os.environ.items() if not k.startswith("I2SDF_")}
    r = subprocess.run([probe, desc, str(m_sdf), str(m_main), str(fbar)] + [f"{k}={v}" for k, v in opts.items()], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-500:])
    return r.stdout


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("wgrad_probe") / "wgrad_probe")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-result",
           "-x", "hip", os.path.join(ROOT, "tests", "wgrad_probe.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("name", sorted(CASES))
def test_passes_tasks_and_reduction_table_match_the_recording(probe, tmp_path, name):
    got = run_case(probe, name, tmp_path).splitlines()
    want = open(os.path.join(GOLDEN, name + ".txt")).read().splitlines()
    head = lambda ls: [l for l in ls if l.startswith("pass ")]
    assert head(got) == head(want)                                      # which kernels, in which order, on which stream
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: {g} != recorded {w}"
    assert len(got) == len(want)


def test_recording_holds_the_launch_rules():
    """the recording itself against the rules worked out by hand"""
    rec = lambda name: open(os.path.join(GOLDEN, name + ".txt")).read().splitlines()
    passes = lambda name: [(l.split()[1], l.split()[7], int(l.split()[9])) for l in rec(name) if l.startswith("pass ")]
    tasks = lambda name: sum(l.startswith("task ") for l in rec(name))
    # without ranges: the narrow launch on the side stream, the 256 x 256 blocks on the caller's
    assert passes("synthetic") == [("wgrad_narrow_kernel<3>", "side", 1), ("wgrad3p_kernel<3>", "main", 1)]
    assert passes("synthetic_x2") == [("wgrad_narrow_kernel<3>", "side", 1), ("wgrad3p_kernel<2>", "main", 1)]
    assert passes("synthetic_fp32") == [("wgrad_narrow_kernel<0>", "side", 1), ("wgrad_kernel<0,0>", "main", 2)]
    # point ranges: one grid, the two-job blocks in front, the narrow tasks behind
    assert passes("synthetic_parts") == [("wgrad_all_kernel<3>", "main", 1)]
    assert passes("synthetic_parts_x2_saves24") == [("wgrad_all_kernel<2>", "main", 1)]
    order = [(int(l.split()[1]), int(l.split()[2])) for l in rec("synthetic_parts") if l.startswith("task ")]
    assert order == sorted(order, key=lambda vn: (vn[0] != 4, -vn[1] if vn[0] == 4 else 0)) and order[0] == (4, 2)
    # synthetic.yml: 7 + 1 blocks of the SDF net (hidden layers 1..7, the feature rows), 4 of the radiance net, 6 + 4 narrow tiles;
    # without split arithmetic every block is four 128 x 128 tiles: 48 tasks, two WgLaunch batches
    assert tasks("synthetic") == tasks("synthetic_parts") == 12 + 10 and tasks("synthetic_fp32") == 4 * 12 + 10
    # more tasks than one WgLaunch holds: the narrow launch, then the block launch, per range
    assert tasks("deep_parts") == 32 and passes("deep_parts") == [("wgrad_narrow_kernel<3>", "main", 1), ("wgrad3p_kernel<3>", "main", 1)]
    # packed 24-bit operands only with ranges, blocked saves and two planes
    p24 = lambda name: any(l.startswith("job ") and "1" in l.split()[-2:] for l in rec(name))
    assert p24("synthetic_parts_x2_saves24") and not p24("synthetic_parts_saves24_only") and not p24("synthetic_saves24_no_parts")
