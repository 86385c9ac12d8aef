"""CPU: the plan is the only description of the packed weight streams, and it describes what it described before.

Every MLP launch takes (stream start, stage count) from two marks of the plan (plan.h: span()).  A stage count that is off by one is not
a failing assertion on the device: the stream's DMA look-ahead runs past, or stops short of, the ops the kernel's static structure
consumes.  So the numbers are pinned here, on the CPU, against a recording that does not come from the code under test.

tests/plan_probe.cpp is compiled together with csrc/plan.cpp (host code only, a few seconds, no GPU: a plan without a device keeps its
host-side table) and prints, for a descriptor `ParamLayout.net_desc()` produced, the segment table -- every Seg field of every segment --
and the span of every launch site.

tests/golden/plan_layout/<configuration>.txt were recorded at commit 8fe6da1, the last one with the hand-mirrored stage formulas, by a
throwaway program with the same output format: the segment table of that commit's plan, and per launch site the `*_chunk0` /
`*_wsdf_chunk` field the entry point read together with the value of the formula it called (`sdf_fwd_stages`, `sdf_fwd_hidden_stages`,
`sdf_rev_stages`, `sdf_rev_bwd_stages`, `sdf_fwd3_stages`, `sdf_fwd3_hidden_stages`, `sdf_rev3_stages`, `sdf_rev3_bwd_stages`,
`sdf_fwd3h_stages` with 3 and 2 planes, `sdf_fwd3h_train_stages`, `rgb_fwd_stages`, `rgb_rev_stages`, `rgb_fwd3h_stages`,
`rgb_rev3h_stages`, the two sums of the light head), evaluated for that configuration's widths; "refused" where that commit's plan had no
such stream (`*_chunks == 0`: the 16-point-wave streams of the 64-wide nets)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i2sdf_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_layout")


def _confs():
    from i2sdf_amd.config import synthetic_conf, plumbing_conf
    return {"synthetic": synthetic_conf(), "synthetic_light": synthetic_conf(True), "plumbing": plumbing_conf(),
            "plumbing_skip_light": plumbing_conf(True, True)}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("plan_probe") / "plan_probe")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-result",
           "-x", "hip", os.path.join(ROOT, "tests", "plan_probe.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(probe, conf, tmp_path):
    from i2sdf_amd.config import NetConfig
    from i2sdf_amd.params import ParamLayout
    desc = os.path.join(str(tmp_path), "net.desc")
    with open(desc, "wb") as f:
        f.write(bytes(ParamLayout(NetConfig.from_conf(conf)).net_desc()))
    r = subprocess.run([probe, desc], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    lines = r.stdout.splitlines()
    return [l for l in lines if not l.startswith("check ")], dict(l.split()[1:] for l in lines if l.startswith("check "))


@pytest.mark.parametrize("name", ["synthetic", "synthetic_light", "plumbing", "plumbing_skip_light"])
def test_segment_table_and_launch_spans_match_the_recording(probe, tmp_path, name):
    got, _ = _run(probe, _confs()[name], tmp_path)
    want = open(os.path.join(GOLDEN, name + ".txt")).read().splitlines()
    seg = lambda ls: [l for l in ls if not l.startswith("span ")]
    spans = lambda ls: {l.split()[1]: tuple(l.split()[2:]) for l in ls if l.startswith("span ")}
    assert seg(got)[0] == seg(want)[0]                                      # segments, total chunks, scale region
    for i, (g, w) in enumerate(zip(seg(got)[1:], seg(want)[1:])):
        assert g == w, f"segment {i}: {g} != recorded {w}"
    assert len(seg(got)) == len(seg(want))
    assert len(spans(want)) >= 16
    assert spans(got) == spans(want)                                        # (start chunk, stages) of every launch site, or ('refused',)


def test_recording_holds_the_numbers_of_the_two_shipped_shapes():
    """the recording itself against the stage counts worked out by hand for the two 256-wide shapes (L = 9 skip 4; L = 7 skip 3)"""
    rec = lambda name: {l.split()[1]: l.split()[2:] for l in open(os.path.join(GOLDEN, name + ".txt")) if l.startswith("span ")}
    a, b = rec("synthetic"), rec("synthetic_light")
    for key, na, nb in (("sdf.fwd_all", 79, 61), ("sdf.rev_chain", 62, 46), ("sdf.rev3_chain", 92, 68), ("sdf.rev3_sweep2", 103, 79),
                        ("sdf.fwd3_all", 100, 74), ("sdf.fwd3h_all", 112, 86), ("sdf.fwd2h", 69, 51)):
        assert (int(a[key][1]), int(b[key][1])) == (na, nb), key
    assert (int(a["rgb.fwd3h"][1]), int(a["rgb.rev3h"][1])) == (55, 50)
    assert open(os.path.join(GOLDEN, "synthetic.txt")).readline().split()[:4] == ["segs", "136", "total_chunks", "23072"]


def test_span_refuses_empty_and_ragged_spans(probe, tmp_path):
    _, chk = _run(probe, _confs()["synthetic"], tmp_path)
    assert chk["empty"] == "0" and chk["backwards"] == "0"                  # nothing between the marks: refused
    assert chk["ragged"] == "0"                                             # not a whole number of stages: refused
    assert chk["whole"] == "1"                                              # the same marks with a stage size that divides: accepted
