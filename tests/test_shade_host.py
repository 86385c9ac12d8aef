"""CPU: csrc/brdf_dev.h compiled for the host (tests/shade_probe.cpp, the tests/plan_probe.cpp precedent) and fed the inputs of the goldens
tests/golden/g23_shade_*.npz: per sample wo, pdf, f_spec and d / d rough of the seven against the reference's fp64 functions
(`sub.rows.f64`, every fourth point of a fixture).

In fp64 the header must BE the reference's function: 1e-9, max-norm relative per column, derivative columns included -- this is what pins the
tangent the backward kernel carries.  In fp32 -- the arithmetic of the kernels but for the hardware sine -- wo and the estimator's weight
f_spec max(wo_z, 0) / pdf are held to the project's forward bar 2e-5, and d wo / d rough to the bars of tests/test_gpu_shade.py: 1e-4 on the
well-posed fixture, max(1e-4, 2 x the fixture's recorded fp32-reference deviation of grough) on the wide one.  pdf and f_spec ALONE are
printed, not bounded, in fp32: both carry D = A / (pi b^2) with b = 1 - (1 - A) H_z^2, a difference of numbers near 1 that is as small as
A = alpha^4 (1.6e-3 at rough 0.2, 1e-5 at the clamp), so fp32 leaves D a relative error of 2 eps / b, 1e-4 and more, in any operation
order, the reference's included; D cancels in f_spec / pdf wherever the specular lobe carries the pdf, which is why the weight is well
conditioned and is what the kernels' outputs are made of."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i2sdf_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("shade_probe") / "shade_probe")
    cmd = [cxx, "-O1", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "shade_probe.cpp"), "-o", exe]
    if cxx.endswith("hipcc"):
        cmd[1:1] = ["--offload-arch=gfx950", "-x", "hip"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _rows(probe, g, tmp_path, precision):
    sub = g["sub_points"]
    raw = os.path.join(str(tmp_path), "in.raw")
    with open(raw, "wb") as f:
        for k in ("normal", "view_direction", "Kd", "Ks", "rough", "samples"):
            f.write(np.ascontiguousarray(g[k][sub], dtype=np.float32).tobytes())
    spp = g["samples"].shape[1]
    r = subprocess.run([probe, raw, str(len(sub)), str(spp), precision], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]
    return np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()]).reshape(len(sub), spp, 14)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


GROUPS = {"wo": slice(0, 3), "pdf": slice(3, 4), "f_spec": slice(4, 7), "d wo": slice(7, 10), "d pdf": slice(10, 11), "d f_spec": slice(11, 14)}


@pytest.mark.parametrize("name", ["well", "wide"])
def test_host_instantiation_against_the_reference(probe, tmp_path, name):
    g = np.load(os.path.join(GOLDEN, f"g23_shade_{name}.npz"))
    want = g["sub.rows.f64"]
    above = g["wi_mask"][g["sub_points"]]                      # rows with the view behind the surface: finite, nothing more
    got64, got32 = _rows(probe, g, tmp_path, "f64"), _rows(probe, g, tmp_path, "f32")
    assert np.isfinite(got64).all() and np.isfinite(got32).all()
    assert ((~above).sum() == 0) == (name == "well")             # the wide subset keeps a row with the view behind the surface
    d_bar = 1e-4 if name == "well" else max(1e-4, 2 * float(g["dev.grough"]))
    for what, cols in GROUPS.items():
        e64, e32 = _rel(got64[above][..., cols], want[above][..., cols]), _rel(got32[above][..., cols], want[above][..., cols])
        print(f"{name} {what}: fp64 {e64:.2e}, fp32 {e32:.2e}")
        assert e64 <= 1e-9, (what, e64)
        if what in ("wo", "d wo"):
            assert e32 <= (d_bar if what == "d wo" else 2e-5), (what, e32)
    weight = lambda r: r[..., 4:7] * np.maximum(r[..., 2:3], 0) / r[..., 3:4]
    e32 = _rel(weight(got32[above]), weight(want[above]))
    print(f"{name} f_spec max(wo_z, 0) / pdf: fp32 {e32:.2e}")
    assert e32 <= 2e-5, e32
