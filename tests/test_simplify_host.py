"""CPU: a host build of csrc/quadric.h (g++, the stand-alone program tests/simplify_host.cpp) against the numpy restatement
tests/simplify_ref.py: the summed quadric A, bvec of every cell, the representative x and the fallback flag bit for bit (nothing but
+ - * / is called), on the fixtures of the GPU test and their copies shifted by +1000."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as R
import simplify_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, D = np.float32, np.float64


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("simplify_host") / "simplify_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "simplify_host.cpp"),
                    "-o", exe], check=True)

    def run(v, f, h, reg):
        res = S.simplify(v, f, h, "quadric", reg, detail=True)
        cell, cc, mean = res["cell"], res["centres"], res["mean"]
        M = len(cc)
        corner_cell = cell[f.astype(np.int64)].reshape(-1)
        order = np.argsort(corner_cell, kind="stable")
        start = np.searchsorted(corner_cell[order], np.arange(M + 1), "left")
        tri = v[f].reshape(len(f), 9)
        src, dst = exe + ".in", exe + ".out"
        with open(src, "wb") as fh:
            fh.write(np.int32(M).tobytes() + D(reg).tobytes() + D(h).tobytes())
            for m in range(M):
                rows = order[start[m]:start[m + 1]] // 3
                fh.write(np.int32(len(rows)).tobytes() + cc[m].tobytes() + (mean[m] - cc[m]).tobytes())
                fh.write(np.ascontiguousarray(tri[rows], F32).tobytes())
        subprocess.run([exe, src, dst], check=True)
        return np.fromfile(dst, D).reshape(M, 13), res
    return run


def _bits(x):
    return np.ascontiguousarray(x, D).view(np.int64)


@pytest.mark.parametrize("by", [0.0, 1000.0])
def test_host_build_reproduces_the_restatement(host, by):
    cells = fallbacks = long_runs = 0
    for name, (v, f), h in (("ico3", R.icosphere(3), 0.25), ("ico3 fine", R.icosphere(3), 0.1), ("one cell", R.icosphere(3), 3.0),
                            ("cube8", S.cube(8), 0.3), ("soup", R.soup(1000, seed=2), 0.2)):
        for reg in (1e-3, 1e-6):
            got, res = host(S.shift(v, by), f, h, reg)
            x = res["cell_verts"].astype(D)                       # (what the law rounds to fp32 is cc + x: compare x before that)
            q = res["quadrics"]
            assert np.array_equal(_bits(got[:, :9]), _bits(q)), (name, reg)
            want_x, want_fb = S.solve(q, reg, res["mean"] - res["centres"], D(0.5) * D(h))
            assert np.array_equal(got[:, 12] != 0, want_fb) and np.array_equal(want_fb, res["cell_fallback"]), (name, reg)
            assert np.array_equal(_bits(got[:, 9:12]), _bits(want_x)), (name, reg)
            assert np.array_equal((res["centres"] + want_x).astype(F32).view(np.int32), res["cell_verts"].view(np.int32))
            cells += len(q)
            fallbacks += int(want_fb.sum())
            long_runs += int((np.bincount(res["cell"][f.astype(np.int64)].reshape(-1)) > 64).sum())
            assert x.shape == (len(q), 3)
    print(f"shift {by:g}: {cells} cells, {fallbacks} fallbacks, {long_runs} runs longer than one round of 64 lanes")
    assert cells > 3000 and fallbacks > 0 and long_runs > 0
