"""CPU: a host build of csrc/tri_solid_angle.h (g++, the stand-alone program tests/winding_host.cpp) against the numpy restatement
tests/winding_ref.py: both arguments of atan2 bit for bit, the face moments, the finished record and the far-field rule bit for bit
(none of them calls anything but + - * / sqrt), and the solid angle itself within the bound of atan2.

The bound of atan2.  The GNU C library documents its atan2 as good to 1 ulp in binary64 (manual, "Known Maximum Errors in Math
Functions"); numpy's arctan2 is that function or a vector routine held to the same 1 ulp.  Two results of the same arguments, each
within 1 ulp of the true value, differ by at most 2 ulp; the factor 2 of the solid angle is exact.  So: 2 ulp of the result."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as R
import winding_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, D = np.float32, np.float64
ATAN2_ULP = 2.0
O = np.array([0.125, -0.25, 0.5])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("winding_host") / "winding_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "winding_host.cpp"),
                    "-o", exe], check=True)

    def run(q, A, B, C, o=O):
        n = len(q)
        rec = np.concatenate([np.asarray(x, F32).reshape(n, 3) for x in (q, A, B, C)], 1)
        src, dst = exe + ".in", exe + ".out"
        with open(src, "wb") as fh:
            fh.write(np.int32(n).tobytes())
            fh.write(np.asarray(o, D).tobytes())
            fh.write(np.ascontiguousarray(rec, F32).tobytes())
        subprocess.run([exe, src, dst], check=True)
        return np.fromfile(dst, D).reshape(n, 37)
    return run


def _pairs():
    """(name, q, T (n, 3, 3)): random queries against random faces, and queries on vertices, edges and faces"""
    g = np.random.default_rng(61)
    for name, (v, f) in (("icosphere2", R.icosphere(2)), ("soup", R.soup(400, seed=2)), ("grid", R.flat_grid(8)), ("cube", W.open_cube())):
        for by in (0.0, 1000.0):
            vs = W.shift(v, by)
            P = vs[f]
            k = g.integers(0, len(f), 600)
            q = (g.uniform(-2, 2, (600, 3)) + by).astype(F32)
            q[:100] = (P[k[:100]].astype(D).mean(1) + g.normal(0, 1e-3, (100, 3))).astype(F32)      # close to the face
            yield f"{name}+{by:g}", q, P[k]
            w = g.dirichlet([1, 1, 1], 200)
            Pd = P[k[:200]].astype(D)
            on = np.concatenate([Pd[:, 0], (Pd[:, 0] + Pd[:, 1]) / 2, (Pd * w[:, :, None]).sum(1)]).astype(F32)
            yield f"{name}+{by:g}/on", on, P[np.concatenate([k[:200]] * 3)]


def _bits(x):
    return np.ascontiguousarray(x, D).view(np.int64)


def test_host_build_reproduces_the_restatement(host):
    total, zero, far, worst = 0, 0, 0, 0.0
    for name, q, T in _pairs():
        A, B, C = T[:, 0], T[:, 1], T[:, 2]
        got = host(q, A, B, C)
        det, den = W.solid_angle_terms(q, A, B, C)
        assert np.array_equal(_bits(got[:, 0]), _bits(det)), name
        assert np.array_equal(_bits(got[:, 1]), _bits(den)), name
        want = W.solid_angle(q, A, B, C)
        assert np.isfinite(got[:, 2]).all(), name
        err = np.abs(got[:, 2] - want) / np.spacing(np.abs(want))
        worst = max(worst, float(err.max()))
        assert (err <= ATAN2_ULP).all(), (name, float(err.max()))
        # the moments, the record and the far field: no library function but sqrt, so bit for bit
        for i in range(0, len(q), 7):
            m = W.face_moments(T[i], O)
            assert np.array_equal(_bits(got[i, 3:19]), _bits(m)), (name, i)
            t = W.finish(m, O, T[i].min(0), T[i].max(0))
            assert np.array_equal(_bits(got[i, 19:35]), _bits(t)), (name, i)
            ok, omega = W.far_field(q[i:i + 1].astype(D), t, D(4.0))
            assert bool(ok[0]) == bool(got[i, 35]), (name, i)
            if ok[0]:
                assert _bits(omega)[0] == _bits(got[i, 36:37])[0], (name, i)
                far += 1
        total += len(q)
        zero += int((got[:, 0] == 0).sum())
    print(f"{total} pairs, {zero} with det = 0, {far} far fields compared; largest difference of the solid angle: {worst:.2f} ulp")
    assert total > 8000 and zero > 500 and far > 300, (total, zero, far)


def test_the_surface_and_degenerate_faces_on_the_host(host):
    q = np.array([[0, 0, 0], [0.25, 0.25, 0], [0.5, 0, 0], [0.25, 0.25, 1], [0.25, 0.25, -1], [0.5, 0.5, 0.5]], F32)
    A = np.array([[0, 0, 0]] * 5 + [[0, 0, 0]], F32)
    B = np.array([[1, 0, 0]] * 5 + [[1, 1, 1]], F32)
    C = np.array([[0, 1, 0]] * 5 + [[2, 2, 2]], F32)
    got = host(q, A, B, C)
    assert got[0, 2] == 0.0                                    # on a vertex: atan2(0, 0)
    assert abs(got[1, 2]) == 2 * np.pi                         # inside the face: atan2(+-0, < 0)
    assert got[2, 1] == 0.0 and got[2, 2] == 0.0               # inside an edge a and b are antiparallel and den cancels: atan2(0, 0)
    assert got[3, 2] < 0 < got[4, 2] and got[3, 2] == -got[4, 2]                # the normal (+z) points towards q, away from q
    assert abs(got[5, 2]) == 2 * np.pi and got[5, 3] == 0.0 and np.isinf(got[5, 22])      # on a degenerate face; no area: r = +inf
    assert got[5, 35] == 0.0                                   # and never accepted
