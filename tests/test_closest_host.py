"""CPU: a host build of csrc/tri_closest.h (g++, the stand-alone program tests/closest_host.cpp) reproduces the numpy restatement of
the per-face rule bit for bit -- the closest point, d^2, the feature and the weights -- on the fixtures' queries, with coordinates
shifted by 1000 and with queries at distance 0; and its box bound never turns away a face's own exact box (the tightest box a tree
can hold around it) for that face's computed d^2."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import closest_ref as CR
import raycast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, D = np.float32, np.float64


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("closest_host") / "closest_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "closest_host.cpp"),
                    "-o", exe], check=True)

    def run(p, A, B, C):
        n = len(p)
        rec = np.concatenate([np.asarray(x, F32).reshape(n, 3) for x in (p, A, B, C)], 1)
        src, dst = exe + ".in", exe + ".out"
        with open(src, "wb") as fh:
            fh.write(np.int32(n).tobytes())
            fh.write(np.ascontiguousarray(rec, F32).tobytes())
        subprocess.run([exe, src, dst], check=True)
        return np.fromfile(dst, D).reshape(n, 11)
    return run


def _pairs():
    """(name, p, A, B, C): one face per point -- the face the law finds, and a random one"""
    g = np.random.default_rng(21)
    meshes = [("icosphere2", R.icosphere(2)), ("soup", R.soup(400, seed=2)), ("wedge", CR.wedge()), ("grid", R.flat_grid(8))]
    for name, (v, f) in meshes:
        for shift in (0.0, 1000.0):
            vs = (v.astype(D) + shift).astype(F32)
            q = CR.queries(vs, f, 300, seed=22)
            q = q[np.isfinite(q).all(1)]
            P = vs[f].astype(D)
            k = g.integers(0, len(f), 200)
            w = g.dirichlet([1, 1, 1], 200)
            on = np.concatenate([P[k, 0], (P[k, 0] + P[k, 1]) / 2, (P[k] * w[:, :, None]).sum(1)]).astype(F32)      # distance 0, or nearly
            law = CR.closest(vs, f, q)["face"]
            yield f"{name}+{shift:g}", q, vs[f[law]]
            yield f"{name}+{shift:g}/random", q, vs[f[g.integers(0, len(f), len(q))]]
            yield f"{name}+{shift:g}/on", on, vs[f[np.concatenate([k, k, k])]]


def test_host_build_reproduces_the_restatement_bit_for_bit(host):
    total, feats, zero = 0, set(), 0
    for name, p, T in _pairs():
        A, B, C = T[:, 0], T[:, 1], T[:, 2]
        got = host(p, A, B, C)
        c, d2, u, v, ft = CR.tri_closest(p.astype(D), A.astype(D), B.astype(D), C.astype(D))
        bits = lambda x: np.ascontiguousarray(x, D).view(np.int64)
        assert np.array_equal(got[:, 6].astype(int), ft), name
        assert np.array_equal(bits(got[:, :3]), bits(c)), name
        for col, want in ((3, d2), (4, u), (5, v)):
            assert np.array_equal(bits(got[:, col]), bits(want)), (name, col)
        assert not got[:, 7].any(), name
        # the box bound: restated, and it never turns the face's own box away for the face's own d2
        lo, hi = T.min(1), T.max(1)
        M = np.maximum(np.abs(p).max(1), np.maximum(np.abs(lo).max(1), np.abs(hi).max(1))).astype(D)
        assert np.array_equal(bits(got[:, 8]), bits(CR.box_dist2(p, lo, hi))), name
        assert np.array_equal(bits(got[:, 9]), bits(CR.box_skip_above(d2, M))), name
        assert not got[:, 10].any(), (name, "the box bound turned away a face for its own d2", int(got[:, 10].sum()))
        assert (got[:, 9] >= d2).all(), name                       # q equal to the best d2 is entered
        total += len(p)
        zero += int((d2 == 0).sum())
        feats |= set(ft.tolist())
    assert total > 10000 and feats == set(range(7)) and zero > 500, (total, feats, zero)


def test_degenerate_faces_and_nan_on_the_host(host):
    p = np.array([[0.3, 0.2, 0.1]] * 4, F32)
    A = np.array([[0, 0, 0], [0.25, 0.25, 0.25], [1, 2, 3], [0, 0, 0]], F32)
    B = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1, 2, 3], [1, 0, 0]], F32)
    C = np.array([[1, 0, 0], [1.0, 1.0, 1.0], [1, 2, 3], [0, 1, 0]], F32)
    got = host(p, A, B, C)
    assert got[:, 7].tolist() == [1, 1, 1, 0]
    # a NaN box distance or threshold never skips
    assert not (np.float64("nan") > CR.box_skip_above(1.0, 1.0)) and not (1.0 > CR.box_skip_above(np.float64("nan"), 1.0))
    assert CR.box_skip_above(np.inf, 1.0) == np.inf and CR.box_skip_above(0.0, 1000.0) == (1000.0 * 2.0 ** -32) ** 2
