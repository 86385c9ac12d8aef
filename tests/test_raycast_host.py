"""CPU: a host build of csrc/tri_isect.h (g++, the stand-alone program tests/raycast_host.cpp) reproduces the fp32 restatement of the
per-face rule bit for bit -- t, barycentrics and the accept / reject decision -- on the fixtures' rays, on rays with zero direction
components and on rays exactly in an edge's plane; and its box test never turns away a face the rule accepts (the face's own exact box,
the tightest box a tree can hold around it)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("raycast_host") / "raycast_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "raycast_host.cpp"),
                    "-o", exe], check=True)

    def run(o, d, A, B, C, t_min, t_max, cull):
        n = len(o)
        rec = np.concatenate([np.asarray(x, F32).reshape(n, -1) for x in (o, d, A, B, C, np.broadcast_to(F32(t_min), (n,)),
                                                                          np.broadcast_to(F32(t_max), (n,)), np.full(n, float(cull == "back")))], 1)
        assert rec.shape == (n, 18)
        src, dst = exe + ".in", exe + ".out"
        with open(src, "wb") as fh:
            fh.write(np.int32(n).tobytes())
            fh.write(np.ascontiguousarray(rec, F32).tobytes())
        subprocess.run([exe, src, dst], check=True)
        raw = np.fromfile(dst, np.int32).reshape(n, 6)
        return raw[:, 0].astype(bool), raw[:, 1].astype(bool), raw[:, 2].astype(bool), raw[:, 3:].view(F32)
    return run


def _pairs():
    """(name, o, d, A, B, C): one face per ray"""
    g = np.random.default_rng(11)
    for name, v, f, o, d in _cases():
        # every ray against the face the law finds, and against a random one
        hitf = R.trace(v, f, o, d, dt=F32)["face"]
        for faces in (np.where(hitf >= 0, hitf, 0), g.integers(0, len(f), len(o))):
            P = v[f[faces]]
            yield name, o, d, P[:, 0], P[:, 1], P[:, 2]


def _cases():
    from test_raycast_ref import _watertight_cases
    yield from _watertight_cases()
    g = np.random.default_rng(12)
    v, f = R.soup(400, seed=2)
    o = g.uniform(-1.5, 1.5, (1500, 3))
    d = g.normal(size=(1500, 3))
    d[::3, g.integers(0, 3)] = 0.0                              # zero direction components, one and two of them
    d[::6, 0] = 0.0
    d[::7] = np.eye(3)[g.integers(0, 3, len(d[::7]))] * g.choice([-2.0, 0.5], (len(d[::7]), 1))
    yield "soup", v, f, o, d
    # rays exactly in an edge's plane: from a point of the plane z = x (which holds the diagonal edges of a tilted grid) to edge points
    gv, gf = R.flat_grid(8)
    gv = gv.copy()
    gv[:, 2] = gv[:, 0]                                         # exact
    tg = R.watertight_targets(gv, gf, interior_only=True)
    o = np.tile([[0.25, -3.0, 0.25]], (len(tg), 1))
    yield "edge_plane", gv, gf, o, tg - o


@pytest.mark.parametrize("cull", ["none", "back"])
def test_host_build_reproduces_the_restatement_bit_for_bit(host, cull):
    total = accepted = 0
    for name, o, d, A, B, C in _pairs():
        o32, d32 = o.astype(F32), d.astype(F32)
        ray_ok, acc, box, res = host(o32, d32, A, B, C, 0.0, np.inf, cull)
        Rr = R.ray_shear(o32, d32, F32)
        ok, t, u, v, _ = R.tri_hit(Rr, A, B, C, F32(0), F32(np.inf), cull, F32)
        ok &= Rr["ok"]
        assert np.array_equal(ray_ok, Rr["ok"]), name
        assert np.array_equal(acc, ok), (name, int((acc != ok).sum()))
        for got, want in zip(res.T, (t, u, v)):
            assert np.array_equal(got[ok].view(np.int32), want[ok].astype(F32).view(np.int32)), name
        assert box[ok].all(), (name, "the box test turned away a face the rule accepts")
        total += len(o)
        accepted += int(ok.sum())
    # (seen from inside the sphere and from below the sheet nearly every face is a back face: culling leaves the soup's front faces)
    assert total > 10000 and accepted > (3000 if cull == "none" else 50), (total, accepted)


def test_bounds_and_bad_rays_on_the_host(host):
    o = np.array([[0.1, 0.3, -1.0]] * 6, F32)
    d = np.array([[0, 0, 1.0]] * 6, F32)
    d[4], d[5] = (0, 0, 0), (np.nan, 0, 1)
    A, B, C = (np.tile(np.array([x], F32), (6, 1)) for x in ((-1, -1, 0.5), (1, -1, 0.5), (0, 1, 0.5)))
    for t_min, t_max, want in ((0.0, np.inf, True), (1.5, np.inf, False), (0.0, 1.5, True), (0.0, 1.4999, False), (np.nan, np.inf, False)):
        ray_ok, acc, box, res = host(o, d, A, B, C, t_min, t_max, "none")
        assert ray_ok.tolist() == [True] * 4 + [False] * 2
        assert acc[:4].tolist() == [want] * 4 and not acc[4:].any()
        if want:
            assert (res[:4, 0] == F32(1.5)).all() and box[:4].all()
