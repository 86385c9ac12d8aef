"""CPU: the numpy restatement of the winding-number law (tests/winding_ref.py) against closed forms, against itself under mutation,
and the approximation error of the hierarchical rule against the exact sum.

Tolerance of the closed forms.  The exact sum of F terms, each 2 atan2 good to a couple of ulp of a value <= 2 pi, summed in fp64:
|error of sum| <= F (4 + F) 2^-53 2 pi at the very worst; divided by 4 pi that is below F (4 + F) 2^-53.  The largest fixture here
has 640 faces: 4.6e-11.  The closed forms themselves (5/6, asin) are good to an ulp.

The measured maxima of |w - w_exact| (queries at least 0.05 of the diameter from the surface; Karras tree, box radii; printed by
test_error_of_the_hierarchical_rule) are recorded in include/i2sdf.h and the README.  No bar is set for them: the properties held are
round(w) == round(w_exact) at beta = 2 and max error at beta = 3 < max error at beta = 2.
    icosphere(3), 1280 faces   beta = 2: 5.11e-2    beta = 3: 2.15e-2
    open cap of it             beta = 2: 2.17e-2    beta = 3: 7.65e-3
    soup, 3000 faces           beta = 2: 3.11e-3    beta = 3: 1.04e-3"""
import numpy as np
import pytest

import raycast_ref as R
import winding_ref as W

F32, D = np.float32, np.float64
_CACHE = {}


def _tol(F):
    return max(F, 4) * (4 + F) * 2.0 ** -53


def _closed_forms():
    """(name, verts, faces, queries (fp64, before the shift), expected w)"""
    iv, ifc = R.icosphere(2)
    g = np.random.default_rng(3)
    u = g.normal(size=(40, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    inside = u * g.uniform(0.0, 0.9, (40, 1))
    outside = u * g.uniform(1.1, 4.0, (40, 1))
    q = np.concatenate([inside, outside])
    want = np.concatenate([np.ones(40), np.zeros(40)])
    yield "icosphere", iv, ifc, q, want
    yield "flipped", iv, W.flipped(ifc), q, -want
    yield "duplicated", iv, W.duplicated(ifc), q, 2 * want
    cv, cf = W.open_cube()
    yield "open_cube", cv, cf, np.zeros((1, 3)), np.array([5.0 / 6.0])
    a = 0.5
    sv, sf = W.square(a)
    h = np.array([0.25, 0.5, 1.0, 3.0, -0.25, -2.0])
    # the solid angle of a square of side 2a from height h above its centre is 4 asin(a^2 / (a^2 + h^2)); below it, the negative
    yield "square", sv, sf, np.stack([0 * h, 0 * h, h], 1), np.sign(h) * 4 * np.arcsin(a * a / (a * a + h * h)) / (4 * np.pi)


@pytest.mark.parametrize("by", [0.0, 1000.0])
def test_closed_forms_of_the_exact_sum(by):
    for name, v, f, q, want in _closed_forms():
        vs = W.shift(v, by)
        qs = (q + by).astype(F32)
        if name in ("icosphere", "flipped", "duplicated"):
            # (the rounded query must still be on its side of the rounded surface: 0.9 and 1.1 leave 0.1, fp32 at 1000 moves 6e-5)
            assert (np.abs(np.linalg.norm(qs.astype(D) - by, axis=1) - 1.0) > 0.05).all()
            got = W.exact(vs, f, qs)[0]
            assert np.abs(got - want).max() <= _tol(len(f)), (name, by, np.abs(got - want).max())
        else:
            assert np.array_equal(qs.astype(D), q + by), name           # the fixture's coordinates are exact in fp32, shifted too
            got = W.exact(vs, f, qs)[0]
            assert np.abs(got - want).max() <= _tol(len(f)), (name, by, got, want)
        # the tree route without a far field is the same sum in another order
        tree = W.tree_of(vs, f)
        table = W.moments(tree)[0]
        h = W.hierarchical(tree, table, qs, np.inf)
        assert (h["exact"] == len(f)).all() and (h["terms"] == len(f)).all(), name
        assert np.abs(h["w"] - want).max() <= _tol(len(f)), (name, by)


@pytest.mark.parametrize("mutate", ["dropped_factor_2", "den_sign"])
def test_a_mutated_term_fails_the_closed_forms(mutate):
    failed = []
    for name, v, f, q, want in _closed_forms():
        got = W.exact(v, f, q.astype(F32), mutate)[0]
        failed.append(np.abs(got - want).max() > 1e-3)
    assert all(failed), (mutate, failed)


def _patch():
    """a 100-odd-face spherical patch, lopsided about its box, moved off the origin"""
    v, f = R.icosphere(3)
    c = v[f].astype(D).mean(1)
    axis = np.array([0.48, 0.6, 0.64])
    keep = c @ axis > 0.8
    return W.shift(v, 0.0) + np.array([3.0, -2.0, 1.0], F32), np.ascontiguousarray(f[keep])


def _root_far_field_errors(mutate=None):
    """|far field of the ROOT record - exact| at 4, 8, 16 radii from the patch, orders 0 and 0 + 1 -> (3, 2) maxima"""
    v, f = _patch()
    tree = W.tree_of(v, f)
    table = W.moments(tree, mutate)[0]
    p, r = table[0, :3], table[0, 3]
    g = np.random.default_rng(5)
    u = g.normal(size=(60, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    out = np.zeros((3, 2))
    for k, radii in enumerate((4.0, 8.0, 16.0)):
        q = (p + radii * r * u).astype(F32)
        want = W.exact(v, f, q)[0]
        for order in (0, 1):
            ok, omega = W.far_field(q.astype(D), table[0], D(0.0), mutate, order)
            assert ok.all()
            out[k, order] = np.abs(omega / W.FOUR_PI - want).max()
    return out, len(f)


def _order1_helps(err):
    """order 1 lowers the error at every distance, and by a factor that grows with the distance (in theory as d: held to 1.5 per doubling)"""
    ratio = err[:, 1] / err[:, 0]
    return bool((ratio < 1.0).all() and (ratio[:-1] / ratio[1:] > 1.5).all())


def test_the_far_field_falls_as_the_law_says():
    err, F = _root_far_field_errors()
    print(f"patch of {F} faces, |far field - exact| at 4, 8, 16 radii: order 0 {err[:, 0]}, orders 0 + 1 {err[:, 1]}")
    assert 100 <= F <= 200
    # order 0 leaves the dipole's first correction, d^-3: a factor 8 per doubling; with order 1 the remainder falls as d^-4: 16.
    # (Held to 6 and 12: the next order is not yet negligible at 4 radii.)
    for k in (0, 1):
        assert err[k, 0] / err[k + 1, 0] > 6.0 and err[k, 1] / err[k + 1, 1] > 12.0, err
    assert _order1_helps(err), err


@pytest.mark.parametrize("mutate", ["no_recentre", "order1_sign"])
def test_a_mutated_far_field_fails_the_decay(mutate):
    good, _ = _root_far_field_errors()
    bad, _ = _root_far_field_errors(mutate)
    assert not _order1_helps(bad), (mutate, bad)
    assert (bad[:, 1] > good[:, 1]).all(), (mutate, bad, good)


def _error_cases():
    if "err" not in _CACHE:
        g = np.random.default_rng(11)
        cases = {}
        for name, (v, f) in (("icosphere(3), 1280 faces", R.icosphere(3)), ("open cap of it", W.cap(3)), ("soup, 3000 faces", R.soup(3000))):
            P = v[f].astype(D)
            lo, hi = P.min((0, 1)), P.max((0, 1))
            diam = float(np.linalg.norm(hi - lo))
            q = g.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (1500, 3)).astype(F32)
            q = q[W.surface_distance_at_least(v, f, q, 0.05 * diam)]
            if name.startswith("open"):
                # round() jumps where w crosses 1/2, and for a sheet that is the surface that closes it: here the flat disc across
                # the rim (sheet + disc is closed, the disc alone subtends 2 pi from a point on it).  The queries keep the same
                # 0.05 of the diameter from that surface as from the sheet itself.
                e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
                ue, cnt = np.unique(e, axis=0, return_counts=True)
                rim_z = v[ue[cnt == 1].ravel(), 2].astype(D)
                q = q[(q[:, 2] < rim_z.min() - 0.05 * diam) | (q[:, 2] > rim_z.max() + 0.05 * diam)]
            q = q[:500]
            tree = W.tree_of(v, f)
            cases[name] = (v, f, q, tree, W.moments(tree)[0], W.exact(v, f, q)[0])
        _CACHE["err"] = cases
    return _CACHE["err"]


def test_error_of_the_hierarchical_rule():
    worst = {}
    for name, (v, f, q, tree, table, want) in _error_cases().items():
        assert len(q) >= 200, (name, len(q))
        errs = {}
        for beta in (2.0, 3.0):
            h = W.hierarchical(tree, table, q, beta)
            errs[beta] = float(np.abs(h["w"] - want).max())
            frac = float(h["terms"].mean()) / len(f)
            print(f"{name}: beta = {beta:g}: max |w - w_exact| = {errs[beta]:.2e} over {len(q)} queries; {h['terms'].mean():.0f} terms per query "
                  f"({100 * frac:.1f} % of the faces), {h['exact'].mean():.0f} of them faces")
            if beta == 2.0:
                assert np.array_equal(np.round(h["w"]), np.round(want)), name
                assert h["terms"].mean() < 0.5 * len(f), name                   # the far field is taken at all
        assert errs[3.0] < errs[2.0], (name, errs)
        worst[name] = errs
    inside = sum(int((np.round(c[5]) != 0).sum()) for c in _error_cases().values())
    assert inside > 50                                                         # both sides of a surface are queried


def test_moments_that_are_not_recentred_fail_the_hierarchical_check(mutate="no_recentre"):
    """(the opposite sign of the order-1 term is caught by the decay above, not here: on meshes this small the order-1 term does
    not lower the MAXIMUM error at beta = 2, so its sign does not show in it)"""
    v, f, q, tree, table, want = _error_cases()["icosphere(3), 1280 faces"]
    good = np.abs(W.hierarchical(tree, table, q, 2.0)["w"] - want).max()
    bad = np.abs(W.hierarchical(tree, W.moments(tree, mutate)[0], q, 2.0, mutate)["w"] - want).max()
    assert bad > 2 * good, (mutate, bad, good)


def test_moments_compose_and_radii_are_conservative():
    for by in (0.0, 1000.0):
        v, f = R.icosphere(2)
        v = W.shift(v, by)
        f = W.shuffled(f, 1)
        tree = W.tree_of(v, f)
        table, raw, mag = W.moments(tree)
        P = v[f].astype(D)
        nrm = 0.5 * np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        area = np.linalg.norm(nrm, axis=1)
        cen = P.mean(1)
        # the root against direct sums
        assert abs(raw[0, 0] - area.sum()) <= 1e-13 * area.sum()
        assert np.abs(table[0, :3] - (area[:, None] * cen).sum(0) / area.sum()).max() <= 1e-12 * max(1.0, by)
        assert np.abs(table[0, 4:7]).max() <= 1e-13                               # a closed mesh: the area vectors cancel
        N1 = ((cen - table[0, :3])[:, :, None] * nrm[:, None, :]).sum(0)
        assert np.abs(table[0, 7:].reshape(3, 3) - N1).max() <= 1e-12, by          # the shift does not cancel it
        vol = np.linalg.det(P - by).sum() / 6.0
        assert abs(np.trace(N1) - 3 * vol) <= 1e-9 and 3.9 < vol < 4 * np.pi / 3    # trace = 3 x volume of the inscribed polyhedron
        # every node: all vertices below lie within r of the centroid

        def verts_below(c):
            if c < 0:
                return tree["leaf_v"][~c].astype(D)
            return np.concatenate([verts_below(tree["child"][c, 0]), verts_below(tree["child"][c, 1])])
        for i in range(len(table)):
            d = np.linalg.norm(verts_below(i) - table[i, :3], axis=1).max()
            assert d <= table[i, 3], (i, d, table[i, 3])


def test_rejected_faces_bad_points_small_meshes_and_the_surface():
    iv, ifc = R.icosphere(2)
    v, f = W.with_bad_faces(iv, ifc)
    g = np.random.default_rng(4)
    q = g.uniform(-1.5, 1.5, (60, 3)).astype(F32)
    q[5, 1], q[9, 0], q[11] = np.nan, np.inf, 1e6
    w, _, status = W.exact(v, f, q)
    w0, _, status0 = W.exact(iv, ifc, q)
    assert status == (W.BAD_POINT | W.BAD_FACE) and status0 == W.BAD_POINT
    assert np.isnan(w[[5, 9]]).all() and np.isfinite(np.delete(w, [5, 9])).all()
    assert np.array_equal(np.nan_to_num(w, nan=7.0), np.nan_to_num(w0, nan=7.0))       # the rejected faces add nothing, in order
    assert abs(w[11]) < 1e-9
    tree = W.tree_of(v, f)
    table = W.moments(tree)[0]
    for beta in (2.0, np.inf):
        h = W.hierarchical(tree, table, q, beta)
        assert np.isnan(h["w"][[5, 9]]).all() and np.abs(np.delete(h["w"] - w, [5, 9])).max() < (0.1 if beta == 2.0 else 1e-12)
    # F = 0, 1, 2 through both restatements
    sv, sf = R.soup(4)
    for F in (0, 1, 2):
        tree = W.tree_of(sv, sf[:F])
        table = W.moments(tree)[0]
        assert table.shape == (max(F - 1, 0), 16)
        a, b = W.exact(sv, sf[:F], q[:20])[0], W.hierarchical(tree, table, q[:20], np.inf)["w"]
        assert np.allclose(a, b, rtol=0, atol=1e-15, equal_nan=True) and (F > 0 or (a[np.isfinite(a)] == 0).all())
    # nothing but degenerate faces: no area, radius +inf, always descended
    dv = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], F32)
    df = np.array([[0, 1, 2], [1, 2, 3], [0, 0, 3]], np.int32)
    tree = W.tree_of(dv, df)
    table = W.moments(tree)[0]
    assert np.isinf(table[:, 3]).all()
    assert (W.hierarchical(tree, table, q[:4], 2.0)["exact"] == 3).all()
    # on the surface: finite, and a face's interior sees half the sphere
    s = W.on_surface(iv, ifc)
    ws = W.exact(iv, ifc, s)[0]
    assert np.isfinite(ws).all() and (np.abs(ws) < 1.5).all()
    assert W.solid_angle(np.zeros((1, 3)), [0, 0, 0], [1, 0, 0], [0, 1, 0])[0] == 0.0           # atan2(0, 0) at a vertex
    assert abs(W.solid_angle(np.array([[0.25, 0.25, 0.0]]), [0, 0, 0], [1, 0, 0], [0, 1, 0])[0]) == 2 * np.pi
