"""CPU: the numpy form of the density-clustering law (tests/dbscan_ref.py, include/i2sdf.h "Density clustering") against
sklearn.cluster.DBSCAN -- labels_ and core_sample_indices_ exactly -- on the fixtures the GPU tests use; and three mutations of the
law, each of which the library tells from it on at least one fixture.

The library rounds its distances its own way.  So for every fixture whose coordinates are not exact, the smallest |d2 - eps^2| / eps^2
over all pairs is asserted to be at least 1e-7: no rounding of a double-precision distance can decide a pair there.  The lattices have
exact coordinates and exact squared distances (multiples of 1/16 below 2^4) in any precision."""
import numpy as np
import pytest

import dbscan_ref as R

sklearn_cluster = pytest.importorskip("sklearn.cluster")


def _library(P, eps, min_samples):
    fit = sklearn_cluster.DBSCAN(eps=eps, min_samples=min_samples).fit(P)
    core = np.zeros(P.shape[0], dtype=bool)
    core[fit.core_sample_indices_] = True
    return fit.labels_.astype(np.int64), core


def _fixtures():
    """name -> (points, eps, min_samples, coordinates exact)"""
    out = {name: R.cloud(name) + (False,) for name in R.CLOUDS}
    for order in R.ORDERS:
        out[f"contested_{order}"] = R.contested(order) + (False,)
        out[f"contested_exact_{order}"] = R.contested(order, exact=True) + (True,)
    for eps, min_samples in R.LATTICES:
        out[f"lattice_{eps}_{min_samples}"] = (R.lattice(), eps, min_samples, True)
    return out


FIXTURES = _fixtures()


@pytest.fixture(scope="module")
def library():
    return {name: _library(P, eps, ms) for name, (P, eps, ms, _) in FIXTURES.items()}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_law_equals_the_library(library, name):
    P, eps, min_samples, exact = FIXTURES[name]
    labels, core, k = R.dbscan(P, eps, min_samples)
    want_labels, want_core = library[name]
    _, margin = R.neighbour_matrix(P, eps)
    border = int(((labels >= 0) & ~core).sum())
    print(f"{name}: n = {P.shape[0]}, {k} clusters, {int(core.sum())} core, {border} border, {int((labels < 0).sum())} noise, "
          f"min |d2 - eps^2| / eps^2 = {margin:.2e}")
    if not exact:
        assert margin >= 1e-7, margin                                      # the library's own rounding cannot decide a pair
    else:
        assert margin == 0.0                                               # pairs at exactly eps: the inclusive bound is on trial
    assert np.array_equal(core, want_core)
    assert np.array_equal(labels, want_labels)
    assert k == (int(want_labels.max()) + 1 if (want_labels >= 0).any() else 0)


def test_the_fixtures_cover_what_they_are_for():
    sizes, clusters, borders = [], [], []
    for name in R.CLOUDS:
        P, eps, ms = R.cloud(name)
        labels, core, k = R.dbscan(P, eps, ms)
        sizes.append(P.shape[0]); clusters.append(k); borders.append(int(((labels >= 0) & ~core).sum()))
    assert min(sizes) >= 900 and max(sizes) <= 2000, sizes
    assert min(clusters) >= 4 and max(clusters) >= 100, clusters
    assert min(borders[:3] + borders[4:]) >= 20, borders                   # (min_samples = 1 has no border points: every point is core)
    for order in R.ORDERS:
        for exact in (False, True):
            P, eps, ms = R.contested(order, exact)
            A, _ = R.neighbour_matrix(P, eps)
            labels, core, k = R.dbscan(P, eps, ms)
            mid = int(np.flatnonzero(~core)[0])
            assert k == 2 and (~core).sum() == 1 and labels[mid] == 0
            assert sorted(set(labels[A[mid] & core])) == [0, 1]            # contested: a core neighbour in each cluster


@pytest.mark.parametrize("mutation", [dict(strict=True), dict(border="max"), dict(numbering="member")], ids=lambda m: next(iter(m)))
def test_the_library_tells_each_mutation_from_the_law(library, mutation):
    failed = []
    for name, (P, eps, min_samples, _) in FIXTURES.items():
        labels, core, _ = R.dbscan(P, eps, min_samples, **mutation)
        want_labels, want_core = library[name]
        if not (np.array_equal(labels, want_labels) and np.array_equal(core, want_core)):
            failed.append(name)
    print(f"{mutation}: differs from the library on {failed}")
    assert failed, mutation
