"""GPU: marching cubes (csrc/mcubes.hip, i2sdf_amd.mesh.marching_cubes, I2SDFNetwork.extract_mesh) against the numpy restatement
(tests/mcubes_ref.py): faces exactly, vertices / normals to fp32 rounding, on the scikit-image fixtures and on odd shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcubes_ref as R

pytestmark = pytest.mark.gpu


def _check(vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    from i2sdf_amd.mesh import marching_cubes
    vol = np.ascontiguousarray(vol, np.float32)
    m = marching_cubes(torch.from_numpy(vol).cuda(), level, spacing, origin)
    v, f, n = R.marching_cubes(vol, level, spacing, origin)
    assert m.verts.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.normals.dtype == torch.float32
    assert m.faces.shape == f.shape and m.verts.shape == v.shape
    assert np.array_equal(m.faces.cpu().numpy(), f)
    sp = float(np.min(spacing))
    gv = m.verts.cpu().numpy()
    assert np.allclose(gv, v, rtol=1e-6, atol=1e-6 * sp, equal_nan=True)
    assert np.allclose(m.normals.cpu().numpy(), n, rtol=0, atol=1e-5, equal_nan=True)
    return m


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixtures(golden, tag):
    z = golden("g18_mcubes")
    _check(z[f"{tag}.vol"], float(z[f"{tag}.level"]), tuple(float(s) for s in z[f"{tag}.spacing"]), (0.5, -1.0, 0.25))


@pytest.mark.parametrize("shape", [(2, 7, 5), (9, 2, 13), (3, 3, 2), (17, 33, 65), (131, 97, 331)])
def test_random_padded_odd_shapes(shape):
    """(131, 97, 331) = 4.2 M points: more than one level of scan workgroups (4 096 blocks of 256 points > 1 024)."""
    g = np.random.default_rng(sum(shape))
    vol = g.standard_normal(shape).astype(np.float32)
    if min(shape) > 2:
        vol = np.pad(vol[1:-1, 1:-1, 1:-1], 1, constant_values=1.0)
    _check(vol, 0.0, (0.5, 0.25, 1.0))


def test_values_equal_to_the_level():
    vol = np.random.default_rng(7).integers(-2, 3, (21, 18, 23)).astype(np.float32)
    _check(vol, 0.0)
    _check(vol, 1.0)


def test_no_crossing_gives_an_empty_mesh():
    from i2sdf_amd import lib as L
    from i2sdf_amd.mesh import marching_cubes
    m = marching_cubes(torch.ones(5, 6, 7, device="cuda"))
    assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.normals.shape == (0, 3)
    lib = L.load()
    vol = torch.ones(5, 6, 7, device="cuda")
    ws = torch.empty(int(lib.i2sdf_marching_cubes_workspace_bytes(5, 6, 7)), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert lib.i2sdf_marching_cubes_count(L.ptr(vol), 5, 6, 7, 0.0, L.ptr(ws), L.ptr(counts), L.stream_ptr()) == 0
    assert counts.tolist() == [0, 0]


def test_argument_and_capacity_errors():
    from i2sdf_amd import lib as L
    lib = L.load()
    assert lib.i2sdf_marching_cubes_workspace_bytes(1, 5, 5) == 0
    vol = torch.randn(6, 5, 4, device="cuda")
    nb = int(lib.i2sdf_marching_cubes_workspace_bytes(6, 5, 4))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    st = L.stream_ptr()
    assert lib.i2sdf_marching_cubes_count(L.ptr(vol), 6, 5, 1, 0.0, L.ptr(ws), L.ptr(counts), st) == -1
    assert lib.i2sdf_marching_cubes_count(L.ptr(vol), 6, 5, 4, 0.0, L.ptr(ws), L.ptr(counts), st) == 0
    n_v, n_f = counts.tolist()
    assert n_v > 0 and n_f > 0
    sp = (C.c_float * 3)(1, 1, 1)
    verts = torch.empty(n_v, 3, device="cuda")
    normals = torch.empty(n_v, 3, device="cuda")
    faces = torch.empty(n_f, 3, dtype=torch.int32, device="cuda")
    emit = lambda cv, cf: lib.i2sdf_marching_cubes_emit(L.ptr(vol), 6, 5, 4, 0.0, sp, sp, L.ptr(ws), L.ptr(verts), L.ptr(normals),
                                                        L.ptr(faces), cv, cf, st)
    assert emit(n_v - 1, n_f) == -4 and emit(n_v, n_f - 1) == -4
    assert emit(n_v, n_f) == 0
    torch.cuda.synchronize()


def test_nan_values():
    vol = np.random.default_rng(3).standard_normal((12, 10, 11)).astype(np.float32)
    vol[np.random.default_rng(4).random(vol.shape) < 0.05] = np.nan
    _check(vol, 0.0, (0.1, 0.1, 0.1))


def test_runs_are_bitwise_identical():
    from i2sdf_amd.mesh import marching_cubes
    vol = torch.from_numpy(np.random.default_rng(5).standard_normal((64, 80, 96)).astype(np.float32)).cuda()
    a, b = marching_cubes(vol, 0.1, (0.1, 0.2, 0.3)), marching_cubes(vol, 0.1, (0.1, 0.2, 0.3))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _synthetic_net():
    from i2sdf_amd import I2SDFNetwork, synthetic_conf
    from oracle import i2sdf_oracle as orc
    ocfg = orc.synthetic_cfg()
    sd = orc.perturb_params(orc.init_params(ocfg, seed=5), 0.02, seed=6)
    net = I2SDFNetwork(synthetic_conf())
    net.load_state_dict(sd)
    return net.cuda().eval()


def test_extract_mesh_uniform_and_aligned():
    from i2sdf_amd import uniform_axes
    from i2sdf_amd.mesh import marching_cubes
    net = _synthetic_net()
    ax = uniform_axes(48, (-1.5, 1.5))
    m = net.extract_mesh(ax)
    want = marching_cubes(net.sdf_volume(ax), 0.0, ax.spacing, ax.origin)
    assert m.faces.shape[0] > 100
    for x, y in zip(m, want):
        assert torch.equal(x, y)
    # rotated / shifted grid: world vertices = rot @ (v + origin) + trans, and the SDF there is ~ the level
    g = torch.Generator().manual_seed(3)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    trans = torch.tensor([0.05, -0.1, 0.2])
    w = net.extract_mesh(ax, level=0.0, rot=q, trans=trans)
    grid = marching_cubes(net.sdf_volume(ax, rot=q, trans=trans), 0.0, ax.spacing, ax.origin)
    assert torch.equal(w.faces, grid.faces)
    torch.testing.assert_close(w.verts, grid.verts @ q.cuda().t() + trans.cuda(), rtol=0, atol=1e-5)
    sdf = net.sdf_grid(w.verts.contiguous())
    s = ax.spacing[0]
    assert float(sdf.abs().max()) <= 0.25 * s, float(sdf.abs().max())
