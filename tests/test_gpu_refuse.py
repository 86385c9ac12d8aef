"""GPU: the visibility culling on the device (csrc/raster.hip, csrc/tsdf.hip; i2sdf_amd.mesh.mesh_depth / tsdf_integrate /
tsdf_extract / refuse / score) against the numpy restatement (tests/refuse_ref.py, itself checked against closed-form geometry in
tests/test_refuse_ref.py) and against closed-form geometry that does not depend on it.  Neither open3d nor pyrender is available.

Bars.
  depth     Coverage is an integer decision (fp64 edge functions of fp32 camera-space vertices, the same operations in the same order
            on both sides): masks must be equal, except at samples within 1e-6 px of a triangle's edge (at most 0.1 % of the covered
            samples, asserted).  The depth is one fp64 division rounded to fp32 on both sides: 1 fp32 ulp allowed, 0 expected; what is
            seen is printed.
  fusion    Six cameras whose views overlap on the walls (refuse_ref.overlapping_cameras): a fifth of the updated voxels get a
            fractional t from three or more cameras, so the running average is exercised (asserted).  Touched units and weights are
            integers: equal.  tsdf: the restatement takes the kernel's fp32 coordinates, pixel and sdf and then computes t and the
            running average in fp64; the kernel's fp32 chain rounds one division (t) and one average (a product, a sum, a division)
            per camera, 4 roundings for each of up to 6 cameras; the bar is 4 fp32 ulp of the fp64 value rounded to fp32 (the ulp
            of that value itself).  The kernel follows the fp32 restatement operation by operation with contraction off, so it is
            also asked to equal it bit for bit, which a different order of cameras or of operations would not.  Voxels that are
            borderline in fp64 (projection within 1e-4 px of a pixel boundary, sdf within 1e-5 sdf_trunc of -sdf_trunc) may be left
            out: at most 0.5 % of the updated voxels (asserted here and, for the same inputs, on the CPU).
  mesh      The vertex set equals the restatement's from the same volume within 1e-6 voxel_length; face counts equal.
  scene     1.0 x 0.8 x 0.6 room with a partition, an outer shell 0.15 outside, a void box hidden behind the partition
            (tests/refuse_ref.py); voxel_length 0.02: several 16-voxel units per axis."""
import numpy as np
import pytest
import torch

import refuse_ref as R

pytestmark = pytest.mark.gpu

VL = R.VOXEL
SIZES = [(48, 64), (72, 96)]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulps(a, b):
    def image(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(image(a) - image(b))


def _np(mesh):
    return mesh[0].cpu().numpy(), mesh[1].cpu().numpy()


@pytest.fixture(scope="module")
def scene():
    """Meshes (numpy and device), made once: marching-cubes meshes of the two volumes (triangles near pixel size) and their
    large-triangle twins."""
    from i2sdf_amd.mesh import marching_cubes, Mesh
    out = {}
    for name, (vol, sp, org) in R.scene_volumes().items():
        m = marching_cubes(_cuda(vol), 0.0, spacing=tuple(sp), origin=tuple(org))
        out[name + "_mc"] = Mesh(m.verts, m.faces, m.normals)
    for name, (v, f) in R.scene_triangles().items():
        out[name + "_tri"] = Mesh(_cuda(v), _cuda(f), None)
    return out


@pytest.fixture(scope="module")
def cams():
    from i2sdf_amd.mesh import camera_matrices
    out = {}
    for H, W in SIZES:
        poses, K = R.scene_cameras(H, W)
        c2w, w2c = camera_matrices(torch.from_numpy(poses))
        out[(H, W)] = dict(poses=torch.from_numpy(poses), K=K, c2w=c2w.numpy(), w2c=w2c.numpy())
        poses, K = R.overlapping_cameras(H, W)
        c2w, w2c = camera_matrices(torch.from_numpy(poses))
        out[(H, W, "overlap")] = dict(poses=torch.from_numpy(poses), K=K, c2w=c2w.numpy(), w2c=w2c.numpy())
    return out


_ref_depth_cache = {}


def _ref_depth(scene, cams, name, size, cull):
    key = (name, size, cull)                                              # (size: (H, W), or (H, W, "overlap") for the fusion tests' cameras)
    if key not in _ref_depth_cache:
        v, f = _np(scene[name])
        c = cams[size]
        _ref_depth_cache[key] = R.mesh_depth(v, f, c["w2c"], c["K"], size[0], size[1], cull=cull)
    return _ref_depth_cache[key]


# ------------------------------------------------------------------------------------------------------------- depth
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name,cull", [("trgt_mc", "back"), ("trgt_tri", "back"), ("pred_tri", "none"), ("pred_mc", "none")])
def test_depth_matches_the_restatement(scene, cams, name, cull, size):
    from i2sdf_amd.mesh import mesh_depth
    H, W = size
    c = cams[size]
    stats = []
    got = mesh_depth(scene[name], c["poses"], c["K"], H, W, cull=cull, _stats=stats)
    assert got.shape == (6, H, W) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    ref = _ref_depth(scene, cams, name, size, cull)
    covered = ref["depth"] > 0
    near = ref["near_edge"]
    share = near.sum() / max(covered.sum(), 1)
    mism = (got > 0) != covered
    u = _ulps(got, ref["depth"])[covered & (got > 0)]
    counters = dict(stats)["raster_counters"].cpu().numpy()
    print(f"depth {name} {W}x{H} cull={cull}: {covered.sum()} covered samples, {mism.sum()} mask differences ({(mism & ~near).sum()} away "
          f"from edges), {near.sum()} samples within 1e-6 px of an edge ({share:.2e}), depth differs by at most {u.max()} ulp; "
          f"triangles per camera by workgroup {counters[:, 0].tolist()}, by lane {counters[:, 1].tolist()}")
    assert covered.mean() > 0.95                                          # cameras stand inside a closed room
    assert share <= 1e-3
    assert not (mism & ~near).any()
    assert u.max() <= 1
    # both populations, judged by the box rule (the restatement's own count of it), not by timing
    assert np.array_equal(counters[:, 0], ref["n_large"]) and np.array_equal(counters[:, 1], ref["n_small"])
    if name.endswith("_tri"):
        assert counters[:, 0].min() > 0                                   # walls go to the workgroup-per-triangle kernel
    else:
        # marching-cubes triangles are near pixel size: every camera walks some with one lane each, and over all cameras most of
        # them (a camera close to a surface sees its triangles larger than 64 pixels' box: those go to the other kernel, which is
        # why no count per camera is asked for beyond "some")
        assert counters[:, 1].min() > 0 and counters[:, 1].sum() > counters[:, 0].sum()
    if name == "trgt_tri":
        # every camera has walls behind it and wall triangles that cross its plane z = 0 (and z = znear): clipped by sample
        v, f = _np(scene[name])
        zc = np.stack([R.transform(c["w2c"][k], v)[:, 2] for k in range(6)])
        zf = zc[:, f]
        assert ((zf.min(2) < 0) & (zf.max(2) > 0.05)).any(1).all() and (zc.max(1) > 0).all() and (zc.min(1) < 0).all()


def test_depth_of_a_wall_and_a_sphere_in_closed_form():
    from i2sdf_amd.mesh import mesh_depth
    H, W = 48, 64
    K = np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]])
    poses = torch.eye(4, dtype=torch.float64)[None]
    d, (xa, xb, ya, yb) = 1.7, (-0.61, 0.43, -0.37, 0.52)
    v = np.array([[xa, ya, d], [xb, ya, d], [xb, yb, d], [xa, yb, d]], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    dep = mesh_depth((_cuda(v), _cuda(f)), poses, K, H, W).cpu().numpy()[0]
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    x, y = (uu - K[0, 2]) / K[0, 0] * d, (vv - K[1, 2]) / K[1, 1] * d
    inside = (x > xa) & (x < xb) & (y > ya) & (y < yb)
    assert np.array_equal(dep > 0, inside)
    assert np.abs(dep[inside] - np.float32(d)).max() <= np.spacing(np.float32(d))
    assert (mesh_depth((_cuda(v), _cuda(f[:, ::-1].copy())), poses, K, H, W).cpu().numpy() == 0).all()        # back face, culled
    assert np.array_equal(mesh_depth((_cuda(v), _cuda(f[:, ::-1].copy())), poses, K, H, W, cull="none").cpu().numpy()[0], dep)
    # sphere: between the sphere and the sphere shrunk by the tessellation's sag (bound from the longest edge, see the CPU test)
    Rad, centre = 0.5, np.array([0.1, -0.05, 2.0])
    sv, sf = R.uv_sphere(Rad, 24, 48, centre)
    dep = mesh_depth((_cuda(sv), _cuda(sf)), poses, K, H, W).cpu().numpy()[0]
    e = np.concatenate([sv[sf[:, i]] - sv[sf[:, (i + 1) % 3]] for i in range(3)])
    L = np.linalg.norm(e.astype(np.float64), axis=1).max()
    r_in = np.sqrt(Rad ** 2 - L ** 2 / 2)
    dirs = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu, float)], -1)

    def hit(r):
        a, b, c = (dirs ** 2).sum(-1), -2 * (dirs @ centre), centre @ centre - r * r
        disc = b * b - 4 * a * c
        return np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.nan), disc

    (z_out, disc_out), (z_in, disc_in) = hit(Rad), hit(r_in)
    core = disc_in > 0
    tol = 4 * np.spacing(np.float32(2.0))
    assert core.sum() > 300 and (dep[disc_out < 0] == 0).all() and (dep[core] > 0).all()
    assert (dep[core] >= z_out[core] - tol).all() and (dep[core] <= z_in[core] + tol).all()


def test_shared_edges_through_samples_are_covered_once():
    """Two triangles sharing an edge that runs exactly through pixel samples: the image equals the restatement's everywhere (no sample
    is left out here), which the CPU test shows to cover every sample once; both triangle orders give the same image."""
    from i2sdf_amd.mesh import mesh_depth, camera_matrices
    H, W = 48, 64
    Kp = np.array([[32.0, 0, 32.0], [0, 32.0, 24.0], [0, 0, 1]])
    poses = torch.eye(4, dtype=torch.float64)[None]
    w2c = camera_matrices(poses)[1].numpy()
    d = 2.0
    cases = [(np.array([[-1.0, -1.0, d], [0.5, -1.0, d], [0.5, 1.0, d], [-1.0, 1.0, d], [1.5, -1.0, d], [1.5, 1.0, d]], np.float32),
              np.array([[0, 2, 1], [0, 3, 2], [1, 5, 4], [1, 2, 5]], np.int32)),
             (np.array([[-0.5, -1.0, d], [1.5, 1.0, d], [-0.5, 1.0, d], [1.5, -1.0, d]], np.float32), np.array([[0, 2, 1], [0, 1, 3]], np.int32))]
    for v, f in cases:
        ref = R.mesh_depth(v, f, w2c, Kp, H, W)
        assert ref["near_edge"].sum() >= 20 and ref["hits"].max() == 1
        for ff in (f, f[::-1].copy()):
            got = mesh_depth((_cuda(v), _cuda(ff)), poses, Kp, H, W).cpu().numpy()
            assert np.array_equal(got > 0, ref["depth"] > 0)
            assert _ulps(got, ref["depth"]).max() <= 1


# ------------------------------------------------------------------------------------------------------------ fusion
@pytest.fixture(scope="module")
def fused(scene, cams):
    """The restatement's depth maps of the marching-cubes room from the six overlapping cameras, fused on the device and by the
    restatement (once per size / stride)."""
    from i2sdf_amd.mesh import tsdf_integrate
    out = {}
    for size, stride in ((SIZES[0], 4), (SIZES[0], 1), (SIZES[1], 4)):
        c = cams[size + ("overlap",)]
        depth = _ref_depth(scene, cams, "trgt_mc", size + ("overlap",), "back")["depth"]
        stats = []
        vol = tsdf_integrate(_cuda(depth), c["poses"], c["K"], voxel_length=VL, depth_trunc=5.0, depth_sampling_stride=stride, _stats=stats)
        ref = R.tsdf_integrate(depth, c["c2w"], c["w2c"], c["K"], voxel_length=VL, depth_trunc=5.0, stride=stride)
        out[(size, stride)] = (vol, ref, depth)
    return out


@pytest.mark.parametrize("key", [(SIZES[0], 4), (SIZES[0], 1), (SIZES[1], 4)])
def test_fusion_matches_the_restatement(fused, key):
    vol, ref, _ = fused[key]
    units = vol.units.cpu().numpy()
    assert np.array_equal(units, ref["units"]), "the sets of allocated units differ"
    span = units.max(0) - units.min(0) + 1
    assert (span >= 3).all() and units.shape[0] >= 30                     # several units per axis: cells cross unit borders
    assert tuple(vol.slot.shape) == tuple(span) and int((vol.slot >= 0).sum()) == units.shape[0]
    w, t = vol.weight.cpu().numpy(), vol.tsdf.cpu().numpy()
    updated = ref["weight"] > 0
    skip = ref["borderline"]
    share = (skip & updated).sum() / updated.sum()
    r64 = ref["tsdf64"].astype(np.float32)                                # the fp64 value rounded
    err = _ulps(t, r64)
    averaged = updated & (ref["weight"] >= 3) & (ref["tmax"] < 1)         # three or more cameras, a fractional t from each of them
    rounds = updated & (ref["tsdf32"] != r64)
    exact = t[~skip] == ref["tsdf32"][~skip]
    print(f"fusion {key}: {units.shape[0]} units, {updated.sum()} updated voxels, weights {np.bincount(ref['weight'][updated]).tolist()}, "
          f"{averaged.sum()} averaged over >= 3 fractional t; borderline share {share:.2e}; weight differences {(w != ref['weight']).sum()} "
          f"({((w != ref['weight']) & ~skip).sum()} not borderline); tsdf vs fp64 rounded: max {err[updated & ~skip].max()} ulp "
          f"({err[averaged & ~skip].max()} on the averaged ones; the fp32 chain itself differs from it in {rounds.sum()} voxels); "
          f"not equal to the fp32 restatement bit for bit: {(~exact).sum()}")
    # the inputs exercise the rule: many voxels averaged over several fractional t, and fp32 and fp64 averages that differ
    assert averaged.sum() >= 5000 and rounds.sum() >= 1000 and (rounds & averaged).sum() >= 1000
    assert share <= 5e-3
    assert np.array_equal(w[~skip], ref["weight"][~skip].astype(np.float32))
    assert err[updated & ~skip].max() <= 4
    assert exact.all()
    assert (t[~updated & ~skip] == 0).all()


@pytest.mark.parametrize("key", [(SIZES[0], 4), (SIZES[1], 4)])
def test_extraction_matches_the_restatement(fused, key):
    from i2sdf_amd.mesh import tsdf_extract
    vol, _, _ = fused[key]
    mesh = tsdf_extract(vol)
    v, f = _np(mesh)
    n = mesh.normals.cpu().numpy()
    units, t, w = vol.units.cpu().numpy().astype(np.int64), vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    rv, rf = R.tsdf_extract(units, t, w, VL)
    print(f"extraction {key}: {v.shape[0]} vertices / {f.shape[0]} faces, restatement {rv.shape[0]} / {rf.shape[0]}")
    assert v.shape == rv.shape and f.shape[0] == rf.shape[0] and v.shape[0] > 2000

    def srt(a):
        q = np.round(a.astype(np.float64) / (VL * 1e-3)).astype(np.int64)
        return a[np.lexsort((q[:, 2], q[:, 1], q[:, 0]))]
    dv = np.abs(srt(v).astype(np.float64) - srt(rv).astype(np.float64)).max()
    print(f"  sorted vertex sets differ by at most {dv:.3e} (bar {1e-6 * VL:.1e})")
    assert dv <= 1e-6 * VL
    assert f.min() >= 0 and f.max() < v.shape[0] and np.unique(f).shape[0] == v.shape[0]      # every vertex is used
    # winding towards positive tsdf: the face normal agrees with the tsdf gradient at the face's nearest voxel
    org, dense, valid = R.dense_volume(units, t, w)
    a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
    fn = np.cross(b - a, c - a)
    keep = np.linalg.norm(fn, axis=1) > 1e-9 * VL * VL                    # (a triangle squeezed to a line has no direction)
    cen = (a + b + c) / 3
    fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-300)
    ul = np.float64(np.float32(np.float32(16) * np.float32(VL)))

    def sample(p):                                                        # trilinear tsdf at world points (all 8 corners are valid near faces)
        g = (p - org * ul) / np.float64(np.float32(VL)) - 0.5
        i0 = np.floor(g).astype(np.int64)
        fr = g - i0
        out = np.zeros(p.shape[0])
        for cx in range(8):
            o = np.array([cx & 1, (cx >> 1) & 1, (cx >> 2) & 1])
            ii = np.clip(i0 + o, 0, np.array(dense.shape) - 1)
            wgt = np.prod(np.where(o == 1, fr, 1 - fr), axis=1)
            out += wgt * dense[ii[:, 0], ii[:, 1], ii[:, 2]]
        return out
    step = 0.25 * VL
    rise = sample(cen + step * fn) - sample(cen - step * fn)
    print(f"  faces wound against the tsdf gradient: {(rise[keep] <= 0).sum()} of {keep.sum()}")
    assert (rise[keep] > 0).all()
    # vertex normals: unit length, on the side of the face normals
    ln = np.linalg.norm(n, axis=1)
    assert np.abs(ln[ln > 0] - 1).max() < 1e-5 and (ln > 0).mean() > 0.999
    assert ((n[f[:, 0]] * fn).sum(1)[keep] > 0).mean() > 0.99
    # no edge is shared by more than two faces
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key_ = np.minimum(e[:, 0], e[:, 1]) * v.shape[0] + np.maximum(e[:, 0], e[:, 1])
    _, cnt = np.unique(key_, return_counts=True)
    assert cnt.max() <= 2
    dk = e[:, 0] * v.shape[0] + e[:, 1]
    assert np.unique(dk).shape[0] == dk.shape[0]                          # consistently oriented: no directed edge twice


# -------------------------------------------------------------------------------------------------------- end to end
def _dist_visible(p):
    return R.distance_to_box_surface(p, R.VIS_LO, R.VIS_HI)


@pytest.mark.parametrize("size,stride,name,cull", [(SIZES[0], 4, "pred_mc", "back"), (SIZES[0], 1, "pred_tri", "none"),
                                                   (SIZES[1], 4, "pred_tri", "back"), (SIZES[1], 1, "pred_mc", "none")])
def test_refuse_keeps_what_cameras_see_and_nothing_else(scene, cams, size, stride, name, cull):
    """cull="back" is the default pipeline (the reference's): the meshes of this scene face the free space the cameras stand in, so
    both modes have to keep the same surfaces."""
    from i2sdf_amd.mesh import refuse
    H, W = size
    c = cams[size]
    m = refuse(scene[name], c["poses"], c["K"], H, W, voxel_length=VL, depth_sampling_stride=stride, cull=cull)
    v = m.verts.cpu().numpy().astype(np.float64)
    assert v.shape[0] > 2000 and m.faces.shape[0] > 4000
    d_shell = R.distance_to_box_surface(v, R.SHELL_LO, R.SHELL_HI)
    d_hidden = R.distance_to_box_surface(v, R.HIDDEN_LO, R.HIDDEN_HI)
    d_room = _dist_visible(v)
    print(f"refuse {name} {W}x{H} stride {stride} cull={cull}: {v.shape[0]} vertices; nearest to the shell {d_shell.min():.3f}, to the hidden box "
          f"{d_hidden.min():.3f}; farthest from the visible room's surface {d_room.max():.4f} (voxel {VL})")
    assert d_shell.min() > 0.05 and d_hidden.min() > 0.05
    assert d_room.max() <= VL
    pts, seen = R.visible_lattice(c["c2w"], c["w2c"], c["K"], H, W)
    assert seen.sum() > 100
    near = np.array([np.sqrt(((v - p) ** 2).sum(1).min()) for p in pts[seen]])
    print(f"  {seen.sum()} of {pts.shape[0]} lattice points are seen; farthest from a vertex {near.max():.4f} (bar {2 * VL})")
    assert near.max() <= 2 * VL


def test_far_clip_drops_the_far_wall(scene, cams):
    from i2sdf_amd.mesh import refuse
    H, W = SIZES[0]
    c = cams[SIZES[0]]
    two = c["poses"][[1, 4]]                 # one looks at the partition x = 0.70 from 0.48 away, one down at the floor from 0.38 above it
    full = refuse(scene["trgt_tri"], two, c["K"], H, W, voxel_length=VL).verts.cpu().numpy()
    cut = refuse(scene["trgt_tri"], two, c["K"], H, W, far_clip=0.43, voxel_length=VL).verts.cpu().numpy()
    assert (np.abs(full[:, 0] - 0.70) < VL).sum() > 200 and (np.abs(full[:, 2]) < VL).sum() > 200
    assert (np.abs(cut[:, 2]) < VL).sum() > 200 and (np.abs(cut[:, 0] - 0.70) < 0.05).sum() == 0
    assert cut.shape[0] < full.shape[0]


def test_score_is_refuse_refuse_evaluate_and_beats_the_unrefused_scores(scene, cams):
    from i2sdf_amd.mesh import refuse, evaluate, score
    H, W = SIZES[0]
    c = cams[SIZES[0]]
    pred, trgt = scene["pred_mc"], scene["trgt_mc"]
    thr = 0.05
    raw = evaluate(pred, trgt, threshold=thr)
    got = score(pred, trgt, c["poses"], c["K"], H, W, far_clip=3.0, threshold=thr, voxel_length=VL)
    want = evaluate(refuse(pred, c["poses"], c["K"], H, W, voxel_length=VL), refuse(trgt, c["poses"], c["K"], H, W, 3.0, voxel_length=VL),
                    threshold=thr)
    print(f"unrefused {raw}\nrefused   {got}")
    assert got == want                                                    # exactly: the same calls
    assert 0.1 < raw["Prec"] < 0.9
    assert got["Prec"] > raw["Prec"] and got["Recal"] > raw["Recal"]
    assert got["Prec"] > 0.99 and got["Recal"] > 0.99                     # what the cameras see of the two scenes is the same surface
    default = score(pred, trgt, c["poses"], c["K"], H, W)                 # the reference's voxel_length 0.01
    assert default["Prec"] > raw["Prec"] and default["Recal"] > raw["Recal"]


# ------------------------------------------------------------------------------------------------------- other cases
def test_everything_is_bitwise_reproducible(scene, cams):
    from i2sdf_amd.mesh import mesh_depth, tsdf_integrate, tsdf_extract
    H, W = SIZES[0]
    c = cams[SIZES[0]]
    runs = []
    for _ in range(2):
        d = mesh_depth(scene["pred_mc"], c["poses"], c["K"], H, W, cull="none")
        vol = tsdf_integrate(d, c["poses"], c["K"], voxel_length=VL)
        m = tsdf_extract(vol)
        runs.append((d, vol.tsdf, vol.weight, vol.units, vol.slot, m.verts, m.faces, m.normals))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_empty_inputs():
    from i2sdf_amd.mesh import mesh_depth, tsdf_fuse, refuse, tsdf_integrate
    dev = torch.device("cuda")
    K = np.array([[50.0, 0, 31.5], [0, 50.0, 23.5], [0, 0, 1]])
    poses = torch.eye(4)[None].repeat(2, 1, 1)
    ev, ef = torch.empty(0, 3, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev)
    d = mesh_depth((ev, ef), poses, K, 48, 64)
    assert d.shape == (2, 48, 64) and (d == 0).all()
    v, f = R.box_mesh((-1, -1, 1), (1, 1, 2))
    assert mesh_depth((_cuda(v), _cuda(f)), poses[:0], K, 48, 64).shape == (0, 48, 64)
    for m in (tsdf_fuse(d, poses, K), refuse((ev, ef), poses, K, 48, 64), refuse((_cuda(v), _cuda(f)), poses[:0], K, 48, 64),
              tsdf_fuse(torch.full((2, 48, 64), 7.0, device=dev), poses, K, depth_trunc=5.0)):
        assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.normals.shape == (0, 3) and m.verts.is_cuda
    assert tsdf_integrate(d, poses, K).tsdf.shape == (0, 4096)


def test_bad_arguments_raise():
    from i2sdf_amd.mesh import mesh_depth, tsdf_fuse, refuse, score
    from i2sdf_amd.lib import I2SDFError
    K = np.array([[50.0, 0, 31.5], [0, 50.0, 23.5], [0, 0, 1]])
    poses = torch.eye(4)[None]
    v, f = R.box_mesh((-1, -1, 1), (1, 1, 2))
    mesh = (_cuda(v), _cuda(f))
    sing = poses.clone()
    sing[0, 0, 0] = 0.0
    for kw in (dict(cull="front"), dict(znear=0.0), dict(zfar=0.01), dict(zfar=float("inf")), dict(H=0), dict(W=-3), dict(poses=sing),
               dict(poses=torch.eye(4)), dict(poses=poses.to(torch.int32)), dict(K=np.eye(2)), dict(K=np.zeros((3, 3))),
               dict(mesh=(mesh[0].cpu(), mesh[1])), dict(mesh=(mesh[0], mesh[1].long())), dict(mesh=(mesh[0].double(), mesh[1]))):
        a = dict(mesh=mesh, poses=poses, K=K, H=48, W=64)
        a.update(kw)
        with pytest.raises(ValueError):
            mesh_depth(a.pop("mesh"), a.pop("poses"), a.pop("K"), a.pop("H"), a.pop("W"), **a)
    bad_face = (mesh[0], torch.tensor([[0, 1, 99]], dtype=torch.int32, device="cuda"))
    with pytest.raises(I2SDFError):
        mesh_depth(bad_face, poses, K, 48, 64)
    d = torch.full((1, 48, 64), 1.5, device="cuda")
    for kw in (dict(voxel_length=0.0), dict(voxel_length=-1.0), dict(sdf_trunc=0.0), dict(depth_trunc=0.0), dict(depth_sampling_stride=0),
               dict(depths=d.cpu()), dict(depths=d.double()), dict(depths=d[0]), dict(poses=poses.repeat(2, 1, 1)), dict(poses=sing)):
        a = dict(depths=d, poses=poses, K=K)
        a.update(kw)
        with pytest.raises(ValueError):
            tsdf_fuse(a.pop("depths"), a.pop("poses"), a.pop("K"), **a)
    with pytest.raises(ValueError):
        refuse(mesh, poses, K, 48, 64, bogus=1)
    with pytest.raises(ValueError):
        score(mesh, (mesh[0].cpu(), mesh[1]), poses, K, 48, 64)
    # an extent that overflows the unit table: two cameras 700 m apart along every axis at a 1 cm voxel span 4400^3 units
    far = poses.repeat(2, 1, 1)
    far[1, :3, 3] = 700.0
    with pytest.raises(I2SDFError, match="2\\^24"):
        tsdf_fuse(d.repeat(2, 1, 1), far, K, voxel_length=0.01)
