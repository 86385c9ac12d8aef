"""CPU: the numpy restatement of the visibility culling (tests/refuse_ref.py) against closed-form geometry, so that the GPU tests that
compare the kernels with it do not rest on the restatement alone.  Neither open3d nor pyrender is available to compare with."""
import numpy as np
import pytest

import refuse_ref as R

K = np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]])
H, W = 48, 64


def _mats(poses):
    from i2sdf_amd.mesh import camera_matrices
    import torch
    c2w, w2c = camera_matrices(torch.as_tensor(np.asarray(poses)))
    return c2w.numpy(), w2c.numpy()


def _identity_cam():
    return _mats(np.eye(4)[None])


def _wall(xa, xb, ya, yb, d, flip=False):
    v = np.array([[xa, ya, d], [xb, ya, d], [xb, yb, d], [xa, yb, d]], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2]], np.int32)                       # right-hand normal towards -z: facing a camera at the origin
    return v, (f[:, ::-1].copy() if flip else f)


def test_camera_matrices_invert_poses():
    P = np.stack([R.look_at((0.3, -0.2, 0.1), (1, 2, 0.5)), R.look_at((1, 1, 1), (0, 0, 0))])
    c2w, w2c = _mats(P)
    for c in range(2):
        full = np.eye(4)
        full[:3] = w2c[c]
        assert np.allclose(full @ P[c], np.eye(4), atol=1e-6)
        assert np.array_equal(c2w[c], P[c][:3].astype(np.float32))
    # x right, y down, z forward: a right-handed frame whose z axis looks at the target
    assert np.allclose(np.cross(P[0][:3, 0], P[0][:3, 1]), P[0][:3, 2], atol=1e-12)
    from i2sdf_amd.mesh import camera_matrices
    import torch
    bad = torch.eye(4)[None].clone()
    bad[0, :3, :3] = 0.0
    with pytest.raises(ValueError):
        camera_matrices(bad)
    with pytest.raises(ValueError):
        camera_matrices(torch.eye(3)[None])


def test_fronto_parallel_wall_has_its_distance_inside_its_silhouette_and_zero_outside():
    d = 1.7
    xa, xb, ya, yb = -0.61, 0.43, -0.37, 0.52                           # (no silhouette edge runs through a pixel sample)
    v, f = _wall(xa, xb, ya, yb, d)
    _, w2c = _identity_cam()
    out = R.mesh_depth(v, f, w2c, K, H, W)
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    x, y = (uu - K[0, 2]) / K[0, 0] * d, (vv - K[1, 2]) / K[1, 1] * d
    inside = (x > xa) & (x < xb) & (y > ya) & (y < yb)
    assert inside.sum() > 500 and (~inside).sum() > 500
    dep = out["depth"][0]
    assert np.array_equal(dep > 0, inside)
    assert np.abs(dep[inside] - np.float32(d)).max() <= np.spacing(np.float32(d))
    assert (out["hits"][0][inside] == 1).all() and (out["hits"][0][~inside] == 0).all()     # the diagonal is covered once
    assert out["n_large"][0] == 2 and out["n_small"][0] == 0


def test_sphere_depth_lies_between_the_sphere_and_the_sphere_shrunk_by_the_sag():
    Rad, centre = 0.5, np.array([0.1, -0.05, 2.0])
    v, f = R.uv_sphere(Rad, 24, 48, centre)
    _, w2c = _identity_cam()
    dep = R.mesh_depth(v, f, w2c, K, H, W)["depth"][0]
    # every point of a triangle lies on a segment between a vertex and a point of the opposite edge; both ends are at radius >=
    # sqrt(R^2 - L^2 / 4) and the segment is no longer than L, the longest edge: the mesh stays outside radius sqrt(R^2 - L^2 / 2)
    e = np.concatenate([v[f[:, i]] - v[f[:, (i + 1) % 3]] for i in range(3)])
    L = np.linalg.norm(e.astype(np.float64), axis=1).max()
    r_in = np.sqrt(Rad ** 2 - L ** 2 / 2)
    assert Rad - r_in < 0.02
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    dirs = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu, float)], -1)

    def hit(r):                                                          # z of the first intersection of t * dirs with the sphere
        a, b, c = (dirs ** 2).sum(-1), -2 * (dirs @ centre), centre @ centre - r * r
        disc = b * b - 4 * a * c
        return np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.nan), disc

    z_out, disc_out = hit(Rad)
    z_in, disc_in = hit(r_in)
    assert (dep[disc_out < 0] == 0).all()                                # the mesh lies inside the sphere: no hit where the ray misses it
    core = disc_in > 0                                                   # the ray reaches the inner sphere: it must have crossed the mesh
    assert core.sum() > 300
    assert (dep[core] > 0).all()
    tol = 4 * np.spacing(np.float32(2.0))                                # (fp32 vertices, fp32 projection)
    assert (dep[core] >= z_out[core] - tol).all() and (dep[core] <= z_in[core] + tol).all()
    assert float((z_in - z_out)[core].min()) > 0


def test_two_triangles_sharing_an_edge_cover_every_sample_once():
    _, w2c = _identity_cam()
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    Kp = np.array([[32.0, 0, 32.0], [0, 32.0, 24.0], [0, 0, 1]])          # powers of two: an edge can run exactly through samples
    # (a) a vertical shared edge at x = 0.25 * d -> column u = 32 + 8 exactly; (b) a diagonal that runs through samples (u - v = 8);
    # (c) a generic one
    d = 2.0
    quads = [np.array([[-1.0, -1.0, d], [0.5, -1.0, d], [0.5, 1.0, d], [-1.0, 1.0, d], [1.5, -1.0, d], [1.5, 1.0, d]], np.float32)]
    faces = [np.array([[0, 2, 1], [0, 3, 2], [1, 5, 4], [1, 2, 5]], np.int32)]
    quads.append(np.array([[-0.5, -1.0, d], [1.5, 1.0, d], [-0.5, 1.0, d], [1.5, -1.0, d]], np.float32))        # diagonal x - y = 0.5
    faces.append(np.array([[0, 2, 1], [0, 1, 3]], np.int32))
    quads.append(np.array([[-0.83, -0.61, 1.9], [0.77, -0.52, 2.3], [0.69, 0.58, 2.6], [-0.71, 0.66, 2.1]], np.float32))
    faces.append(np.array([[0, 2, 1], [0, 3, 2]], np.int32))
    on_edge = 0
    for v, f in zip(quads, faces):
        for cull in ("back", "none"):
            for ff in (f, f[::-1].copy()):                               # (the order of the triangles must not matter)
                out = R.mesh_depth(v, ff, w2c, Kp, H, W, cull=cull)
                assert out["hits"].max() == 1, "a sample is covered twice"
                # no hole: the union of the two triangles is a convex quad; every sample strictly inside it is covered
                single = R.mesh_depth(v, ff, w2c, Kp, H, W, cull="none")
                assert np.array_equal(out["hits"], single["hits"])
        on_edge += int(out["near_edge"].sum())
        hull = out["hits"][0] > 0
        assert hull.sum() > 200
        # rows are covered without gaps (a sample lost on the shared edge would leave a hole)
        for r in range(H):
            cols = np.nonzero(hull[r])[0]
            assert cols.size == 0 or cols.size == cols[-1] - cols[0] + 1
    assert on_edge >= 40, "the cases meant to put samples exactly on an edge did not"


def test_back_faces_and_znear():
    _, w2c = _identity_cam()
    v, f = _wall(-0.5, 0.5, -0.4, 0.4, 1.5, flip=True)                   # faces away
    assert (R.mesh_depth(v, f, w2c, K, H, W, cull="back")["depth"] == 0).all()
    both = R.mesh_depth(v, f, w2c, K, H, W, cull="none")["depth"]
    front = R.mesh_depth(*_wall(-0.5, 0.5, -0.4, 0.4, 1.5), w2c, K, H, W)["depth"]
    assert np.array_equal(both, front) and (front > 0).sum() > 300
    # in front of znear, beyond zfar: nothing
    assert (R.mesh_depth(*_wall(-0.5, 0.5, -0.4, 0.4, 0.04), w2c, K, H, W)["depth"] == 0).all()
    assert (R.mesh_depth(*_wall(-0.5, 0.5, -0.4, 0.4, 1.5), w2c, K, H, W, zfar=1.0)["depth"] == 0).all()
    # a floor below the camera that runs from behind it to far in front: y = 0.3, z from -1 to 4.  Samples are clipped, not the
    # triangle: every pixel row below the horizon whose floor depth is >= znear is covered, with depth 0.3 / dy
    fl = np.array([[-2, 0.3, -1.0], [2, 0.3, -1.0], [2, 0.3, 4.0], [-2, 0.3, 4.0]], np.float32)
    ff = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    out = R.mesh_depth(fl, ff, w2c, K, H, W, znear=0.5, cull="none")
    dep = out["depth"][0]
    rows = np.arange(H)
    dy = (rows - K[1, 2]) / K[1, 1]
    with np.errstate(divide="ignore"):
        z = np.where(dy > 0, np.float32(0.3) / dy, -1.0)
    vis = (z >= 0.5) & (z <= 4.0 - 1e-6)
    assert vis.sum() >= 10
    for r in rows:
        if vis[r]:
            x = (np.arange(W) - K[0, 2]) / K[0, 0] * z[r]
            inside = np.abs(x) < 2 - 1e-6
            assert (dep[r][inside] > 0).all(), r
            assert np.abs(dep[r][inside] - z[r]).max() <= 4 * np.spacing(np.float32(z[r]))
        elif dy[r] <= 0:
            assert (dep[r] == 0).all()
    near_rows = (dy > 0) & (np.float32(0.3) / np.where(dy > 0, dy, 1) < 0.5)
    assert (dep[near_rows] == 0).all()                                   # closer than znear: clipped samples
    assert out["hits"].max() == 1


def test_fusing_one_depth_plane_gives_vertices_within_a_voxel_of_it():
    d, vl = 1.013, 0.02
    depth = np.full((1, H, W), d, np.float32)
    c2w, w2c = _identity_cam()
    for stride in (1, 4):
        vol = R.tsdf_integrate(depth, c2w, w2c, K, voxel_length=vl, depth_trunc=5.0, stride=stride)
        assert vol["units"].shape[0] > 4 and vol["weight"].max() == 1
        assert np.array_equal(vol["tsdf32"], vol["tsdf64"].astype(np.float32))      # one camera: t itself, one rounding
        verts, faces = R.tsdf_extract(vol["units"], vol["tsdf32"], vol["weight"], vl)
        assert verts.shape[0] > 1000 and faces.shape[0] > 1000
        # a vertex lies between two voxel centres of opposite sign: within one voxel_length of the plane z = d
        assert np.abs(verts[:, 2] - d).max() <= vl
        # and the plane's part inside the frustum is there: x, y span the image footprint at that depth up to the units' border
        assert verts[:, 0].min() < -0.6 and verts[:, 0].max() > 0.6
        # faces wind towards the camera (positive tsdf is in front of the plane: smaller z)
        a, b, c = (verts[faces[:, i]].astype(np.float64) for i in range(3))
        nz = np.cross(b - a, c - a)[:, 2]
        assert (nz < 0).all()
    # a depth at or beyond depth_trunc is no measurement
    assert R.tsdf_integrate(depth, c2w, w2c, K, voxel_length=vl, depth_trunc=d, stride=1)["units"].shape[0] == 0


def test_the_gpu_tests_scene_stays_under_the_shares_they_may_leave_out():
    """tests/test_gpu_refuse.py may leave out samples within 1e-6 px of an edge (at most 0.1 % of the covered ones) and voxels that are
    borderline in fp64 (at most 0.5 % of the updated ones): the same inputs, built on the host, stay under both.  The fusion inputs
    also have to exercise the running average: cameras that overlap on the walls, many voxels with three or more fractional t."""
    import mcubes_ref as M
    H_, W_ = 48, 64
    poses, Kc = R.scene_cameras(H_, W_)
    c2w, w2c = _mats(poses)
    vol, sp, org = R.scene_volumes()["trgt"]
    v, f, _ = M.marching_cubes(vol, 0.0, sp, org)
    out = R.mesh_depth(v, f, w2c, Kc, H_, W_)
    covered = out["depth"] > 0
    assert covered.mean() > 0.95 and out["near_edge"].sum() <= 1e-3 * covered.sum()
    assert out["hits"].max() <= 2                                          # (the far wall of the chamber behind the partition also faces the camera)
    assert out["n_small"].min() > 0 and out["n_small"].sum() > out["n_large"].sum()
    tri = R.mesh_depth(*R.scene_triangles()["trgt"], w2c, Kc, H_, W_)
    assert tri["n_large"].min() > 0 and tri["near_edge"].sum() <= 1e-3 * (tri["depth"] > 0).sum()
    # the two versions of the room give the same depth up to the marching-cubes mesh's own error (a fraction of its 2.5 cm grid)
    both = covered & (tri["depth"] > 0)
    assert np.abs(out["depth"] - tri["depth"])[both].max() < 0.03
    # fusion: the cameras of the GPU fusion tests overlap on the walls, so that the running average is exercised
    poses, Kc = R.overlapping_cameras(H_, W_)
    c2w, w2c = _mats(poses)
    out = R.mesh_depth(v, f, w2c, Kc, H_, W_)
    assert (out["depth"] > 0).mean() > 0.95 and out["near_edge"].sum() <= 1e-3 * (out["depth"] > 0).sum()
    for stride in (4, 1):
        fz = R.tsdf_integrate(out["depth"], c2w, w2c, Kc, voxel_length=R.VOXEL, stride=stride)
        upd = fz["weight"] > 0
        assert upd.sum() > 2 * 10 ** 4 and (fz["borderline"] & upd).sum() <= 5e-3 * upd.sum()
        span = fz["units"].max(0) - fz["units"].min(0) + 1
        assert (span >= 3).all()
        # a substantial number of voxels is averaged over three or more cameras with a fractional t (|t| < 1) from each, and the
        # fp32 chain and the fp64 one round differently in many of them: the ulp bar below measures something
        averaged = upd & (fz["weight"] >= 3) & (fz["tmax"] < 1)
        r64 = fz["tsdf64"].astype(np.float32)
        rounds = upd & (fz["tsdf32"] != r64)
        assert averaged.sum() >= 5000 and rounds.sum() >= 1000 and (rounds & averaged).sum() >= 1000
        # the order of the cameras matters to the bits (not to the value): the reversed list gives other roundings somewhere
        rev = R.tsdf_integrate(out["depth"][::-1], c2w[::-1], w2c[::-1], Kc, voxel_length=R.VOXEL, stride=stride)
        assert np.array_equal(rev["weight"], fz["weight"]) and (rev["tsdf32"] != fz["tsdf32"]).sum() >= 100
        assert np.abs(rev["tsdf64"] - fz["tsdf64"]).max() < 1e-12
        i32 = lambda x: np.where(x.view(np.int32) < 0, -(x.view(np.int32).astype(np.int64) & 0x7FFFFFFF), x.view(np.int32).astype(np.int64))
        err = np.abs(i32(fz["tsdf32"]) - i32(r64))
        assert err[upd].max() <= 4                                         # the bar of the GPU test (4 ulp of the value) holds for the fp32 chain itself
