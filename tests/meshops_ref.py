"""Numpy restatement of the library's mesh operations (csrc/meshops.hip, i2sdf_amd.mesh / grid.pca_frame): face components on
sorted edge keys with smallest-face-index labels, face and component areas, compaction, trimesh's surface sampling with
explicit draws, and the fixed PCA frame.  Vectorised throughout; shared by the CPU and GPU tests."""
import numpy as np


def edge_keys(faces):
    """(3F,) int64 keys min(a, b) << 32 | max(a, b), entry 3f + c = side (v_c, v_{c+1}) of face f."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f, np.roll(f, -1, axis=1)
    return ((np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1)


def adjacency_pairs(faces):
    """(P, 2) face pairs that share an edge: neighbours in the sorted key order (a run of k equal keys gives k - 1 pairs)."""
    keys = edge_keys(faces)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    same = np.nonzero(sk[1:] == sk[:-1])[0]
    owner = order // 3
    return np.stack([owner[same], owner[same + 1]], -1)


def face_components(faces):
    """labels (F,) int32: the smallest face index of each face's component.  Min-label propagation over the adjacency pairs
    with pointer jumping until nothing changes."""
    F = np.asarray(faces).reshape(-1, 3).shape[0]
    lab = np.arange(F, dtype=np.int64)
    if F == 0:
        return lab.astype(np.int32)
    pairs = adjacency_pairs(faces)
    a, b = pairs[:, 0], pairs[:, 1]
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, lab[a], m)              # hook the LABELS (roots), not only the two faces
        np.minimum.at(new, lab[b], m)
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:                                # pointer jumping: label of my label
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return lab.astype(np.int32)


def canonical(labels):
    """Any labeling -> smallest-member-index labeling."""
    labels = np.asarray(labels)
    first = np.full(int(labels.max()) + 1 if labels.size else 0, labels.size, np.int64)
    np.minimum.at(first, labels, np.arange(labels.size))
    return first[labels].astype(np.int32)


def face_areas(verts, faces, dtype=np.float32):
    """0.5 |(v1 - v0) x (v2 - v0)| with every product and sum rounded in `dtype`."""
    v = np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return (dtype(0.5) * np.sqrt(cx * cx + cy * cy + cz * cz)).astype(dtype)


def component_areas(verts, faces, labels):
    """(labels of the components ascending, their fp64 areas from fp32 face areas)."""
    area = face_areas(verts, faces).astype(np.float64)
    ids, inv = np.unique(labels, return_inverse=True)
    return ids, np.bincount(inv, weights=area, minlength=ids.shape[0])


def compact(verts, faces, normals, mask):
    f = np.asarray(faces).reshape(-1, 3)[np.asarray(mask, bool)]
    used = np.zeros(len(verts), bool)
    used[f.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return verts[used], new[f].astype(np.int32), None if normals is None else normals[used]


def largest_component(verts, faces, normals=None):
    labels = face_components(faces)
    ids, areas = component_areas(verts, faces, labels)
    best = ids[np.argmax(areas)]                   # (first maximum = the smaller label)
    return compact(verts, faces, normals, labels == best)


def area_cdf(verts, faces):
    """fp64 running sum of the fp32 face areas (trimesh sums float64 areas; the library's face areas are fp32)."""
    return np.cumsum(face_areas(verts, faces).astype(np.float64))


def points_on_faces(verts, faces, face_index, u_bary):
    """The sample of trimesh.sample.sample_surface for given faces and barycentric draws, in fp64."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(face_index, np.int64)]
    ab = np.asarray(u_bary, np.float64).copy()
    out = ab.sum(axis=1) > 1.0
    ab[out] = np.abs(ab[out] - 1.0)
    return v[f[:, 0]] + ab[:, :1] * (v[f[:, 1]] - v[f[:, 0]]) + ab[:, 1:] * (v[f[:, 2]] - v[f[:, 0]])


def sample_surface(verts, faces, u_face, u_bary):
    """-> (points (n,3) fp64, face_index (n,) int32, cdf): pick = u_face * cdf[-1], searchsorted side='left', clamped to F-1."""
    cdf = area_cdf(verts, faces)
    pick = np.asarray(u_face, np.float64) * cdf[-1]
    face = np.minimum(np.searchsorted(cdf, pick), cdf.shape[0] - 1)
    return points_on_faces(verts, faces, face, u_bary), face.astype(np.int32), cdf


def pca_frame(points):
    """(vecs with eigenvectors in ROWS, s_mean) in fp64: eigenvalues ascending, each row's largest-magnitude entry positive,
    then rows 1 and 2 swapped when det < 0."""
    p = np.asarray(points, np.float64)
    s_mean = p.mean(axis=0)
    d = p - s_mean
    _, v = np.linalg.eigh(d.T @ d)
    vecs = v.T.copy()
    for r in range(3):
        if vecs[r, np.argmax(np.abs(vecs[r]))] < 0:
            vecs[r] *= -1.0
    if np.linalg.det(vecs) < 0:
        vecs = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0]], np.float64) @ vecs
    return vecs, s_mean
