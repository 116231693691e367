"""numpy restatement of the oriented normals (ppsurf_amd/csrc/pps_normals.hip, ppsurf_amd/normals.py): the specification
the GPU is held to, bit for bit.  Every step is one float64 numpy operation in the order the kernels use; nothing here comes from the device.

Rule A (vertex normals): a face is valid when its three indices lie in [0, nv) and are pairwise distinct; a valid face t = (a, b, c)
contributes the keys (a << 32) | t, (b << 32) | t, (c << 32) | t, so the sorted keys list every vertex's faces in ascending face index.  Per
vertex i: acc = (0, 0, 0); for every face of the row, with n the corner after i and q the one after that, e1 = V[n] - V[i], e2 = V[q] - V[i],
g = e1 x e2; 'area': acc = acc + g; 'max': d = |e1|^2 |e2|^2, acc = acc + g / d when d > 0 and finite.  L = sqrt((ax^2 + ay^2) + az^2); the
normal is f32(acc / L) when L > 0 and finite, else (0, 0, 0).
Rule B (point normals): per row, columns in order, a neighbour counts when 0 <= idx < nv: w = 1 / (double(d2) + eps), T = T + w * double(N[idx]);
normalised as in rule A.
"""
import numpy as np

from smooth_spec import fan, noisy_sphere  # noqa: F401  (the meshes of section 16 serve section 17 too)
from topology_spec import SENTINEL, corner_keys, incidence, valid_faces  # noqa: F401  (the rows of section 17 are restated in topology_spec)
import transfer_spec

D = np.float64
F = np.float32
EPS = 1e-30
WEIGHTS = ('area', 'max')


def _unit(acc):
    """f32 [n,3]: acc / L per component where L = sqrt((ax^2 + ay^2) + az^2) is > 0 and finite, else zeros."""
    with np.errstate(all='ignore'):
        L = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        ok = (L > 0) & np.isfinite(L)
        out = np.zeros(acc.shape, dtype=F)
        out[ok] = (acc[ok] / L[ok][:, None]).astype(F)
    return out


def _cross(e1, e2):
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _len2(e):
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def accumulate(verts, faces, weight='area'):
    """float64 [nv,3]: the sums of rule A before the normalisation.  The sum of a row runs in row order, one float64 addition per face: turn k
    adds the k-th face of every row that has one."""
    assert weight in WEIGHTS
    x = np.asarray(verts, dtype=F).reshape(-1, 3).astype(D)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = x.shape[0]
    offsets, inc = incidence(f, nv)
    deg = np.diff(offsets)
    acc = np.zeros((nv, 3), dtype=D)
    with np.errstate(all='ignore'):
        for k in range(int(deg.max()) if deg.size else 0):
            rows = np.nonzero(deg > k)[0]
            tri = f[inc[offsets[rows] + k]]
            p = np.argmax(tri == rows[:, None], axis=1)               # the corner that is i (a valid face holds i once)
            r = np.arange(rows.shape[0])
            e1 = x[tri[r, (p + 1) % 3]] - x[rows]
            e2 = x[tri[r, (p + 2) % 3]] - x[rows]
            g = _cross(e1, e2)
            if weight == 'max':
                d = _len2(e1) * _len2(e2)
                ok = (d > 0) & np.isfinite(d)
                rows, g = rows[ok], g[ok] / d[ok][:, None]            # a face with d not > 0 and finite adds nothing, not even a zero
            acc[rows] = acc[rows] + g
    return acc


def vertex_normals(verts, faces, weight='area'):
    """float32 [nv,3]: rule A."""
    return _unit(accumulate(verts, faces, weight))


def vertex_info(verts, faces, weight='area'):
    """The `info` of normals.vertex_normals."""
    v = np.asarray(verts, dtype=F).reshape(-1, 3)
    out = vertex_normals(v, faces, weight)
    return {'vertices': int(v.shape[0]), 'faces_valid': int(valid_faces(faces, v.shape[0]).sum()),
            'zero_normals': int((out == 0).all(axis=1).sum()), 'weight': weight}


def blend(idx, d2, normals, eps=EPS):
    """float32 [m,3]: rule B on given neighbours idx int64 [m,k], d2 float32 [m,k] and normals float32 [nv,3]; a separate multiply and add."""
    idx, d2 = np.asarray(idx, dtype=np.int64), np.asarray(d2, dtype=F)
    nrm = np.asarray(normals, dtype=F).reshape(-1, 3)
    m, k = idx.shape
    nv = nrm.shape[0]
    eps = D(eps)
    T = np.zeros((m, 3), dtype=D)
    with np.errstate(all='ignore'):
        for j in range(k):
            t = idx[:, j]
            rows = np.nonzero((t >= 0) & (t < nv))[0]                 # a skipped neighbour adds nothing, not even a zero
            w = D(1.0) / (d2[rows, j].astype(D) + eps)
            prod = w[:, None] * nrm[t[rows]].astype(D)                # rounded on its own ...
            T[rows] = T[rows] + prod                                  # ... then added
    return _unit(T)


def point_normals(points, verts, faces, k=8, weight='area', eps=EPS):
    """float32 [m,3]: rule B with the min(k, nv) nearest vertices by brute force (transfer_spec.knn: exact, ordered by (d2, index))."""
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    v = np.asarray(verts, dtype=F).reshape(-1, 3)
    if pts.shape[0] == 0:
        return np.zeros((0, 3), dtype=F)
    idx, d2 = transfer_spec.knn(v, pts, min(int(k), v.shape[0]))
    return blend(idx, d2, vertex_normals(v, faces, weight), eps)


def point_info(points, verts, faces, k=8, weight='area'):
    """The `info` of normals.point_normals."""
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    v = np.asarray(verts, dtype=F).reshape(-1, 3)
    out = point_normals(pts, v, faces, k, weight)
    return {'points': int(pts.shape[0]), 'vertices': int(v.shape[0]), 'k': min(int(k), int(v.shape[0])),
            'zero_normals': int((out == 0).all(axis=1).sum()), 'weight': weight}


def angle_deg(a, b):
    """Angle in degrees between the rows of two arrays of unit vectors (float64; atan2 of |a x b| and a . b, accurate near 0)."""
    a, b = np.asarray(a, dtype=D), np.asarray(b, dtype=D)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.einsum('ij,ij->i', a, b)))
