"""numpy restatement of the feature-preserving denoising (ppsurf_amd/csrc/pps_denoise.hip, ppsurf_amd/denoise.py): the
specification the GPU is held to, bit for bit.  Every step is one float64 numpy operation in the order the kernels use; nothing here comes
from the device.

Rule (Sun, Rosin, Martin, Langbein 2007): a face is valid when its three indices lie in [0, nv) and are pairwise distinct; an invalid face
has the normal (0, 0, 0) throughout and belongs to no neighbourhood.  The normal of a valid face (a, b, c) is n = (x_b - x_a) x (x_c - x_a),
each component p*q - r*s, over L = sqrt((nx^2 + ny^2) + nz^2) when L > 0 and finite, else zeros.  N(i) is the distinct valid faces that
share a vertex with i, i included, in ascending face index: the duplicate-free union of the three incidence rows of i's corners.  A normal
pass: acc = 0; for j in N(i) ascending, d = (n_i.x n_j.x + n_i.y n_j.y) + n_i.z n_j.z; when d > T, w = (d - T)(d - T) and acc = acc + w n_j;
n_i' = acc / L when L = |acc| > 0 and finite, else n_i.  A vertex pass: for the valid faces k of vertex v in ascending face index,
c_k = ((x_a + x_b) + x_c) / 3.0, t = n_k . (c_k - x_v) (summed like d), acc = acc + n_k t; x_v' = x_v + acc / double(count).  Both are
Jacobi passes; the normals are filtered `normal_iters` times first and then stay fixed over the `vertex_iters` vertex passes.  The state
is float64 on the widened float32 input and is rounded to float32 once at the end.
"""
import numpy as np

from topology_spec import incidence, valid_faces

D = np.float64


def _dot(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]


def _unit_or(acc, otherwise):
    """acc / L per row where L = sqrt((x^2 + y^2) + z^2) is > 0 and finite, the row of `otherwise` elsewhere."""
    L = np.sqrt(_dot(acc, acc))
    good = (L > 0) & np.isfinite(L)
    out = otherwise.copy()
    out[good] = acc[good] / L[good, None]
    return out


def face_normals(verts, faces):
    """float64 [nf,3]: the unit normal of every valid face of the float32 vertices, zeros for an invalid or an area-free one."""
    x = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(D)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = np.nonzero(valid_faces(f, x.shape[0]))[0]
    e1, e2 = x[f[ok, 1]] - x[f[ok, 0]], x[f[ok, 2]] - x[f[ok, 0]]
    g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    n = np.zeros((f.shape[0], 3), dtype=D)
    n[ok] = _unit_or(g, np.zeros_like(g))
    return n


def neighbourhoods(faces, nv):
    """(offsets int64 [nf + 1], nb int64): row i lists N(i) in ascending face index; the row of an invalid face is empty."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows_off, inc = incidence(f, nv)
    ok = valid_faces(f, nv)
    rows = [np.unique(np.concatenate([inc[rows_off[v]:rows_off[v + 1]] for v in f[i]])) if ok[i] else np.zeros(0, dtype=np.int64)
            for i in range(f.shape[0])]
    offsets = np.zeros(f.shape[0] + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([r.shape[0] for r in rows])
    return offsets, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)).astype(np.int64)


def filter_pass(n, offsets, nb, threshold):
    """One Jacobi pass over the normals float64 [nf,3].  The sum of a row runs in row order: turn k visits the k-th neighbour of every row that
    has one."""
    T = D(threshold)
    deg = np.diff(offsets)
    acc = np.zeros_like(n)
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.nonzero(deg > k)[0]
        nj = n[nb[offsets[rows] + k]]
        d = _dot(n[rows], nj)
        take = d > T
        w = (d - T) * (d - T)
        rows, nj, w = rows[take], nj[take], w[take]
        acc[rows] = acc[rows] + w[:, None] * nj
    return _unit_or(acc, n)


def vertex_pass(x, faces, n, rows_off, inc):
    """One Jacobi pass over the positions float64 [nv,3] with the face normals n: turn k visits the k-th face of every vertex that has one."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    deg = np.diff(rows_off)
    acc = np.zeros_like(x)
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.nonzero(deg > k)[0]
        t = inc[rows_off[rows] + k]
        c = ((x[f[t, 0]] + x[f[t, 1]]) + x[f[t, 2]]) / D(3.0)
        s = _dot(n[t], c - x[rows])
        acc[rows] = acc[rows] + n[t] * s[:, None]
    out = x.copy()
    rows = np.nonzero(deg > 0)[0]
    out[rows] = x[rows] + acc[rows] / deg[rows].astype(D)[:, None]
    return out


def filtered_normals_spec(verts, faces, threshold, normal_iters):
    """float64 [nf,3]: the face normals after `normal_iters` passes."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    n = face_normals(v, faces)
    if int(normal_iters) > 0:
        offsets, nb = neighbourhoods(faces, v.shape[0])
        for _ in range(int(normal_iters)):
            n = filter_pass(n, offsets, nb, threshold)
    return n


def denoise_spec(verts, faces, threshold=0.5, normal_iters=5, vertex_iters=10):
    """float32 [nv,3]: the filtered normals, then `vertex_iters` vertex passes on the widened float32 vertices, rounded to float32 once."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if int(vertex_iters) == 0:
        return v.copy()
    n = filtered_normals_spec(v, f, threshold, normal_iters)
    rows_off, inc = incidence(f, v.shape[0])
    x = v.astype(D)
    for _ in range(int(vertex_iters)):
        x = vertex_pass(x, f, n, rows_off, inc)
    return x.astype(np.float32)


def info_spec(verts, faces, threshold=0.5, normal_iters=5, vertex_iters=10):
    """The `info` of denoise.denoise_mesh."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out = denoise_spec(v, f, threshold, normal_iters, vertex_iters)
    ok = valid_faces(f, v.shape[0])
    return {'vertices': int(v.shape[0]), 'faces_valid': int(ok.sum()),
            'degenerate_faces': int((ok & (face_normals(v, f) == 0).all(axis=1)).sum()),
            'moved_vertices': int((out.view(np.int32) != v.view(np.int32)).any(axis=1).sum()),
            'threshold': float(threshold), 'normal_iters': int(normal_iters), 'vertex_iters': int(vertex_iters)}


def cube(n):
    """(verts float64 [nv,3], faces int64 [12 n^2,3], normals float64 [12 n^2,3]): the welded integer lattice on the surface of [0, n]^3 in
    lexicographic order, every unit quad split into two triangles wound outward, and the true (axis) normal of every face."""
    g = np.arange(n + 1)
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    pts = pts[((pts == 0) | (pts == n)).any(axis=1)]
    index = {tuple(p): i for i, p in enumerate(pts.tolist())}
    faces, normals = [], []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3                      # e_u x e_w = e_axis
        for side, sign in ((0, -1.0), (n, 1.0)):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return index[tuple(p)]
                    quad = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]
                    if sign < 0:
                        quad.reverse()
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
                    normal = [0.0, 0.0, 0.0]
                    normal[axis] = sign
                    normals += [normal, normal]
    verts, faces, normals = pts.astype(D), np.array(faces, dtype=np.int64), np.array(normals, dtype=D)
    assert np.array_equal(face_normals(verts, faces), normals)
    return verts, faces, normals


def cube_surface_distance(points, n):
    """float64 [m]: the distance of every point from the surface of the cube [0, n]^3."""
    q = np.abs(np.asarray(points, dtype=D) - n / 2.0) - n / 2.0
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    inside = np.minimum(q.max(axis=1), 0.0)
    return np.abs(outside + inside)


def mean_normal_angle(verts, faces, normals):
    """Degrees: the mean angle between the face normals of the mesh and the given unit normals."""
    got = face_normals(np.asarray(verts, dtype=np.float32), faces)
    return float(np.degrees(np.arccos(np.clip((got * normals).sum(axis=1), -1.0, 1.0))).mean())
