"""numpy restatement of the trim by support (ppsurf_amd/csrc/pps_tri.h, pps_trim.hip, ppsurf_amd/trim.py): the
specification the GPU is held to, bit for bit.  Every step is one float64 numpy operation in the order the kernel uses; nothing here comes
from the device, and nothing here knows of cells: support is brute force over all (face, point) pairs.
"""
import numpy as np

import transfer_spec

D = np.float64


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _clamp01(v):
    return np.where(v < 0, D(0), np.where(v > 1, D(1), v))          # a NaN stays a NaN, as in the kernel's selects


def closest_on_triangle(p, a, b, c):
    """(s, t, d2) float64 [m] of closest_on_triangle<double> (csrc/pps_tri.h) for points p [m,3] against ONE triangle a, b, c [3], operation
    for operation: the closest point is a + s ab + t ac, d2 its squared distance (the interior region as the plane distance h h / n.n); a
    face with n.n <= 1e-12 |ab|^2 |ac|^2 is its longest edge."""
    p = np.asarray(p, dtype=D).reshape(-1, 3)
    a, b, c = (np.asarray(x, dtype=D).reshape(3) for x in (a, b, c))
    m = p.shape[0]
    with np.errstate(all='ignore'):
        ab, ac, bc = b - a, c - a, c - b
        n = _cross(ab, ac)
        nn, lab, lac = _dot(n, n), _dot(ab, ab), _dot(ac, ac)
        if not nn > D(1e-12) * (lab * lac):
            lbc = _dot(bc, bc)
            o, e, le, which = a, ab, lab, 0
            if lac > le:
                e, le, which = ac, lac, 1
            if lbc > le:
                o, e, le, which = b, bc, lbc, 2
            u = _clamp01(_dot(p - o[None], e[None]) / le) if le > 0 else np.zeros(m, dtype=D)
            s = u if which == 0 else (np.zeros(m, dtype=D) if which == 1 else D(1) - u)
            t = np.zeros(m, dtype=D) if which == 0 else u
            q = o[None] + u[:, None] * e[None]
            dq = p - q
            return s, t, _dot(dq, dq)
        ap, bp, cp = p - a[None], p - b[None], p - c[None]
        d1, d2_, d3, d4, d5, d6 = _dot(ab[None], ap), _dot(ac[None], ap), _dot(ab[None], bp), _dot(ac[None], bp), _dot(ab[None], cp), _dot(ac[None], cp)
        vc, vb, va = d1 * d4 - d3 * d2_, d5 * d2_ - d1 * d6, d3 * d6 - d5 * d4
        s, t = np.zeros(m, dtype=D), np.zeros(m, dtype=D)
        region = np.full(m, -1, dtype=np.int64)                      # the first rule that holds, in the kernel's order
        rules = [(d1 <= 0) & (d2_ <= 0),                             # 0 vertex a
                 (d3 >= 0) & (d4 <= d3),                             # 1 vertex b
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),                  # 2 edge ab
                 (d6 >= 0) & (d5 <= d6),                             # 3 vertex c
                 (vb <= 0) & (d2_ >= 0) & (d6 <= 0),                 # 4 edge ac
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]    # 5 edge bc
        for k, rule in enumerate(rules):
            region[(region < 0) & rule] = k
        region[region < 0] = 6                                       # interior
        s[region == 1] = 1
        t[region == 3] = 1
        r = region == 2
        s[r] = _clamp01(d1[r] / (d1[r] - d3[r]))
        r = region == 4
        t[r] = _clamp01(d2_[r] / (d2_[r] - d6[r]))
        r = region == 5
        w = _clamp01((d4[r] - d3[r]) / ((d4[r] - d3[r]) + (d5[r] - d6[r])))
        s[r], t[r] = D(1) - w, w
        r = region == 6
        den = (va[r] + vb[r]) + vc[r]
        si = np.where(den > 0, _clamp01(vb[r] / den), D(0))
        ti = np.where(den > 0, _clamp01(vc[r] / den), D(0))
        over = si + ti > 1
        k = D(1) / (si + ti)
        s[r], t[r] = np.where(over, si * k, si), np.where(over, ti * k, ti)
        q = (a[None] + s[:, None] * ab[None]) + t[:, None] * ac[None]
        dq = p - q
        d2 = _dot(dq, dq)
        h = _dot(ap, n[None])
        d2[r] = (h[r] * h[r]) / nn
    return s, t, d2


def face_d2(cloud, verts, faces):
    """float64 [nf]: the smallest d2 of any cloud point to every face; inf for a face with an index outside [0, nv) or a non-finite corner
    and for an empty cloud, NaN distances never win."""
    cloud = np.asarray(cloud, dtype=np.float32).astype(D).reshape(-1, 3)
    verts = np.asarray(verts, dtype=np.float32).astype(D).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = verts.shape[0]
    out = np.full(faces.shape[0], np.inf, dtype=D)
    if cloud.shape[0] == 0:
        return out
    for f, (i0, i1, i2) in enumerate(faces):
        if not (0 <= i0 < nv and 0 <= i1 < nv and 0 <= i2 < nv):
            continue
        a, b, c = verts[i0], verts[i1], verts[i2]
        if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
            continue
        d2 = closest_on_triangle(cloud, a, b, c)[2]
        d2 = d2[~np.isnan(d2)]
        if d2.size:
            out[f] = d2.min()
    return out


def face_support_spec(cloud, verts, faces, r):
    """bool [nf]: face f is supported iff its indices lie in [0, nv), its corners are finite and some cloud point has d2 <= r * r (one
    float64 multiply).  Brute force over all pairs."""
    r = D(r)
    return face_d2(cloud, verts, faces) <= r * r


def spacing_spec(cloud, k=8):
    """float: sqrt(float64(m)), m the LOWER median (rank (n - 1) // 2 in ascending order) of the float32 squared distances of every point to
    its k-th nearest other point -- column k of the (k + 1)-NN search of the cloud in itself (column 0 is the point or a duplicate of it)."""
    cloud = np.asarray(cloud, dtype=np.float32)
    n = cloud.shape[0]
    if n <= k:
        raise ValueError('spacing needs more than k = {} points, got {}'.format(k, n))
    col = transfer_spec.knn(cloud, cloud, k + 1)[1][:, k]
    m = np.sort(col)[(n - 1) // 2]
    assert m.dtype == np.float32
    return float(np.sqrt(D(m)))


def threshold_cases():
    """[(name, verts f32 [3,3], point f32 [3], distance)] with dyadic coordinates, so that every product and sum of closest_on_triangle and
    r * r are exact: the point is at exactly `distance` from the triangle (0,0,0) (4,0,0) (0,4,0) -- over the interior at height 0.5, off
    the edge ab and off the vertex a by a 3-4-5 offset scaled by 2^-3 (0.625)."""
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32)
    return [('interior', tri, np.array([1.0, 1.0, 0.5], dtype=np.float32), 0.5),
            ('edge', tri, np.array([1.0, -0.375, 0.5], dtype=np.float32), 0.625),
            ('vertex', tri, np.array([-0.375, -0.5, 0.0], dtype=np.float32), 0.625)]
