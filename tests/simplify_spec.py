"""numpy restatement of the mesh simplification (ppsurf_amd/csrc/pps_simplify.hip, ppsurf_amd/simplify.py): the
specification the GPU is held to, bit for bit.  Every fp64 step is one numpy float64 operation, in the order the kernels use; nothing here comes
from the device.  The sequential per-cell sums are done in rounds -- "the r-th member of every segment" -- so that every cell adds its members in
ascending order, one rounding per addition.
"""
import numpy as np

import grid_spec
from grid_spec import MAX_AXIS

D = np.float64


def box(verts):
    return grid_spec.box(verts, D)


def grid_step(ext, G):
    """h and 1 / h of a grid with G cells along the longest box edge `ext`, both in fp64."""
    return grid_spec.grid_step(ext, G, D)


def grid_dims(lo, hi, inv_h):
    return grid_spec.grid_dims(lo, hi, inv_h, D)


def cells(verts, lo, hi, inv_h):
    """Cell coordinates int64 [n,3], dims [3] and 64-bit keys [n]."""
    return grid_spec.cells(verts, lo, hi, inv_h, D)


def leaders(key):
    """leader[v]: the lowest vertex index with the key of v."""
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int64)


def cluster_ids(leader):
    """(cid [nv], number of clusters): the rank of every vertex's leader among all leaders."""
    flag = leader == np.arange(leader.shape[0])
    return (np.cumsum(flag) - 1)[leader].astype(np.int64), int(flag.sum())


def survivors(faces, leader):
    a, b, c = leader[faces[:, 0]], leader[faces[:, 1]], leader[faces[:, 2]]
    return int(((a != b) & (b != c) & (a != c)).sum())


def count(verts, faces, G):
    """Faces whose corners lie in three different cells of the grid with G cells along the longest edge."""
    lo, hi, ext = box(verts)
    if faces.shape[0] == 0 or not ext > 0:
        return 0
    h, inv_h = grid_step(ext, G)
    return survivors(faces, leaders(cells(verts, lo, hi, inv_h)[2]))


def segments(ids, rows):
    """Stable CSR of the entries by row: (order, offsets)."""
    order = np.argsort(ids, kind='stable').astype(np.int64)
    offsets = np.zeros(rows + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(ids, minlength=rows))
    return order, offsets


def segment_sums(values, order, offsets):
    """out[r] = ((0 + values[order[o_r]]) + values[order[o_r + 1]]) + ... for every row r, one round per member position."""
    rows = offsets.shape[0] - 1
    length = offsets[1:] - offsets[:-1]
    out = np.zeros((rows,) + values.shape[1:], dtype=D)
    for r in range(int(length.max()) if rows else 0):
        live = np.nonzero(length > r)[0]
        out[live] = out[live] + values[order[offsets[live] + r]]
    return out


def quadrics(verts, faces, cid, ncell, centre):
    """A [ncell,6] (A00 A01 A02 A11 A12 A22), b [ncell,3], xhat [ncell,3] in the kernel's order."""
    fc = cid[faces]                                                                  # [nf,3]
    e = np.arange(3 * faces.shape[0], dtype=np.int64)
    f, k = e // 3, e % 3
    own = fc[f, k]
    contributes = ~(((k >= 1) & (fc[f, 0] == own)) | ((k == 2) & (fc[f, 1] == own)))
    e, f, own = e[contributes], f[contributes], own[contributes]
    ctr = centre[own]
    q0, q1, q2 = verts[faces[f, 0]] - ctr, verts[faces[f, 1]] - ctr, verts[faces[f, 2]] - ctr
    u, w = q1 - q0, q2 - q0
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    m = (nx * q0[:, 0] + ny * q0[:, 1]) + nz * q0[:, 2]
    terms = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, m * nx, m * ny, m * nz], axis=1)
    order, offsets = segments(own, ncell)                                            # entries ascend inside a cell: e was ascending
    sums = segment_sums(terms, order, offsets)
    v_order, v_off = segments(cid, ncell)
    xsum = segment_sums(verts - centre[cid], v_order, v_off)
    xhat = xsum / (v_off[1:] - v_off[:-1]).astype(D)[:, None]
    return sums[:, :6], sums[:, 6:], xhat


def place(A, b, xhat, h, placement='quadric'):
    """(x [ncell,3] relative to the cell centre, fallback bool [ncell])."""
    if placement == 'mean':
        return xhat.copy(), np.zeros(A.shape[0], dtype=bool)
    a00, a01, a02, a11, a12, a22 = (A[:, i] for i in range(6))
    with np.errstate(all='ignore'):
        trace = (a00 + a11) + a22
        lam = D(1e-3) * trace
        m00, m11, m22, m01, m02, m12 = a00 + lam, a11 + lam, a22 + lam, a01, a02, a12
        r0, r1, r2 = b[:, 0] + lam * xhat[:, 0], b[:, 1] + lam * xhat[:, 1], b[:, 2] + lam * xhat[:, 2]
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        s = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
        half = D(h) * D(0.5)
        wall = half + half * D(2.0 ** -30)                           # a wall is 2^-30 of the half edge thick (csrc/pps_simplify.hip)
        ok = (trace != 0.0) & (np.abs(s[:, 0]) <= wall) & (np.abs(s[:, 1]) <= wall) & (np.abs(s[:, 2]) <= wall)      # a NaN fails
    return np.where(ok[:, None], s, xhat), ~ok


def cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def simplify(verts, faces, G=None, placement='quadric', h=None):
    """The whole simplification on the grid of G cells along the longest edge (or of step h): a dictionary with every intermediate array,
    `verts` f64 [V,3], `faces` int64 [F,3] and the report's integers."""
    verts, faces = np.asarray(verts, dtype=D), np.asarray(faces, dtype=np.int64)
    lo, hi, ext = box(verts)
    out = {'faces_in': int(faces.shape[0]), 'verts_in': int(verts.shape[0]), 'G': G, 'h': None, 'cells': 0, 'survivors': 0, 'faces_out': 0,
           'verts_out': 0, 'fallback': 0, 'flipped': 0, 'verts': np.zeros((0, 3)), 'faces': np.zeros((0, 3), dtype=np.int64)}
    if not ext > 0:
        out['cells'] = 1
        return out
    if h is None:
        h, inv_h = grid_step(ext, G)
    else:
        h = D(h)
        inv_h = D(1.0) / h
    c, dims, key = cells(verts, lo, hi, inv_h)
    leader = leaders(key)
    cid, ncell = cluster_ids(leader)
    out.update(h=float(h), cells=ncell, survivors=survivors(faces, leader), leader=leader, cid=cid)
    if out['survivors'] == 0:
        return out
    lead_of = np.nonzero(leader == np.arange(leader.shape[0]))[0]                      # leader vertex of every cluster, ascending
    centre = lo[None] + (c[lead_of].astype(D) + D(0.5)) * h
    A, b, xhat = quadrics(verts, faces, cid, ncell, centre)
    x, fell = place(A, b, xhat, h, placement)
    pos = centre + x
    new = cid[faces]
    src = np.nonzero((new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 0] != new[:, 2]))[0]
    new = new[src]
    _, first = np.unique(np.sort(new, axis=1), axis=0, return_index=True)             # first face of every unordered triple
    first = np.sort(first)
    new, src = new[first], src[first]
    old = verts[faces[src]]
    n_old = cross(old[:, 1] - old[:, 0], old[:, 2] - old[:, 0])
    moved = pos[new]
    n_new = cross(moved[:, 1] - moved[:, 0], moved[:, 2] - moved[:, 0])
    dot = (n_old[:, 0] * n_new[:, 0] + n_old[:, 1] * n_new[:, 1]) + n_old[:, 2] * n_new[:, 2]
    used = np.zeros(ncell, dtype=bool)
    used[new.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    out.update(A=A, b=b, xhat=xhat, pos=pos, fallback_mask=fell, used=used, centre=centre, verts=pos[used], faces=remap[new],
               faces_out=int(new.shape[0]), verts_out=int(used.sum()), fallback=int(fell.sum()), flipped=int((~(dot > 0)).sum()))
    return out


def budget_search(verts, faces, max_faces, count_fn=None):
    """grid_spec.bisect on the survivor count.  `count_fn(G)` defaults to the numpy count; the device driver passes its own."""
    return grid_spec.bisect(count_fn if count_fn is not None else (lambda G: count(verts, faces, G)), max_faces)


def simplify_budget(verts, faces, max_faces, placement='quadric'):
    """simplify_mesh(max_faces=...): None when the mesh is within the budget already (returned unchanged)."""
    if faces.shape[0] <= max_faces:
        return None
    return simplify(verts, faces, budget_search(np.asarray(verts, dtype=D), np.asarray(faces, dtype=np.int64), max_faces), placement)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------------
def cube_mesh(n=97):
    """The unit cube, n x n quads per side, every quad split along the same diagonal, welded: 6 n^2 + 2 vertices, 12 n^2 faces, outward normals."""
    g = np.arange(n + 1)
    u, v = np.meshgrid(g, g, indexing='ij')
    u, v = u.reshape(-1), v.reshape(-1)
    idx = lambda a, b: a * (n + 1) + b
    qa, qb = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    qa, qb = qa.reshape(-1), qb.reshape(-1)
    quad = np.stack([idx(qa, qb), idx(qa + 1, qb), idx(qa + 1, qb + 1), idx(qa, qb + 1)], axis=1)
    tri = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]])
    grid_pts, grid_faces = [], []
    for axis in range(3):
        for side in (0, 1):
            p = np.zeros((u.shape[0], 3), dtype=np.int64)
            p[:, axis] = side * n
            p[:, (axis + 1) % 3] = u
            p[:, (axis + 2) % 3] = v
            t = tri if side == 1 else tri[:, ::-1]                                   # (e_u x e_v) points along +axis
            grid_faces.append(t + len(grid_pts) * u.shape[0])
            grid_pts.append(p)
    pts, faces = np.concatenate(grid_pts), np.concatenate(grid_faces)
    key = (pts[:, 0] * (n + 1) + pts[:, 1]) * (n + 1) + pts[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')                                         # welded vertices in order of first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    verts = pts[first[order]].astype(D) / D(n)
    return verts, rank[inv.reshape(-1)][faces].astype(np.int64)


def cube_surface_distance(p):
    """Distance of points in or near the unit cube from its surface."""
    p = np.asarray(p, dtype=D)
    inside = np.minimum(p, 1.0 - p).min(axis=1)
    outside = np.sqrt((np.maximum(np.maximum(-p, p - 1.0), 0.0) ** 2).sum(axis=1))
    return np.where(outside > 0, outside, np.abs(inside))
