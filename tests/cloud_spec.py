"""numpy restatement of the cloud preparation (ppsurf_amd/csrc/pps_cloud.hip, ppsurf_amd/cloud.py): the specification the
GPU is held to, bit for bit.  Every float32 step is one numpy float32 operation, in the order the kernels use; nothing here comes from the device.
"""
import numpy as np

import grid_spec
from grid_spec import MAX_AXIS

F = np.float32
RED = 512                                       # threads of the one-workgroup reduction


def grid_step(ext, G):
    """h and 1 / h of a grid with G cells along the longest box edge `ext` (float32): the quotient in fp64, rounded once to float32."""
    return grid_spec.grid_step(ext, G, F)


def grid_dims(lo, hi, inv_h):
    return grid_spec.grid_dims(lo, hi, inv_h, F)


def cells(pts, lo, hi, h, inv_h):
    """Cell coordinates int64 [n,3], dims [3] and 64-bit keys [n] of float32 points."""
    return grid_spec.cells(pts, lo, hi, inv_h, F)


def voxel_select(pts, lo, hi, h, inv_h):
    """Ascending indices of the point of every occupied cell that is nearest to the cell centre, ties to the lowest index."""
    pts, lo, h = pts.astype(F), lo.astype(F), F(h)
    c, _, key = cells(pts, lo, hi, h, inv_h)
    centre = lo[None] + (c.astype(F) + F(0.5)) * h
    d = pts - centre
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == F
    order = np.lexsort((np.arange(pts.shape[0]), d2.view(np.uint32), key))          # by key, then d2 bits, then index
    first = np.ones(order.shape[0], dtype=bool)
    first[1:] = key[order][1:] != key[order][:-1]
    return np.sort(order[first]).astype(np.int64)


def voxel_count(pts, lo, hi, h, inv_h):
    return int(np.unique(cells(pts, lo, hi, h, inv_h)[2]).shape[0])


def box(pts):
    return grid_spec.box(pts, F)


def budget_search(pts, max_points, count=None):
    """grid_spec.bisect on the number of occupied cells.  `count(h, inv_h)` defaults to the numpy count; the device driver passes its own."""
    lo, hi, ext = box(pts)
    if count is None:
        count = lambda h, inv_h: voxel_count(pts, lo, hi, h, inv_h)
    return grid_spec.bisect(lambda G: count(*grid_step(ext, G)), max_points)


def subsample(pts, max_points):
    """The voxel stage for a budget: (ascending indices, G, h)."""
    n = pts.shape[0]
    if n <= max_points:
        return np.arange(n, dtype=np.int64), None, None
    lo, hi, ext = box(pts)
    if not ext > 0:
        return np.zeros(1, dtype=np.int64), None, None
    G = budget_search(pts, max_points)
    h, inv_h = grid_step(ext, G)
    return voxel_select(pts, lo, hi, h, inv_h), G, h


def knn_d2(pts, k1, chunk=2048, brute_max=20000):
    """The search's own squared distances (pps_knn.hip:14: (dx*dx + dy*dy) + dz*dz in float32) of the k1 nearest cloud points of every point, in
    (d2, index) order -> float32 [n, k1].  Brute force for small clouds; for large ones a kd-tree (scipy) proposes 2 k1 + 8 candidates per point
    whose float32 distances are then recomputed and ordered here -- the candidate set is checked to be wide enough for float32 rounding."""
    pts = pts.astype(F)
    n = pts.shape[0]
    out = np.empty((n, k1), dtype=F)
    if n <= brute_max:
        idx = np.arange(n, dtype=np.uint64)
        for s in range(0, n, chunk):
            q = pts[s:s + chunk]
            dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None]
            key = np.sort(np.partition(key, k1 - 1, axis=1)[:, :k1], axis=1)
            out[s:s + chunk] = (key >> np.uint64(32)).astype(np.uint32).view(F)
        return out
    from scipy.spatial import cKDTree
    kc = min(n, 2 * k1 + 8)
    dist, cand = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=kc)
    d = pts[:, None, :] - pts[cand]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    key = np.sort((d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64), axis=1)[:, :k1]
    out[:] = (key >> np.uint64(32)).astype(np.uint32).view(F)
    if kc < n:          # a point outside the candidates is at least dist[:, -1] away: farther than the k1-th float32 distance by more than rounding
        assert np.all(out[:, -1].astype(np.float64) < (dist[:, -1] ** 2) * (1 - 1e-5)), 'candidate set too narrow'
    return out


def mean_dist(d2):
    """m_i = (sum over columns 1..k of sqrt(double(d2[i, j])), in column order) / k."""
    k = d2.shape[1] - 1
    s = np.zeros(d2.shape[0], dtype=np.float64)
    for j in range(1, k + 1):
        s = s + np.sqrt(d2[:, j].astype(np.float64))
    return s / np.float64(k)


def block_sum(v):
    """Sum in the order of the one-workgroup reduction: thread t adds v[t], v[t + 512], ... in turn, then the halving tree."""
    n = v.shape[0]
    rows = -(-n // RED)
    pad = np.zeros(rows * RED, dtype=np.float64)
    pad[:n] = v
    pad = pad.reshape(rows, RED)
    acc = np.zeros(RED, dtype=np.float64)
    for r in range(rows):
        if (r + 1) * RED <= n:
            acc = acc + pad[r]
        else:                                   # threads past the end add nothing (not even a +0.0)
            live = n - r * RED
            acc[:live] = acc[:live] + pad[r, :live]
    h = RED // 2
    while h > 0:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def outlier_stats(m, ratio):
    """(mu, sigma, threshold) as the kernel computes them."""
    n = np.float64(m.shape[0])
    mu = block_sum(m) / n
    d = m - mu
    sigma = np.sqrt(block_sum(d * d) / n)
    return mu, sigma, mu + np.float64(ratio) * sigma


def outlier_keep(pts, k, ratio, d2=None):
    """Ascending indices kept by the statistical filter, with m and the statistics.  d2: the (k+1)-NN squared distances (default: knn_d2)."""
    n = pts.shape[0]
    if n <= k:
        return np.arange(n, dtype=np.int64), None, None
    if d2 is None:
        d2 = knn_d2(pts, k + 1)
    m = mean_dist(d2)
    stats = outlier_stats(m, ratio)
    return np.nonzero(m <= stats[2])[0].astype(np.int64), m, stats
