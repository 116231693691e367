"""numpy restatement of the colour transfer (ppsurf_amd/csrc/pps_transfer.hip, ppsurf_amd/transfer.py): the specification
the GPU is held to, bit for bit.  Every step is one numpy operation of the stated type, in the order the kernel uses; nothing here comes from
the device.
"""
import numpy as np

F = np.float32
EPS = 1e-30


def knn(cloud, query, k, chunk=512):
    """(idx int64 [m,k], d2 float32 [m,k]) of the k nearest cloud points of every query by brute force: d2 = (dx*dx + dy*dy) + dz*dz in
    float32 (pps_knn.hip:14), ordered by (d2 bits, index)."""
    cloud, query = cloud.astype(F), query.astype(F)
    n, m = cloud.shape[0], query.shape[0]
    assert 1 <= k <= n
    ids = np.arange(n, dtype=np.uint64)
    idx, d2 = np.empty((m, k), dtype=np.int64), np.empty((m, k), dtype=F)
    for s in range(0, m, chunk):
        q = query[s:s + chunk]
        dx, dy, dz = (q[:, None, a] - cloud[None, :, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None]
        key = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
        idx[s:s + chunk] = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d2[s:s + chunk] = (key >> np.uint64(32)).astype(np.uint32).view(F)
    return idx, d2


def blend(idx, d2, rgba, eps=EPS):
    """uint8 [m,4]: per row, j in column order and all in float64 with a separate multiply and add,
        t = idx[i,j], skipped unless 0 <= t < n;  w = 1 / (double(d2[i,j]) + eps);  S = S + w;  T[c] = T[c] + w * double(rgba[t,c]);
    S == 0 -> 0 0 0 0, otherwise min(255, max(0, floor(T[c] / S + 0.5)))."""
    idx, d2, rgba = np.asarray(idx, dtype=np.int64), np.asarray(d2, dtype=F), np.asarray(rgba, dtype=np.uint8)
    m, k = idx.shape
    n = rgba.shape[0]
    eps = np.float64(eps)
    S = np.zeros(m, dtype=np.float64)
    T = np.zeros((m, 4), dtype=np.float64)
    for j in range(k):
        t = idx[:, j]
        ok = (t >= 0) & (t < n)
        rows = np.nonzero(ok)[0]                                  # a skipped neighbour adds nothing, not even a zero
        w = np.float64(1.0) / (d2[rows, j].astype(np.float64) + eps)
        S[rows] = S[rows] + w
        prod = w[:, None] * rgba[t[rows]].astype(np.float64)      # rounded on its own ...
        T[rows] = T[rows] + prod                                  # ... then added
    out = np.zeros((m, 4), dtype=np.uint8)
    live = S != 0.0
    y = np.floor(T[live] / S[live][:, None] + np.float64(0.5))
    out[live] = np.minimum(255.0, np.maximum(0.0, y)).astype(np.uint8)
    return out


def transfer(cloud, rgb, verts, k=8, eps=EPS):
    """(rgba uint8 [m,4], nearest d2 float32 [m]) as ppsurf_amd.transfer.transfer_colors defines them: [n,3] colours get alpha 255 and k is
    clamped to n."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    n, m = cloud.shape[0], verts.shape[0]
    if n == 0:
        raise ValueError('the cloud has no points')
    if rgb.shape[1] == 3:
        rgb = np.concatenate([rgb, np.full((n, 1), 255, dtype=np.uint8)], axis=1)
    if m == 0:
        return np.zeros((0, 4), dtype=np.uint8), np.zeros((0,), dtype=F)
    idx, d2 = knn(cloud, verts, min(k, n))
    return blend(idx, d2, rgb, eps), d2[:, 0].copy()
