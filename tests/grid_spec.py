"""numpy restatement of the cell grid (ppsurf_amd/csrc/pps_cells.h) in the real type T of the grid: np.float32 for the
voxel stage (tests/cloud_spec.py), np.float64 for the vertex clustering (tests/simplify_spec.py).  Every step is one numpy operation in T, in
the order the kernels use; nothing here comes from the device."""
import numpy as np

MAX_AXIS = 1 << 20


def box(pts, T):
    pts = np.asarray(pts, dtype=T)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return lo, hi, T((hi - lo).max())


def grid_step(ext, G, T):
    """h and 1 / h of a grid with G cells along the longest box edge `ext`: the quotient in fp64, rounded once to T."""
    h = T(np.float64(T(ext)) / np.float64(G))
    return h, T(1.0) / h


def grid_dims(lo, hi, inv_h, T):
    """G_a = int(floor((hi_a - lo_a) * inv_h)) + 1, or None where an axis would need more than 2^20 cells."""
    t = np.floor((np.asarray(hi, dtype=T) - np.asarray(lo, dtype=T)) * T(inv_h))
    if not np.all(t < MAX_AXIS):
        return None
    return t.astype(np.int64) + 1


def cells(pts, lo, hi, inv_h, T):
    """Cell coordinates int64 [n,3], dims [3] and 64-bit keys [n]."""
    pts, lo = np.asarray(pts, dtype=T), np.asarray(lo, dtype=T)
    G = grid_dims(lo, hi, inv_h, T)
    if G is None:
        raise ValueError('more than 2^20 cells along an axis')
    t = np.floor((pts - lo[None]) * T(inv_h))
    c = np.minimum(t.astype(np.int64), (G - 1)[None])
    return c, G, (c[:, 2] * G[1] + c[:, 1]) * G[0] + c[:, 0]


def bisect(count_at, budget):
    """Bisection of the integer G in [1, 2^20] with count_at(G_lo) <= budget < count_at(G_hi): 20 counting passes, the answer is G_lo."""
    g_lo, g_hi, passes = 1, MAX_AXIS, 0
    while g_hi - g_lo > 1:
        mid = (g_lo + g_hi) // 2
        passes += 1
        if count_at(mid) <= budget:
            g_lo = mid
        else:
            g_hi = mid
    assert passes == 20
    return g_lo


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------------
WALL_STEPS = (0.5, 0.25, 0.125, 0.03125)        # exact in both types, and so is every product below: float32 and float64 give the same cells
WALL_CELLS = (124, 717, 3621, 5678)             # occupied cells of wall_clouds()[1] at WALL_STEPS


def wall_clouds():
    """(random float32 cloud [50000,3], float32 cloud [8000,3] in [0, 2]^3 with exact duplicates and points exactly on cell walls: multiples of
    1/8 are exact in float32, walls of the h = 0.125 and h = 0.25 grids) from one RandomState(21)."""
    rng = np.random.RandomState(21)
    rand = (rng.rand(50000, 3) * np.array([1.0, 0.6, 0.3]) - 0.5).astype(np.float32)
    lattice = (rng.randint(0, 17, size=(4000, 3)) / 8.0).astype(np.float32)
    return rand, np.concatenate([lattice, lattice[:1000], (rng.rand(3000, 3) * 2.0).astype(np.float32)])
