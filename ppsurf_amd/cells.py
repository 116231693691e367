"""The cell grid over a device array of positions (csrc/pps_cells.h): box, table scratch, step rule and budget search
shared by cloud.VoxelGrid (float32) and simplify.ClusterGrid (float64)."""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_AXIS = 1 << 20


class CellGrid:
    """Box of `pos` [n,3] in its own real type (float32 or float64: lo, hi numpy, ext the longest edge), the lazy cell table, `step` and
    `search`.  A subclass adds its kernels and `count_at(G)`.  `capacity` (a power of two > n) is a test switch: results do not depend on it."""

    def __init__(self, pos: torch.Tensor, capacity=None):
        self.real = np.float32 if pos.dtype == torch.float32 else np.float64
        self.lo, self.hi = pos.min(dim=0)[0].cpu().numpy(), pos.max(dim=0)[0].cpu().numpy()
        self.ext = self.real((self.hi - self.lo).max())
        self.capacity = int(capacity) if capacity is not None else int(_lib.lib().pps_cloud_table_capacity(int(pos.shape[0])))
        self.device = pos.device
        self._table = self._best = None
        self._count = torch.zeros(1, dtype=torch.int64, device=pos.device)

    def _scratch(self, best=False):
        if self._table is None:
            self._table = torch.empty(self.capacity, dtype=torch.int64, device=self.device)
        if best and self._best is None:
            self._best = torch.empty(self.capacity, dtype=torch.int64, device=self.device)

    def _vec3(self, v):
        """lo or hi as the C array of the grid's type."""
        return ((ctypes.c_float if self.real is np.float32 else ctypes.c_double) * 3)(*[float(x) for x in v])

    def step(self, G):
        """h, 1 / h (the grid's type) of the grid with G cells along the longest edge: the quotient in fp64, rounded once."""
        h = self.real(np.float64(self.ext) / np.float64(G))
        return h, self.real(1.0) / h

    def _inv(self, h, inv_h):
        return self.real(1.0) / self.real(h) if inv_h is None else inv_h

    def search(self, budget):
        """The budget search: G_lo of the bisection with count_at(G_lo) <= budget < count_at(G_hi), 20 counting passes."""
        g_lo, g_hi = 1, MAX_AXIS
        while g_hi - g_lo > 1:
            mid = (g_lo + g_hi) // 2
            if self.count_at(mid) <= budget:
                g_lo = mid
            else:
                g_hi = mid
        return g_lo
