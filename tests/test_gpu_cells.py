"""GPU tier of the shared cell grid (csrc/pps_cells.h, ppsurf_amd/cells.py): the float32 instantiation behind
cloud.VoxelGrid and the float64 one behind simplify.ClusterGrid on one cloud where both must find the same cells -- exact duplicates, points on
walls, and a table loaded to 0.69."""
import numpy as np
import pytest
import torch

import cloud_spec
import simplify_spec
from grid_spec import WALL_CELLS, WALL_STEPS, wall_clouds

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def test_both_instantiations_find_the_same_cells():
    from ppsurf_amd import cloud, simplify
    pts = wall_clouds()[1]
    p32, p64 = torch.from_numpy(pts).to(DEV), torch.from_numpy(pts).to(DEV).double()
    no_faces = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    small = 8192                                                 # the smallest legal table for 8 000 points: long probe sequences
    assert small // 2 < pts.shape[0] < small
    p64_host = pts.astype(np.float64)
    lo, hi, _ = simplify_spec.box(p64_host)
    lo32, hi32, _ = cloud_spec.box(pts)
    want = {h: (simplify_spec.leaders(simplify_spec.cells(p64_host, lo, hi, np.float64(1.0) / np.float64(h))[2]),
                cloud_spec.voxel_select(pts, lo32, hi32, np.float32(h), np.float32(1.0) / np.float32(h))) for h in WALL_STEPS}      # nothing from the device
    for cap in (None, small, 8 * small):
        voxels, clusters = cloud.VoxelGrid(p32, capacity=cap), simplify.ClusterGrid(p64, no_faces, capacity=cap)
        assert voxels.capacity == clusters.capacity == (cap or 16384)
        assert voxels.lo.dtype == np.float32 and clusters.lo.dtype == np.float64 and np.array_equal(voxels.lo, clusters.lo)
        for h, occupied in zip(WALL_STEPS, WALL_CELLS):
            want_leader, want_kept = want[h]
            for _ in range(2):
                leader, ncell = clusters.leaders(np.float64(h))
                leader = leader.cpu().numpy()
                assert voxels.count(np.float32(h)) == ncell == occupied, (cap, h)
                assert np.array_equal(leader, want_leader), (cap, h)
                kept = voxels.select(np.float32(h)).cpu().numpy()
                # one winner per cell: as many winners as cells and every leader among theirs, so no two winners share a cell
                assert kept.shape[0] == occupied and np.array_equal(np.sort(leader[kept]), np.unique(want_leader)), (cap, h)
                assert np.array_equal(kept, want_kept), (cap, h)
