"""Host tier of the shared cell grid (tests/grid_spec.py): its float32 and float64 instantiations agree where the
arithmetic is exact -- a cloud in [0, 2]^3 with lo = 0 and steps that are powers of two.  No GPU."""
import numpy as np
import pytest

import cloud_spec
import simplify_spec
from grid_spec import WALL_CELLS, WALL_STEPS, wall_clouds


@pytest.mark.parametrize('h,occupied', list(zip(WALL_STEPS, WALL_CELLS)))
def test_float32_and_float64_grids_agree_where_the_arithmetic_is_exact(h, occupied):
    pts = wall_clouds()[1]
    assert pts.shape == (8000, 3) and pts.dtype == np.float32
    lo32, hi32, ext32 = cloud_spec.box(pts)
    lo64, hi64, ext64 = simplify_spec.box(pts.astype(np.float64))
    assert lo32.dtype == np.float32 and lo64.dtype == np.float64 and ext32.dtype == np.float32 and ext64.dtype == np.float64
    assert np.all(lo32 == 0) and np.all(hi32 == 2) and np.array_equal(lo32, lo64) and np.array_equal(hi32, hi64) and ext32 == ext64 == 2
    h32, h64 = np.float32(h), np.float64(h)
    assert h32 == h64 and cloud_spec.grid_step(ext32, round(2 / h)) == (h32, 1 / h32) and simplify_spec.grid_step(ext64, round(2 / h)) == (h64, 1 / h64)
    c32, dims32, key32 = cloud_spec.cells(pts, lo32, hi32, h32, np.float32(1.0) / h32)
    c64, dims64, key64 = simplify_spec.cells(pts.astype(np.float64), lo64, hi64, np.float64(1.0) / h64)
    assert np.array_equal(c32, c64) and np.array_equal(dims32, dims64) and np.array_equal(key32, key64)
    assert dims32.tolist() == [round(2 / h) + 1] * 3
    assert np.unique(key32).shape[0] == occupied == cloud_spec.voxel_count(pts, lo32, hi32, h32, np.float32(1.0) / h32)
