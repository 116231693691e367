"""CPU tier of the tile claims of the split-precision decoder: inside pps_decode_fwd_mixed_f32 a persistent workgroup
takes its next unit of work from a counter instead of walking a fixed share.  Which queries a unit holds is computed by host-device functions
of csrc/pps_decode.hip; ppsx_decode_units lists them on the host, through those functions, in the order the counters hand them out.  Whatever
the order in which workgroups take units, every query must lie in exactly one unit, and a packed unit of the STN rows kernel must lie wholly
below the split point (the packed arithmetic needs its 16 / lo queries per wave group; above the split point a wave has one query)."""
import ctypes

import numpy as np
import pytest

from ppsurf_amd import _lib

KERNELS = {0: ('interp_pool_f16x3', 2), 1: ('pointnet_stn_rows', None), 2: ('pointnet_stn_head_h', 64), 3: ('pointnet_fc3_feat_rows', 16),
           4: ('decode_tail_h', 64)}
QS = (0, 1, 7, 16, 31, 32, 33, 600, 4200, 50000)
PS = (17, 50, 66, 100, 200)
GRIDS = (1, 8, 256, 512)
WAVES = 4                      # wave groups of an STN rows workgroup


def units(kernel, q, p, grid):
    """int64 [n,3] (first query, query count, mode) of ppsx_decode_units; asks for the count first, like a caller would"""
    fn = _lib.lib().ppsx_decode_units
    count = ctypes.c_int64(-1)
    assert fn(kernel, q, p, grid, None, 0, ctypes.byref(count)) == 0
    n = count.value
    out = np.full((max(n, 1), 3), -1, dtype=np.int64)
    assert fn(kernel, q, p, grid, out.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(count)) == 0 and count.value == n
    return out[:n]


def packing(p):
    """(packed, queries per wave group) of a patch size: patch_packing of csrc/pps_decode.hip, restated"""
    lo = p & 15
    packed = p >= 16 and lo in (2, 4, 8)
    return packed, (16 // lo if packed else 1)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('kernel', sorted(KERNELS))
def test_the_units_of_a_kernel_cover_every_query_exactly_once(kernel, p, grid):
    for q in QS:
        u = units(kernel, q, p, grid)
        hits = np.zeros(q, dtype=np.int64)
        for first, count, _ in u.tolist():
            assert count >= 1 and 0 <= first and first + count <= q, (q, first, count)
            hits[first:first + count] += 1
        assert (hits == 1).all(), (KERNELS[kernel][0], q, p, grid)
        assert (np.diff(u[:, 0]) > 0).all()                                  # handed out in ascending order (range by range: ascending too)
        size = KERNELS[kernel][1]
        if size is not None:
            assert len(u) == (q + size - 1) // size and (u[:, 1] <= size).all() and (u[:, 2] == 0).all()
            assert (u[:-1, 1] == size).all()                                 # only the last unit may be short


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('p', PS)
def test_packed_units_of_stn_rows_never_cross_the_split_point(p, grid):
    packed, qg = packing(p)
    for q in QS:
        per_round = grid * WAVES * qg
        split = (q // per_round) * per_round if packed else 0                # whole rounds over the chip's workgroups
        u = units(1, q, p, grid)
        m1 = u[u[:, 2] == 1]
        rest = u[u[:, 2] != 1]
        assert len(m1) == split // (WAVES * qg) and (m1[:, 1] == WAVES * qg).all()           # full packed units only
        assert (m1[:, 0] + m1[:, 1] <= split).all() and (rest[:, 0] >= split).all()
        assert (rest[:, 2] == (2 if packed else 0)).all() and (rest[:, 1] <= WAVES).all()
        assert len(u) == len(m1) + (q - split + WAVES - 1) // WAVES
        if len(m1) and len(rest):
            assert m1[:, 0].max() < rest[:, 0].min()                         # the packed units are handed out first


def test_the_headline_shape_by_hand():
    # Q = 50 000, P = 50 on 512 workgroups: three rounds of 512 x 32 queries packed, 848 queries in 212 units of one query per wave
    u = units(1, 50000, 50, 512)
    assert len(u) == 1536 + 212 and u[1535].tolist() == [49120, 32, 1] and u[1536].tolist() == [49152, 4, 2] and u[-1].tolist() == [49996, 4, 2]
    # Q = 600 is less than one round of 16 384 queries: no packed unit, 150 units of one query per wave; one round and 24 queries: 512 + 6
    assert (units(1, 600, 50, 512)[:, 2] == 2).all() and len(units(1, 600, 50, 512)) == 150
    u = units(1, 16408, 50, 512)
    assert len(u) == 518 and u[511].tolist() == [16352, 32, 1] and u[512].tolist() == [16384, 4, 2]
    # the interpolation kernel: 25 000 tiles of two queries in eight ranges of 3125
    u = units(0, 50000, 50, 256)
    assert len(u) == 25000 and u[3125].tolist() == [6250, 2, 0]
    assert units(0, 7, 50, 256)[-1].tolist() == [6, 1, 0]


def test_bad_arguments_are_refused():
    fn = _lib.lib().ppsx_decode_units
    count = ctypes.c_int64(0)
    for args in ((-1, 10, 50, 8), (5, 10, 50, 8), (0, -1, 50, 8), (0, 10, 0, 8), (0, 10, 50, 0)):
        assert fn(*args, None, 0, ctypes.byref(count)) == 1, args
    assert fn(0, 10, 50, 8, None, 0, None) == 1 and fn(0, 10, 50, 8, None, 4, ctypes.byref(count)) == 1
    assert _lib.EXT_PARAMS['ppsx_decode_units'] == ['kernel', 'q', 'p', 'wgs', 'units', 'capacity', 'count']
