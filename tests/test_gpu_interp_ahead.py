"""The split-precision interpolation kernel one trip ahead: by default interp_pool_f16x3_kernel loads the neighbour ids and
coordinates of a workgroup's next tile during the current trip and stages half of its G rows in LDS; PPS_INTERP_AHEAD=0 (read per call) selects
the schedule in which every trip fetches its own data at its head.  Both feed the same values into the same operations in the same order, so the
pooled feature, the logits and the occupancy must be EQUAL, not close.  Sizes assume a 256-CU chip (one workgroup per CU, two queries per tile)."""
import numpy as np
import pytest
import torch

from ppsurf_amd import ops
from ppsurf_amd.decoder import DecoderPlan
from ppsurf_amd.synthetic import make_band_queries, make_cloud, make_latents, network_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = 50
_plans, _inputs, _reference = {}, {}, {}

# (N, Q, k) -> what the shape does to the kernel
CASES = {(2000, 1, 64): 'one half-valid tile, no next trip',
         (2000, 2, 64): 'one whole tile',
         (2000, 3, 64): 'the last tile is half valid',
         (2000, 37, 64): 'ragged, one trip per workgroup',
         (2000, 1030, 64): '515 tiles on 256 workgroups: at least two trips for some workgroups, one for others; the half-valid last tile is prefetched',
         (2000, 4200, 64): 'ragged, multi-trip',
         (2000, 1030, 37): 'k = 37: rows >= k are masked and read the id of row 0',
         (2000, 3, 37): 'k = 37 on a half-valid tile',
         (50, 600, 50): 'a cloud of 50 points: k clamped to the cloud'}


def plan(which=0, dtype='f16x3'):
    if (which, dtype) not in _plans:
        _plans[which, dtype] = DecoderPlan(network_state_dict('ppsurf', num_pts_local=P), DEV, dtype=dtype)
    return _plans[which, dtype]


def inputs(n, q, k, scale=1.0):
    """(latents, pts, queries, neighbour ids, patches) on the device, made once per shape"""
    if (n, q, k, scale) not in _inputs:
        cloud = make_cloud(n, seed=13)
        qry = make_band_queries(cloud, q, resolution=65, seed=q + k)
        pts, qd = torch.from_numpy(cloud).to(DEV), torch.from_numpy(qry).to(DEV)
        patches = torch.from_numpy(np.random.default_rng(q + n).uniform(-1.0, 1.0, (q, P, 3)).astype(np.float32)).to(DEV)
        lat = torch.from_numpy(make_latents(256, cloud.shape[0], seed=17)[0] * np.float32(scale)).to(DEV)
        _inputs[n, q, k, scale] = (lat, pts, qd, ops.knn_point_major(pts, qd, k), patches)
    return _inputs[n, q, k, scale]


def decode(pl, n, q, k, scale=1.0):
    """-> (pooled, logits, occ) of one decode() call, cloned"""
    lat, pts, qd, idx, patches = inputs(n, q, k, scale)
    logits, occ = pl.decode(pl.point_table(lat), pts, qd, idx, patches)
    torch.cuda.synchronize()
    return pl.intermediates(q)['pooled'].clone(), logits.clone(), occ.clone()


def reference(monkeypatch, n, q, k, scale=1.0):
    """the same call with every trip fetching its own data: computed once per shape, never changed"""
    if (n, q, k, scale) not in _reference:
        monkeypatch.setenv('PPS_INTERP_AHEAD', '0')
        _reference[n, q, k, scale] = decode(plan(), n, q, k, scale)
        monkeypatch.delenv('PPS_INTERP_AHEAD')
    return _reference[n, q, k, scale]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('n,q,k', sorted(CASES))
def test_a_trip_ahead_gives_the_bits_of_the_reference_schedule(monkeypatch, n, q, k):
    want = reference(monkeypatch, n, q, k)
    assert all(torch.isfinite(t).all() for t in want)
    got = decode(plan(), n, q, k)
    for name, a, b in zip(('pooled', 'logits', 'occ'), got, want):
        assert torch.equal(a, b), (name, CASES[n, q, k])


def test_the_claiming_instantiation_still_equals_the_fixed_share(monkeypatch):
    """PPS_TILE_CLAIMS bit 1: the interpolation kernel claims its tiles and keeps the trip head it had; the fixed share runs a trip ahead"""
    want = reference(monkeypatch, 2000, 1030, 64)
    monkeypatch.setenv('PPS_TILE_CLAIMS', '1')
    assert same(decode(plan(), 2000, 1030, 64), want)
    monkeypatch.delenv('PPS_TILE_CLAIMS')
    assert same(decode(plan(), 2000, 1030, 64), want)


def test_repeated_calls_carry_nothing_over(monkeypatch):
    """The staging slots hold the rows of the last tile of the call before: a different shape in between, then the first shape again"""
    want, other = reference(monkeypatch, 2000, 1030, 64), reference(monkeypatch, 2000, 37, 64)
    pl = plan()
    for _ in range(2):
        assert same(decode(pl, 2000, 1030, 64), want)
        assert same(decode(pl, 2000, 37, 64), other)


def test_two_plans_on_two_streams(monkeypatch):
    want = reference(monkeypatch, 2000, 1030, 64)
    plans = [plan(1), plan(2)]
    lat, pts, qd, idx, patches = inputs(2000, 1030, 64)
    tables = [pl.point_table(lat) for pl in plans]
    for pl, table in zip(plans, tables):                        # workspaces allocated before the streams start
        pl.decode(table, pts, qd, idx, patches)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in plans]
    out = []
    for _ in range(3):                                          # a few calls back to back on each stream, so that the two really overlap
        for pl, table, st in zip(plans, tables, streams):
            with torch.cuda.stream(st):
                out.append(pl.decode(table, pts, qd, idx, patches))
    torch.cuda.synchronize()
    for logits, occ in out:
        assert torch.equal(logits, want[1]) and torch.equal(occ, want[2])
    for pl in plans:
        assert torch.equal(pl.intermediates(1030)['pooled'], want[0])


def test_the_range_guard_sees_the_same_values(monkeypatch):
    """Latents scaled until |G| > 65504 (as tests/test_gpu_decoder.py::test_f16x3_range_guard_falls_back_to_fp32): the staged and the loaded half of a
    row both pass the guard's running maximum, the chunk is recomputed by the fp32 kernels and equals the fp32 plan's, and the next ordinary chunk
    runs in split precision again"""
    n, q, k, scale = 2000, 1030, 64, 1.0e5
    pl, pl32 = plan(), plan(dtype='f32')
    lat, pts, qd, idx, patches = inputs(n, q, k, scale)
    assert float(pl32.point_table(lat).abs().max()) > 65504.0   # the test really leaves the range
    before = pl.range_fallbacks()
    got = decode(pl, n, q, k, scale)
    assert pl.range_fallbacks() == before + 1
    want = decode(pl32, n, q, k, scale)
    assert all(torch.isfinite(t).all() for t in got) and same(got, want)
    assert same(got, reference(monkeypatch, n, q, k, scale))
    # the next, ordinary chunk: split precision again, and the bits of the reference schedule
    ordinary = reference(monkeypatch, n, q, k)
    fallbacks = pl.range_fallbacks()
    assert same(decode(pl, n, q, k), ordinary)
    assert pl.range_fallbacks() == fallbacks
    assert not torch.equal(ordinary[1], decode(pl32, n, q, k)[1])
