"""pointnet_stn_rows_kernel<true> takes ALL full tiles of a query (at most three: every patch below 64 rows) through the conv chain in one pass over
the streamed weights; PPS_STN_TILES=2 selects the earlier schedule (two tiles at a time, a running maximum in registers).  A maximum does not depend
on how its arguments are grouped and the per-tile arithmetic is the same, so g [Q, 256] -- and everything behind it -- must be EQUAL, not close.
The environment switches are read at every launch, so they are set per call in this process."""
import numpy as np
import pytest
import torch

from oracle import ppsurf_oracle as O
from ppsurf_amd.decoder import DecoderPlan
from ppsurf_amd.synthetic import make_cloud, make_latents, network_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_plans, _scene = {}, {}

# P -> what the kernel does with it (fb full tiles, lo left-over rows, qg queries per wave group)
CASES = {50: 'fb 3, lo 2, qg 8: three tiles in one pass + packed left-overs',
         36: 'fb 2, lo 4, qg 4: two tiles in one pass',
         24: 'fb 1, lo 8, qg 2: one tile',
         48: 'not packed, three full tiles',
         17: 'not packed, second tile padded',
         66: 'fb 4: the two-at-a-time loop, unchanged'}


def plan(p, dtype='f16x3'):
    if (p, dtype) not in _plans:
        _plans[p, dtype] = DecoderPlan(network_state_dict('ppsurf', num_pts_local=p), DEV, dtype=dtype)
    return _plans[p, dtype]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene(q):
    """cloud, queries, neighbour ids and latents for q queries (the PointNet branch reads none of them: only the patches)"""
    if q not in _scene:
        cloud = make_cloud(500, seed=3)
        qry = cloud[:q].copy()
        _scene[q] = (dev(cloud), dev(qry), dev(O.knn_point_major(cloud, qry, 64)), dev(make_latents(256, 500, seed=4)[0]))
    return _scene[q]


def random_patches(q, p, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (q, p, 3)).astype(np.float32)


def decode(pl, patches):
    """-> (g, logits, occ) of one decode() call, cloned"""
    q = patches.shape[0]
    pts, qd, ids, lat = scene(q)
    logits, occ = pl.decode(pl.point_table(lat), pts, qd, ids, patches)
    torch.cuda.synchronize()
    return pl.intermediates(q)['g'].clone(), logits.clone(), occ.clone()


@pytest.mark.parametrize('force_pack', [False, True])
@pytest.mark.parametrize('q', [1, 8, 9, 37])
@pytest.mark.parametrize('p', sorted(CASES))
def test_one_pass_schedule_has_the_bits_of_the_two_tile_schedule(p, q, force_pack, monkeypatch):
    """Q: a lone query, one full wave group at P = 50, a group plus one, a ragged workgroup.  As launched, small Q runs the remainder launch (one query
    per wave group); PPS_PN_FORCE_PACK=1 runs packed rounds."""
    pl = plan(p)
    patches = dev(random_patches(q, p, seed=100 * p + q))
    if force_pack:
        monkeypatch.setenv('PPS_PN_FORCE_PACK', '1')
    else:
        monkeypatch.delenv('PPS_PN_FORCE_PACK', raising=False)
    before = pl.range_fallbacks()
    monkeypatch.delenv('PPS_STN_TILES', raising=False)
    g3, lg3, oc3 = decode(pl, patches)
    monkeypatch.setenv('PPS_STN_TILES', '2')
    g2, lg2, oc2 = decode(pl, patches)
    assert pl.range_fallbacks() == before                       # g is the split-precision kernel's, not the fp32 fall-back's
    assert g3.shape == (q, 256) and torch.isfinite(g3).all() and float(g3.max()) > 0.0
    assert torch.equal(g3, g2), (p, q, force_pack, CASES[p])
    if p == 50:
        assert torch.equal(lg3, lg2) and torch.equal(oc3, oc2)


def test_one_pass_schedule_does_not_depend_on_the_chunking(monkeypatch):
    """37 queries at P = 50, whole and cut as 9 + 28: a query's logits do not depend on where in a chunk it sits."""
    monkeypatch.delenv('PPS_STN_TILES', raising=False)
    monkeypatch.delenv('PPS_PN_FORCE_PACK', raising=False)
    pl = plan(50)
    patches = dev(random_patches(37, 50, seed=7))
    pts, qd, ids, lat = scene(37)
    table = pl.point_table(lat)
    whole = pl.decode(table, pts, qd, ids, patches)[0].clone()
    parts = [pl.decode(table, pts, qd[a:b].contiguous(), ids[a:b].contiguous(), patches[a:b].contiguous())[0].clone() for a, b in ((0, 9), (9, 37))]
    assert torch.equal(torch.cat(parts), whole)


@pytest.mark.parametrize('row', [None, 5, 21, 37, 49])
def test_range_guard_sees_every_tile_of_the_pass(row, monkeypatch):
    """ONE query's patch (row None), or one row of it in the first, second or third full tile or among the left-over rows, scaled until conv0a's output leaves the f16
    range (|w x| ~ 1e6 * 0.5 > 65504): the running magnitude is fed from three tiles per call and none may be lost.  The decode then IS the fp32
    plan's and the plan counts one fall-back (the check of test_f16x3_range_guard_falls_back_to_fp32, at Q = 16)."""
    monkeypatch.delenv('PPS_STN_TILES', raising=False)
    monkeypatch.delenv('PPS_PN_FORCE_PACK', raising=False)
    pl, pl32 = plan(50), plan(50, 'f32')
    host = random_patches(16, 50, seed=11)
    if row is None:
        host[11] *= np.float32(1.0e6)
    else:
        host[11, row] = np.float32(1.0e6) * np.array([0.5, -0.7, 0.6], dtype=np.float32)
    patches = dev(host)
    pts, qd, ids, lat = scene(16)
    before = pl.range_fallbacks()
    logits, occ = pl.decode(pl.point_table(lat), pts, qd, ids, patches)
    want, occ32 = pl32.decode(pl32.point_table(lat), pts, qd, ids, patches)
    assert pl.range_fallbacks() == before + 1
    assert torch.isfinite(logits).all() and torch.equal(logits, want) and torch.equal(occ, occ32)
    # the next, ordinary chunk runs in split precision again
    pl.decode(pl.point_table(lat), pts, qd, ids, dev(random_patches(16, 50, seed=11)))
    assert pl.range_fallbacks() == before + 1
