"""Tile claims of the split-precision decoder: inside DecoderPlan.decode the persistent f16x3 kernels take their next
unit of work from counters in the head of the workspace; PPS_TILE_CLAIMS=0 (read per call) selects the fixed share of every workgroup.  A query's
values do not depend on the workgroup or the unit that evaluates it, so g, xbar, the logits and the occupancy must be EQUAL, not close, and the
counters must be back at zero behind every call.  Sizes assume a 256-CU chip (256 or 512 workgroups per kernel)."""
import numpy as np
import pytest
import torch

from ppsurf_amd import ops
from ppsurf_amd.decoder import DecoderPlan
from ppsurf_amd.synthetic import make_band_queries, make_cloud, make_latents, network_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_plans, _inputs, _fixed = {}, {}, {}

# (Q, k, P) -> what the shape does to the claiming kernels
CASES = {(1, 64, 50): 'one query: one workgroup per kernel, one claim each',
         (37, 64, 50): 'fewer tiles than workgroups: most workgroups of the streaming kernels would claim nothing -- the grid shrinks to the tiles',
         (600, 64, 50): '300 interpolation tiles on 256 workgroups: some claim twice; STN rows: 150 units of one query per wave',
         (4200, 64, 50): '263 passes of the fused fc3 + feature kernel on 256 workgroups: a second claim there',
         (600, 37, 50): 'k = 37: masked neighbour rows',
         (600, 64, 66): 'P = 66: patches that do not pack, five tiles per query two at a time',
         (16408, 64, 50): 'one whole packed round of STN rows (512 units) and 24 queries behind the split point in the same launch'}


def plan(p, which=0):
    if (p, which) not in _plans:
        _plans[p, which] = DecoderPlan(network_state_dict('ppsurf', num_pts_local=p), DEV, dtype='f16x3')
    return _plans[p, which]


def inputs(q, k, p):
    """(table source, pts, queries, neighbour ids, patches) on the device, made once per shape; the patches are random points of the unit cube"""
    if (q, k, p) not in _inputs:
        cloud = make_cloud(6000, seed=13)
        qry = make_band_queries(cloud, q, resolution=65, seed=q + k)
        pts, qd = torch.from_numpy(cloud).to(DEV), torch.from_numpy(qry).to(DEV)
        patches = torch.from_numpy(np.random.default_rng(q + p).uniform(-1.0, 1.0, (q, p, 3)).astype(np.float32)).to(DEV)
        lat = torch.from_numpy(make_latents(256, cloud.shape[0], seed=17)[0]).to(DEV)
        _inputs[q, k, p] = (lat, pts, qd, ops.knn_point_major(pts, qd, k), patches)
    return _inputs[q, k, p]


def decode(pl, q, k, p, lane=0):
    """-> (g, xbar, logits, occ) of one decode() call, cloned"""
    lat, pts, qd, idx, patches = inputs(q, k, p)
    logits, occ = pl.decode(pl.point_table(lat), pts, qd, idx, patches, lane=lane)
    torch.cuda.synchronize()
    mid = pl.intermediates(q)
    return mid['g'].clone(), mid['xbar'].clone(), logits.clone(), occ.clone()


def fixed_share(monkeypatch, q, k, p):
    """the same call with every kernel on its fixed share: computed once per shape, never changed"""
    if (q, k, p) not in _fixed:
        monkeypatch.setenv('PPS_TILE_CLAIMS', '0')
        _fixed[q, k, p] = decode(plan(p), q, k, p)
        monkeypatch.delenv('PPS_TILE_CLAIMS')
    return _fixed[q, k, p]


def head_words(pl, name='decode_ws'):
    return pl._scratch[name][:16].view(torch.int32).cpu().tolist()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('q,k,p', sorted(CASES))
def test_claimed_tiles_give_the_bits_of_the_fixed_share(monkeypatch, q, k, p):
    want = fixed_share(monkeypatch, q, k, p)
    assert all(torch.isfinite(t).all() for t in want)
    for mask in (None, '31'):                                   # the product's set of claiming kernels, then all five
        if mask is not None:
            monkeypatch.setenv('PPS_TILE_CLAIMS', mask)
        got = decode(plan(p), q, k, p)
        for name, a, b in zip(('g', 'xbar', 'logits', 'occ'), got, want):
            assert torch.equal(a, b), (name, mask, CASES[q, k, p])
        assert head_words(plan(p))[2:] == [0] * 14


def test_a_forced_packed_launch_with_a_short_last_unit(monkeypatch):
    # PPS_PN_FORCE_PACK moves the split point of STN rows to Q: 19 packed units, the last one with 24 of its 32 queries
    want = fixed_share(monkeypatch, 600, 64, 50)
    monkeypatch.setenv('PPS_PN_FORCE_PACK', '1')
    assert same(decode(plan(50), 600, 64, 50), want)
    assert head_words(plan(50))[2:] == [0] * 14


@pytest.mark.parametrize('mask', [1, 2, 4, 8, 16])
def test_every_kernel_claims_on_its_own(monkeypatch, mask):
    """PPS_TILE_CLAIMS as a bit mask: one kernel claims, the others keep the fixed share (the A/B runs of profiles/NOTES_tile_claims.md)"""
    want = fixed_share(monkeypatch, 4200, 64, 50)
    monkeypatch.setenv('PPS_TILE_CLAIMS', str(mask))
    assert same(decode(plan(50), 4200, 64, 50), want)
    assert head_words(plan(50))[2:] == [0] * 14


def test_repeated_calls_leave_the_counters_at_zero(monkeypatch):
    want = fixed_share(monkeypatch, 600, 64, 50)
    pl = plan(50)
    fallbacks = head_words(pl)[1]
    for _ in range(2):                                          # the second call finds what the first one left in the workspace head
        assert same(decode(pl, 600, 64, 50), want)
        words = head_words(pl)
        assert words[2:] == [0] * 14 and words[1] == fallbacks and words[0] == 0


def test_two_plans_on_two_streams(monkeypatch):
    """Each plan has its own workspace and so its own counters: two decodes in flight at once do not see each other"""
    want = fixed_share(monkeypatch, 600, 64, 50)
    plans = [plan(50, 1), plan(50, 2)]
    lat, pts, qd, idx, patches = inputs(600, 64, 50)
    tables = [pl.point_table(lat) for pl in plans]
    for pl, table in zip(plans, tables):                        # workspaces allocated and zeroed before the streams start
        pl.decode(table, pts, qd, idx, patches)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in plans]
    out = []
    for _ in range(3):                                          # a few calls back to back on each stream, so that the two really overlap
        for pl, table, st in zip(plans, tables, streams):
            with torch.cuda.stream(st):
                out.append((pl, pl.decode(table, pts, qd, idx, patches)))
    torch.cuda.synchronize()
    for pl, (logits, occ) in out:
        assert torch.equal(logits, want[2]) and torch.equal(occ, want[3])
    for pl in plans:
        mid = pl.intermediates(600)
        assert torch.equal(mid['g'], want[0]) and torch.equal(mid['xbar'], want[1])
        assert head_words(pl)[2:] == [0] * 14
