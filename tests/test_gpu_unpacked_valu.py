"""The split-precision decoder kernels are compiled without packed fp32 VALU (PPS_PLAIN_F32, pps_common.h): v_add_f32 / v_mul_f32 / v_fma_f32 where
hipcc used to pair two lanes of an f32x4 into v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32.  A plain op rounds exactly as the packed one, so every
output BIT must be what the kernels gave before: g [Q, 256], xbar [Q, 128], logits [Q, 2] and occupancy [Q] of DecoderPlan(dtype='f16x3') are compared
with torch.equal against tests/golden/unpacked_valu.npz, recorded on an MI355X from the commit BEFORE the change (tests/golden/make_unpacked_valu.py).

Inputs: a seeded 2 000-point synthetic cloud, its first Q points as queries, exact neighbour ids from the CPU oracle, seeded patches, formula-filled
weights.  The shapes are the smallest at which each touched path runs:
    Q   1: the remainder launch;  9: one packed group + remainder;  37: a partial 16-query pass of the fused kernel with an idle second query
    P   50: packed, fb = 3;  17: padded second tile;  66: fb > 3, the running-maximum loop
    k   64;  37: invalid rows in the softmax
    switches (read at every launch)   as launched;  PPS_PN_FUSED=0: pointnet_stn_fc_h_kernel + pointnet_feat_rows_kernel<true>;  PPS_STN_TILES=2:
    the two-tiles-at-a-time schedule of pointnet_stn_rows_kernel<true>
The two switches select other schedules of the same arithmetic (tests/test_gpu_pointnet_fused.py, tests/test_gpu_stn_rows_tiles.py), so one record per
(Q, P, k) serves all three; the recorder checks that on the parent before it writes."""
import os

import numpy as np
import pytest
import torch

from oracle import ppsurf_oracle as O
from ppsurf_amd.decoder import DecoderPlan
from ppsurf_amd.synthetic import make_cloud, make_latents, network_state_dict

DEV = 'cuda:0'
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unpacked_valu.npz')
N_CLOUD = 2000
# (Q, P, k): every value of the three tables above, every P at two query counts, k = 37 at every P
CASES = [(37, 50, 64), (9, 17, 37), (9, 66, 64), (9, 50, 37), (1, 50, 64), (1, 17, 64), (1, 66, 37)]
SWITCHES = {'as_launched': {}, 'two_kernel_pointnet': {'PPS_PN_FUSED': '0'}, 'two_tiles': {'PPS_STN_TILES': '2'}}
NAMES = ('g', 'xbar', 'logits', 'occupancy')
_plans, _scene = {}, {}


def key(q, p, k, name):
    return 'q{}_p{}_k{}_{}'.format(q, p, k, name)


def plan(p):
    if p not in _plans:
        _plans[p] = DecoderPlan(network_state_dict('ppsurf', num_pts_local=p), DEV, dtype='f16x3')
    return _plans[p]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene():
    if not _scene:
        cloud = make_cloud(N_CLOUD, seed=19)
        _scene.update(cloud=cloud, pts=dev(cloud), lat=dev(make_latents(256, N_CLOUD, seed=23)[0]), ids={})
    return _scene


def decode(q, p, k, env, setenv, delenv):
    """-> {name: tensor} of one decode() call at (Q, P, k) under the switches `env`, and the number of fp32 fall-backs it took (must be 0)"""
    s, pl = scene(), plan(p)
    qry = s['cloud'][:q].copy()
    if (q, k) not in s['ids']:
        s['ids'][q, k] = dev(O.knn_point_major(s['cloud'], qry, k))
    patches = dev(np.random.default_rng(1000 * p + q).uniform(-1.0, 1.0, (q, p, 3)).astype(np.float32))
    for name in ('PPS_PN_FUSED', 'PPS_STN_TILES', 'PPS_PN_FORCE_PACK'):
        delenv(name)
    for name, value in env.items():
        setenv(name, value)
    before = pl.range_fallbacks()
    logits, occ = pl.decode(pl.point_table(s['lat']), s['pts'], dev(qry), s['ids'][q, k], patches)
    torch.cuda.synchronize()
    mid = pl.intermediates(q)
    out = {'g': mid['g'].clone(), 'xbar': mid['xbar'].clone(), 'logits': logits.clone(), 'occupancy': occ.clone()}
    return out, pl.range_fallbacks() - before


def test_fixture_holds_every_case():
    """no GPU: the committed record has the four tensors of every case, in the shapes the decoder returns, finite and not trivially zero"""
    with np.load(FIXTURE) as z:
        assert sorted(z.files) == sorted(key(q, p, k, n) for q, p, k in CASES for n in NAMES)
        for q, p, k in CASES:
            shapes = {'g': (q, 256), 'xbar': (q, 128), 'logits': (q, 2), 'occupancy': (q,)}
            for n in NAMES:
                a = z[key(q, p, k, n)]
                assert a.dtype == np.float32 and a.shape == shapes[n] and np.isfinite(a).all() and np.abs(a).max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('switch', sorted(SWITCHES))
@pytest.mark.parametrize('q,p,k', CASES)
def test_outputs_have_the_bits_of_the_packed_build(q, p, k, switch, monkeypatch):
    got, fallbacks = decode(q, p, k, SWITCHES[switch], monkeypatch.setenv, lambda n: monkeypatch.delenv(n, raising=False))
    assert fallbacks == 0                                       # the split-precision kernels' own results, not the fp32 fall-back's
    with np.load(FIXTURE) as z:
        for n in NAMES:
            want = torch.from_numpy(z[key(q, p, k, n)])
            assert torch.equal(got[n].cpu(), want), (q, p, k, switch, n, float((got[n].cpu() - want).abs().max()))
