"""The f16x3 PointNet branch without the round trip of the per-query matrix M through memory (pointnet_stn_head_h_kernel +
pointnet_fc3_feat_rows_kernel, the default) against the two-kernel path that keeps M in the workspace (PPS_PN_FUSED=0): every (row of M, query)
pair and every patch row is accumulated in the same order, so the results are EQUAL, not close.  Parity with the oracle is what the f16x3 cases of
test_gpu_decoder.py check on the default path."""
import numpy as np
import pytest
import torch

from golden_util import filled_sd
from oracle import ppsurf_oracle as O
from ppsurf_amd.decoder import DecoderPlan
from ppsurf_amd.synthetic import make_cloud, make_band_queries, make_latents

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def plan(dtype='f16x3'):
    if dtype not in _cache:
        _cache[dtype] = DecoderPlan(filled_sd('', key='ppsurf'), DEV, dtype=dtype)
    return _cache[dtype]


def scene():
    """One cloud and one latent set for every test of this file (computed once, never changed)."""
    if 'scene' not in _cache:
        cloud = make_cloud(3000, seed=8)
        _cache['scene'] = (cloud, make_latents(256, cloud.shape[0], seed=9)[0])
    return _cache['scene']


def inputs(p, q, seed=2):
    cloud, _ = scene()
    qry = make_band_queries(cloud, q, resolution=65, seed=seed)
    ids = O.knn_point_major(cloud, qry, 64)
    pid = ids[:, :p] if p <= 64 else O.knn_point_major(cloud, qry, p)
    patches = O.normalize_patches(cloud[pid], qry).astype(np.float32)
    return dev(cloud), dev(qry), dev(ids), dev(patches)


def decode(pl, table, args, q, monkeypatch, fused):
    if fused:
        monkeypatch.delenv('PPS_PN_FUSED', raising=False)
    else:
        monkeypatch.setenv('PPS_PN_FUSED', '0')
    logits, occ = pl.decode(table, *args)
    torch.cuda.synchronize()
    return pl.intermediates(q)['xbar'].clone(), logits.clone(), occ.clone()


# (P, Q): one query; the wave / second-query boundary; the pass boundary and its tail; one padded tile; the tile edge; 7 and 13 tiles;
# more than 16 x 256 x 2 queries: every workgroup of a 256-CU chip runs a second and a third pass (exchange buffers reused)
CASES = [(50, 1), (50, 7), (50, 8), (50, 9), (50, 15), (50, 16), (50, 17), (50, 33), (10, 77), (16, 40), (17, 40), (100, 37), (200, 21),
         (50, 8197)]


@pytest.mark.parametrize('p,q', CASES)
def test_fused_equals_two_kernel_path(p, q, monkeypatch):
    pl = plan()
    table = pl.point_table(dev(scene()[1]))
    args = inputs(p, q)
    want = decode(pl, table, args, q, monkeypatch, fused=False)
    got = decode(pl, table, args, q, monkeypatch, fused=True)
    for name, a, b in zip(('xbar', 'logits', 'occupancy'), got, want):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), '{}: {} of {} values differ'.format(name, int((a != b).sum()), a.numel())


def test_range_guard_through_the_fused_kernels(monkeypatch):
    """Latents scaled as in test_gpu_decoder.py::test_f16x3_range_guard_falls_back_to_fp32 (its larger scale, x 1e5): both paths raise the guard word, the fp32
    kernels recompute the chunk, and the next ordinary chunk runs split precision again."""
    pl, pl32 = plan(), plan('f32')
    lat = scene()[1]
    args = inputs(50, 300)
    big = dev(lat * np.float32(1.0e5))
    assert float(pl32.point_table(big).abs().max()) > 65504.0       # the test really leaves the range
    n0 = pl.range_fallbacks()
    want = decode(pl, pl.point_table(big), args, 300, monkeypatch, fused=False)
    n1 = pl.range_fallbacks()
    got = decode(pl, pl.point_table(big), args, 300, monkeypatch, fused=True)
    n2 = pl.range_fallbacks()
    assert n1 - n0 == 1 and n2 - n1 == 1
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    l32, o32 = pl32.decode(pl32.point_table(big), *args)
    assert torch.equal(got[1], l32) and torch.equal(got[2], o32)
    _, l1, _ = decode(pl, pl.point_table(dev(lat)), args, 300, monkeypatch, fused=True)
    l1_32, _ = pl32.decode(pl32.point_table(dev(lat)), *args)
    assert pl.range_fallbacks() == n2 and not torch.equal(l1, l1_32) and float((l1 - l1_32).abs().max()) < 1e-4


def test_a_query_does_not_depend_on_its_place_in_a_pass(monkeypatch):
    """203 queries alone and as rows [5:208] of a 300-query call: another column of the pass, another wave, first or second query of its wave."""
    pl = plan()
    table = pl.point_table(dev(scene()[1]))
    pts, qry, ids, patches = inputs(50, 300, seed=4)
    whole = decode(pl, table, (pts, qry, ids, patches), 300, monkeypatch, fused=True)
    part = decode(pl, table, (pts, qry[5:208].contiguous(), ids[5:208].contiguous(), patches[5:208].contiguous()), 203, monkeypatch, fused=True)
    for a, b in zip(part, whole):
        assert torch.equal(a, b[5:208])
