"""GPU tier of the colour transfer: the search and the blend kernel of csrc/pps_transfer.hip against the numpy
specification tests/transfer_spec.py, bit for bit; the op alone on hand-made indices; `pps.py rec --model.init_args.gen_color_k` and
`python -m ppsurf_amd.transfer` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import transfer_spec as T
from golden_util import REPO
from test_cloud_cpu import ABC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N, M, HITS, DUP, KMAX = 20000, 5000, 1000, 200, 70
START = 968                     # shorter vertex lists start here: they hold exact hits and free vertices alike


@pytest.fixture(scope='module')
def scene():
    """One cloud, one vertex list and ONE brute-force search (k = 70) shared by every case: the k nearest are the first k columns, and the
    neighbours of a vertex do not depend on which other vertices are asked for."""
    rng = np.random.RandomState(31)
    cloud = rng.rand(N, 3).astype(np.float32)
    cloud[N - DUP:] = cloud[:DUP]                                 # 200 points twice, at equal positions with different colours
    rgb = rng.randint(0, 256, size=(N, 3)).astype(np.uint8)
    verts = rng.rand(M, 3).astype(np.float32)
    verts[:HITS] = cloud[:HITS]                                   # 1000 exact hits, the first 200 of them on a duplicated point
    idx, d2 = T.knn(cloud, verts, KMAX)
    assert np.all(d2[:HITS, 0] == 0) and np.all(d2[:DUP, 1] == 0) and np.array_equal(idx[:DUP, 1], np.arange(N - DUP, N))
    dev_cloud = torch.from_numpy(cloud).to(DEV)
    for a in (cloud, rgb, verts, idx, d2):
        a.setflags(write=False)                                   # shared by every case
    return {'cloud': cloud, 'rgb': rgb, 'verts': verts, 'idx': idx, 'd2': d2, 'dev_cloud': dev_cloud}


@pytest.mark.parametrize('k', [1, 8, 70])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 257, 5000])
def test_search_and_blend_match_the_spec_bitwise(scene, m, k):
    from ppsurf_amd import ops, transfer
    lo = 0 if m == M else START
    verts = torch.tensor(scene['verts'][lo:lo + m], device=DEV)
    idx, d2 = scene['idx'][lo:lo + m, :k], scene['d2'][lo:lo + m, :k]
    rgba = np.concatenate([scene['rgb'], np.full((N, 1), 255, dtype=np.uint8)], axis=1)
    want = T.blend(idx, d2, rgba)
    got_idx, got_d2 = ops.KnnBlocks(scene['dev_cloud']).query(verts, k, return_d2=True)
    assert np.array_equal(got_idx.cpu().numpy(), idx) and np.array_equal(got_d2.cpu().numpy().view(np.uint32), d2.view(np.uint32)), 'the search differs'
    for _ in range(2):
        got, near = transfer.transfer_colors(scene['dev_cloud'], scene['rgb'], verts, k=k)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (m, 4) and near.dtype == torch.float32 and tuple(near.shape) == (m,)
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(near.cpu().numpy().view(np.uint32), d2[:, 0].view(np.uint32))
    if m == M:
        assert np.array_equal(want[DUP:HITS], rgba[DUP:HITS])                       # any k: an exact hit outweighs every other neighbour
        if k >= 2:                                                                  # a duplicated point: two equal weights, the mean of two colours
            both = scene['rgb'][:DUP].astype(np.int64) + scene['rgb'][N - DUP:].astype(np.int64)
            assert (both % 2 == 1).any() and np.all(np.abs(2 * want[:DUP, :3].astype(np.int64) - both) <= 1)


def test_small_clouds_and_empty_vertex_lists():
    from ppsurf_amd import transfer
    rng = np.random.RandomState(32)
    verts = rng.rand(100, 3).astype(np.float32)
    for n in (7, 1):
        cloud, rgb = rng.rand(n, 3).astype(np.float32), rng.randint(0, 256, size=(n, 4)).astype(np.uint8)
        want, want_near = T.transfer(cloud, rgb, verts, k=8)                        # k is clamped to n
        got, near = transfer.transfer_colors(torch.from_numpy(cloud).to(DEV), torch.from_numpy(rgb).to(DEV), torch.from_numpy(verts).to(DEV), k=8)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(near.cpu().numpy().view(np.uint32), want_near.view(np.uint32))
        if n == 1:
            assert np.array_equal(want, np.tile(rgb, (100, 1)))
    cloud = torch.from_numpy(rng.rand(50, 3).astype(np.float32)).to(DEV)
    got, near = transfer.transfer_colors(cloud, rng.randint(0, 256, size=(50, 3)).astype(np.uint8), torch.empty((0, 3), device=DEV), k=8)
    assert tuple(got.shape) == (0, 4) and got.dtype == torch.uint8 and tuple(near.shape) == (0,) and near.dtype == torch.float32
    with pytest.raises(ValueError):
        transfer.transfer_colors(torch.empty((0, 3), device=DEV), np.zeros((0, 3), dtype=np.uint8), cloud, k=8)
    for bad in (0, 257):
        with pytest.raises(ValueError):
            transfer.transfer_colors(cloud, np.zeros((50, 3), dtype=np.uint8), cloud, k=bad)
    with pytest.raises(transfer._lib.PpsError):
        transfer.transfer_colors(cloud.cpu(), np.zeros((50, 3), dtype=np.uint8), cloud, k=8)


def test_blend_skips_entries_outside_the_cloud():
    from ppsurf_amd import transfer
    rng = np.random.RandomState(33)
    n, m, k = 300, 777, 5
    rgba = rng.randint(0, 256, size=(n, 4)).astype(np.uint8)
    idx = rng.randint(0, n, size=(m, k)).astype(np.int64)
    d2 = (rng.rand(m, k) ** 4).astype(np.float32)
    d2[rng.rand(m, k) < 0.1] = 0.0
    bad = rng.rand(m, k) < 0.3
    idx[bad] = rng.choice(np.array([-1, n, 1 << 40, -(1 << 40), n + 1], dtype=np.int64), size=int(bad.sum()))
    idx[5] = [-1, n, 1 << 40, -1, n]                              # no valid entry at all
    idx[6] = [-1, n, 7, 1 << 40, -1]
    want = T.blend(idx, d2, rgba)
    assert want[5].tolist() == [0, 0, 0, 0] and want[6].tolist() == rgba[7].tolist()
    got = transfer.blend_rgba(torch.from_numpy(idx).to(DEV), torch.from_numpy(d2).to(DEV), torch.from_numpy(rgba).to(DEV))
    assert np.array_equal(got.cpu().numpy(), want)
    got = transfer.blend_rgba(torch.from_numpy(idx).to(DEV), torch.from_numpy(d2).to(DEV), torch.from_numpy(rgba).to(DEV), eps=1e-3)
    assert np.array_equal(got.cpu().numpy(), T.blend(idx, d2, rgba, eps=1e-3))


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib
    n, m = 40, 130
    rng = np.random.RandomState(34)
    rgba = torch.from_numpy(rng.randint(0, 256, size=(n, 4)).astype(np.uint8)).to(DEV)
    idx = torch.from_numpy(rng.randint(0, n, size=(m, 257)).astype(np.int64)).to(DEV)
    d2 = torch.from_numpy(rng.rand(m, 257).astype(np.float32)).to(DEV)
    out = torch.full((m, 4), 0xA5, dtype=torch.uint8, device=DEV)
    for k, eps in ((0, 1e-30), (257, 1e-30), (4, 0.0), (4, float('nan')), (4, -1.0)):
        rc = _lib.call('ppsx_blend_rgba_u8', idx, d2, m, k, rgba, n, eps, out, unchecked=True)
        torch.cuda.synchronize()
        assert rc == 1 and bool((out == 0xA5).all()), (k, eps)
    for mm, nn in ((-1, n), (m, -1)):
        assert _lib.call('ppsx_blend_rgba_u8', idx, d2, mm, 4, rgba, nn, 1e-30, out, unchecked=True) == 1
    assert _lib.call('ppsx_blend_rgba_u8', None, d2, m, 4, rgba, n, 1e-30, out, unchecked=True) == 1
    assert _lib.call('ppsx_blend_rgba_u8', None, None, 0, 4, None, n, 1e-30, None, on=torch.device(DEV), unchecked=True) == 0       # m == 0
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    with pytest.raises(_lib.PpsError, match='ppsx_blend_rgba_u8 failed with status 1'):
        _lib.call('ppsx_blend_rgba_u8', idx, d2, m, 0, rgba, n, 1e-30, out)
    idx256, d256 = idx[:, :256].contiguous(), d2[:, :256].contiguous()                                                               # 256 is legal
    assert _lib.call('ppsx_blend_rgba_u8', idx256, d256, m, 256, rgba, n, 1e-30, out) == 0
    assert np.array_equal(out.cpu().numpy(), T.blend(idx256.cpu().numpy(), d256.cpu().numpy(), rgba.cpu().numpy()))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _axis_colours(pts):
    """c_a(p) = rint(255 (p_a - lo_a) / (hi_a - lo_a)) per axis, with the box it was made from."""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return np.rint(255.0 * (pts - lo[None]) / (hi - lo)[None]).astype(np.uint8), lo, hi - lo


@pytest.fixture(scope='module')
def rec_runs(tmp_path_factory):
    """`pps.py rec` on a coloured PLY of a golden ABC cloud, with and without gen_color_k 4 (resolution 33, max_points 5000 so that the colours
    must follow the kept rows), and `python -m ppsurf_amd.transfer` on the result: run once for the tests below."""
    from ppsurf_amd import cloud, meshio, runner
    from test_gpu_cloud import _rec_workdir
    tmp = tmp_path_factory.mktemp('transfer_rec')
    pts = meshio.load_pts(ABC)[:, :3].astype(np.float32)
    rgb, lo, ext = _axis_colours(pts.astype(np.float64))
    scan = str(tmp / 'scan.ply')
    meshio.write_ply_mesh_colored(scan, pts, np.zeros((0, 3), dtype=np.int32), rgb)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        _rec_workdir(tmp)
        common = ['--data.init_args.max_points', '5000', '--model.init_args.gen_resolution_global', '33']
        model = runner.main(['pps.py', 'rec', scan, str(tmp / 'out_c'), '--model.init_args.gen_color_k', '4'] + common)
        assert model.gen_color_k == 4 and model.last_prediction is not None and model.last_colors is not None
        last_colors = model.last_colors.copy()
        model = runner.main(['pps.py', 'rec', scan, str(tmp / 'out_p')] + common)
        assert model.gen_color_k is None and model.last_prediction is not None and model.last_colors is None
    finally:
        os.chdir(cwd)
    kept, _ = cloud.prepare_cloud(meshio.load_pts(scan), max_points=5000, device=DEV)
    assert 4 <= kept.shape[0] <= 5000 and kept.shape[0] < pts.shape[0]
    kept_scan = str(tmp / 'kept.ply')                              # the cloud predict_step saw, in the file frame, with its colours
    meshio.write_ply_mesh_colored(kept_scan, pts[kept], np.zeros((0, 3), dtype=np.int32), rgb[kept])
    plain_scan = str(tmp / 'plain.ply')
    meshio.write_ply_points(plain_scan, pts[kept])
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    coloured = str(tmp / 'out_c' / 'scan.ply' / 'scan.ply.ply')
    cli = [subprocess.run([sys.executable, '-m', 'ppsurf_amd.transfer', coloured, s, str(tmp / o), '--k', '4'], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=600) for s, o in ((kept_scan, 'cli.ply'), (plain_scan, 'cli_plain.ply'))]
    return {'tmp': tmp, 'pts': pts, 'rgb': rgb, 'lo': lo, 'ext': ext, 'kept': kept, 'coloured': coloured,
            'plain': str(tmp / 'out_p' / 'scan.ply' / 'scan.ply.ply'), 'last_colors': last_colors, 'cli': cli, 'plain_scan': plain_scan}


def test_rec_writes_the_scans_colours(rec_runs):
    from scipy.spatial import cKDTree
    from ppsurf_amd import meshio
    r = rec_runs
    head_c, head_p = open(r['coloured'], 'rb').read(400), open(r['plain'], 'rb').read(400)
    for name in (b'red', b'green', b'blue', b'alpha'):
        assert b'property uchar ' + name in head_c and b'property uchar ' + name not in head_p
    vc, fc = meshio.read_ply_mesh(r['coloured'], dtype=np.float64)
    vp, fp = meshio.read_ply_mesh(r['plain'], dtype=np.float64)
    assert fc.shape[0] > 0 and np.array_equal(fc, fp) and np.array_equal(vc, vp)
    assert meshio.read_ply_vertex_colors(r['plain']) is None
    q = meshio.read_ply_vertex_colors(r['coloured'])
    assert q.shape == (vc.shape[0], 3) and np.array_equal(q, r['last_colors'][:, :3]) and np.all(r['last_colors'][:, 3] == 255)
    # derived bound: the colour is a convex combination of the colours of kept points within D, the distance to the 4th nearest kept point;
    # c_a is linear in p_a, half a level of rounding on the points' colours and half on the result, 1.001 for the float32 model frame
    D = cKDTree(r['pts'][r['kept']].astype(np.float64)).query(vc, k=4)[0][:, 3]
    ideal = 255.0 * (vc - r['lo'][None]) / r['ext'][None]
    err = np.abs(q.astype(np.float64) - ideal)
    bound = 255.0 * 1.001 * D[:, None] / r['ext'][None] + 1.01
    print('{} vertices, {} kept points; colour error max {:.3f} levels, largest error / bound {:.3f}, median bound {:.2f}'.format(
        vc.shape[0], r['kept'].shape[0], err.max(), (err / bound).max(), np.median(bound)))
    assert np.all(err <= bound)


def test_transfer_command_reproduces_the_colours_of_predict(rec_runs):
    from ppsurf_amd import meshio
    r = rec_runs
    ok, refused = r['cli']
    assert ok.returncode == 0, ok.stderr
    report = json.loads(ok.stdout.strip().split('\n')[-1])
    vc, fc = meshio.read_ply_mesh(r['coloured'], dtype=np.float64)
    assert report['vertices'] == vc.shape[0] and report['points'] == r['kept'].shape[0] and report['k'] == 4
    assert 0 < report['mean_nearest'] <= report['max_nearest'] < float(r['ext'].max())
    out = str(r['tmp'] / 'cli.ply')
    v, f = meshio.read_ply_mesh(out, dtype=np.float64)
    assert np.array_equal(v, vc) and np.array_equal(f, fc)
    # the command works in the file frame, predict_step in the model frame: the weights differ in their last bits, a colour by at most a level
    diff = np.abs(meshio.read_ply_vertex_colors(out).astype(np.int64) - meshio.read_ply_vertex_colors(r['coloured']).astype(np.int64))
    print('command against predict: {} of {} channels differ, by at most {}'.format(int((diff > 0).sum()), diff.size, int(diff.max())))
    assert diff.max() <= 1
    assert refused.returncode != 0 and os.path.basename(r['plain_scan']) in refused.stderr and not os.path.exists(str(r['tmp'] / 'cli_plain.ply'))
