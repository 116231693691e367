"""GPU tier of the cloud preparation: the kernels of csrc/pps_cloud.hip against the numpy specification
tests/cloud_spec.py, bit for bit, and `pps.py rec` on a raw geo-referenced LAS scan end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_spec as S
from golden_util import GOLDEN, REPO
from grid_spec import wall_clouds
from test_cloud_cpu import ABC, planted, write_las

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _abc():
    from ppsurf_amd import meshio
    return meshio.load_pts(ABC)[:, :3].astype(np.float32)


def _voxel_cases():
    rand, dup = wall_clouds()                                    # exact duplicates and points exactly on cell walls
    # two points of one cell at exactly the same distance from its centre (0.25, 0.25, 0.25), the farther index first in memory order
    tie = np.array([[0.375, 0.25, 0.25], [0.125, 0.25, 0.25], [0.125, 0.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5]], dtype=np.float32)
    return {'random': (rand, [0.25, 0.031, 0.0047, 0.0009]), 'abc': (_abc(), [0.2, 0.02, 0.004]),
            'duplicates_and_walls': (dup, [0.5, 0.25, 0.125, 0.03]), 'tie': (tie, [0.5])}


@pytest.mark.parametrize('name', ['random', 'abc', 'duplicates_and_walls', 'tie'])
def test_voxel_kernel_matches_the_spec_bitwise(name):
    from ppsurf_amd import cloud
    pts, steps = _voxel_cases()[name]
    n = pts.shape[0]
    dev = torch.from_numpy(pts).to(DEV)
    small = 64
    while small <= n:
        small *= 2                                               # the smallest legal table: long probe sequences
    grids = [cloud.VoxelGrid(dev), cloud.VoxelGrid(dev, capacity=small), cloud.VoxelGrid(dev, capacity=8 * small)]
    lo, hi, _ = S.box(pts)
    assert np.array_equal(grids[0].lo, lo) and np.array_equal(grids[0].hi, hi)
    for h in steps:
        h = np.float32(h)
        inv_h = np.float32(1.0) / h
        want = S.voxel_select(pts, lo, hi, h, inv_h)
        for g in grids:
            for _ in range(2):
                got = g.select(h, inv_h).cpu().numpy()
                assert got.dtype == np.int64 and np.array_equal(got, want), (name, float(h), g.capacity)
                assert g.count(h, inv_h) == want.shape[0]
    if name == 'tie':
        assert want.tolist() == [0, 4, 5]


def test_degenerate_clouds():
    from ppsurf_amd import cloud
    one = np.array([[3.0, -2.0, 7.0]])
    idx, rep = cloud.prepare_cloud(one, max_points=1, device=DEV)
    assert idx.tolist() == [0] and rep['kept'] == 1
    same = np.tile(one, (500, 1))
    for kw in ({'max_points': 10}, {'voxel_size': 0.1}):
        idx, rep = cloud.prepare_cloud(same, device=DEV, **kw)
        assert idx.tolist() == [0] and rep['kept_voxel'] == 1
    # all points equal with an explicit h > 0 through the kernel: one cell, index 0
    g = cloud.VoxelGrid(torch.from_numpy(same.astype(np.float32)).to(DEV))
    assert g.select(np.float32(0.1)).tolist() == [0] and g.count(np.float32(0.1)) == 1
    # non-finite rows are dropped before anything else and indices refer to the input's rows
    pts = np.random.RandomState(2).rand(100, 3)
    pts[[3, 50]] = np.nan
    pts[7, 1] = np.inf
    idx, rep = cloud.prepare_cloud(pts, max_points=1000, device=DEV)
    assert rep['nonfinite_dropped'] == 3 and idx.tolist() == [i for i in range(100) if i not in (3, 7, 50)]


def test_too_fine_a_grid_is_an_error_return_and_writes_nothing():
    from ppsurf_amd import cloud
    pts = torch.from_numpy(np.random.RandomState(3).rand(1000, 3).astype(np.float32)).to(DEV)
    g = cloud.VoxelGrid(pts)
    g._scratch(best=True)
    g._table.fill_(5)
    g._count.fill_(77)
    h = np.float32(float(g.ext) / (1 << 21))                     # 2^21 cells along the longest edge
    rc, _ = g.count_rc(h, np.float32(1.0) / h)
    torch.cuda.synchronize()
    assert rc == 1
    assert int(g._count.item()) == 77 and bool((g._table == 5).all())
    with pytest.raises(cloud._lib.PpsError):
        g.select(h)
    assert int(g._count.item()) == 77 and bool((g._table == 5).all())
    h_ok = np.float32(float(g.ext) / 1000.0)
    assert g.count(h_ok) == S.voxel_count(pts.cpu().numpy(), g.lo, g.hi, h_ok, np.float32(1.0) / h_ok)


def test_budget_search_matches_the_spec():
    from ppsurf_amd import cloud
    from test_cloud_cpu import clouds
    pts = clouds(120000, 9)['torus']
    for budget in (2000, 30000):
        want, G, h = S.subsample(pts, budget)
        idx, rep = cloud.prepare_cloud(pts, max_points=budget, device=DEV)
        assert rep['G'] == G and np.float32(rep['h']) == h and np.array_equal(idx, want) and rep['kept'] <= budget


def _outlier_cases():
    rng = np.random.RandomState(22)
    abc = _abc()
    d = rng.randn(30000, 3)
    noisy = (0.4 * d / np.linalg.norm(d, axis=1, keepdims=True) + 0.004 * rng.randn(30000, 3)).astype(np.float32)
    noisy = np.concatenate([noisy, (rng.rand(60, 3) * 4 - 2).astype(np.float32), noisy[:50]])         # stray points and exact duplicates
    return {'abc': abc, 'noisy_sphere': noisy}


@pytest.mark.parametrize('name', ['abc', 'noisy_sphere'])
@pytest.mark.parametrize('k,ratio', [(16, 2.0), (8, 1.0)])
def test_outlier_kernels_match_the_spec_bitwise(name, k, ratio):
    from scipy.spatial import cKDTree
    from ppsurf_amd import cloud, ops
    pts = _outlier_cases()[name]
    dev = torch.from_numpy(pts).to(DEV)
    want_keep, want_m, want_stats = S.outlier_keep(pts, k, ratio)                    # nothing from the device
    _, d2 = ops.KnnBlocks(dev).query(dev, k + 1, return_d2=True)
    m = cloud.mean_knn_distance(d2)
    stats = cloud.outlier_stats(m, ratio)
    keep = cloud.outlier_keep(m, stats).cpu().numpy()
    # second check: the spec fed with the device's d2 -- if this holds and the first does not, the search is off, not the new kernels
    dev_keep, dev_m, dev_stats = S.outlier_keep(pts, k, ratio, d2=d2.cpu().numpy())
    assert np.array_equal(m.cpu().numpy().view(np.uint64), dev_m.view(np.uint64)), 'mean distance kernel differs from the spec on the same d2'
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), np.array(dev_stats).view(np.uint64)), 'statistics differ on the same d2'
    assert np.array_equal(keep, dev_keep)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), S.knn_d2(pts, k + 1).view(np.uint32)), 'the search differs from the spec'
    assert np.array_equal(m.cpu().numpy().view(np.uint64), want_m.view(np.uint64))
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), np.array(want_stats).view(np.uint64))
    assert np.array_equal(keep, want_keep)
    got_keep, _ = cloud.remove_outliers(dev, k, ratio)
    assert np.array_equal(got_keep.cpu().numpy(), want_keep)
    # against the kd-tree route in fp64; first the gap that makes the comparison meaningful, on the spec's values
    gap = np.abs(want_m - want_stats[2]) / want_stats[2]
    print('{} k={} ratio={}: threshold {:.6g}, nearest m_i {:.3g} relative away'.format(name, k, ratio, want_stats[2], gap.min()))
    assert gap.min() > 1e-6
    dist, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=k + 1)
    ref_m = dist[:, 1:].mean(axis=1)
    ref_keep = np.nonzero(ref_m <= ref_m.mean() + ratio * ref_m.std())[0]
    assert np.array_equal(keep, ref_keep)


def test_few_points_keep_everything():
    from ppsurf_amd import cloud
    pts = np.random.RandomState(4).rand(12, 3)
    idx, rep = cloud.prepare_cloud(pts, outlier_k=16, device=DEV)
    assert idx.tolist() == list(range(12)) and rep['removed_outliers'] == 0 and rep['mu'] is None


def test_planted_outliers_are_removed():
    from ppsurf_amd import cloud
    pts, ns = planted()
    idx, rep = cloud.prepare_cloud(pts, outlier_k=16, outlier_ratio=2.0, device=DEV)
    kept = np.zeros(pts.shape[0], dtype=bool)
    kept[idx] = True
    far = np.abs(np.linalg.norm(pts[ns:].astype(np.float64), axis=1) - 0.4) > 1.0
    print(json.dumps(rep), 'far planted', int(far.sum()), 'sphere removed', int((~kept[:ns]).sum()))
    assert not kept[ns:][far].any()
    assert (~kept[:ns]).sum() <= 0.01 * ns
    idx, rep = cloud.prepare_cloud(pts[:ns], outlier_k=16, outlier_ratio=2.0, device=DEV)
    print('clean sphere: removed {:.3%}'.format(1 - idx.shape[0] / ns))
    assert ns - idx.shape[0] <= 0.05 * ns
    # budget and filter together: the filter runs on what the voxel stage kept
    idx, rep = cloud.prepare_cloud(pts, max_points=20000, outlier_k=16, device=DEV)
    assert rep['kept_voxel'] <= 20000 and rep['kept'] == rep['kept_voxel'] - rep['removed_outliers'] == idx.shape[0]
    assert np.all(np.diff(idx) > 0)


def _utm_scan(path):
    """A golden ABC cloud scaled to 40 m and moved to UTM coordinates, plus 50 far outliers, as LAS 1.2 format 1 with millimetre scale."""
    rng = np.random.RandomState(23)
    abc = _abc().astype(np.float64)
    abc = (abc - (abc.min(axis=0) + abc.max(axis=0)) * 0.5) / (abc.max(axis=0) - abc.min(axis=0)).max() * 40.0
    far = (rng.rand(50, 3) * 2 - 1) * 400.0
    far = far[np.argsort(rng.rand(50))]
    local = np.concatenate([abc, far])[rng.permutation(abc.shape[0] + 50)]
    scale, offset = (0.001, 0.001, 0.001), (512345.0, 5403210.0, 310.0)
    write_las(path, np.rint(local / 0.001).astype(np.int32), scale, offset)
    return abc.shape[0]


def _rec_workdir(tmp_path):
    """What `pps.py rec` expects under the working directory: configs/{poco,ppsurf,ppsurf_50nn}.yaml (the reference's own files) and
    models/ppsurf_50nn/version_0/checkpoints/last.ckpt.  The formula-filled state dict of tests/test_gpu_cli.py gives an occupancy without a
    sign change, so the checkpoint is made the other way that file makes one: a short `pps.py fit`, here on the real shapes of abc_mini4 like
    the `trained` fixture of tests/test_gpu_configs.py."""
    from ppsurf_amd import runner
    shutil.copytree(os.path.join(GOLDEN, 'configs'), tmp_path / 'configs')
    shutil.copytree(os.path.join(GOLDEN, 'abc_mini4'), tmp_path / 'abc')
    runner.main(['pps.py', 'fit', '-c', 'configs/poco.yaml', '-c', 'configs/ppsurf.yaml', '-c', 'configs/ppsurf_50nn.yaml',
                 '--data.init_args.in_file', str(tmp_path / 'abc' / 'testset.txt'), '--data.init_args.batch_size', '3',
                 '--data.init_args.manifold_points', '5000', '--trainer.max_epochs', '30', '--trainer.check_val_every_n_epoch', '15',
                 '--trainer.precision', 'bf16-mixed', '--lr_scheduler.init_args.milestones', '[22, 27]'])
    assert (tmp_path / 'models' / 'ppsurf_50nn' / 'version_0' / 'checkpoints' / 'last.ckpt').is_file()


def test_rec_on_a_raw_utm_las_scan(tmp_path, monkeypatch, capsys):
    """(a) `rec` on the LAS file with max_points 5000, outlier_k 16; (b) `python -m ppsurf_amd.cloud` to .npy, then plain `rec` on that."""
    from ppsurf_amd import meshio, runner
    monkeypatch.chdir(tmp_path)
    _rec_workdir(tmp_path)
    las = str(tmp_path / 'scan.las')
    _utm_scan(las)
    small = ['--model.init_args.gen_resolution_global', '33']
    model = runner.main(['pps.py', 'rec', las, str(tmp_path / 'out_a'), '--data.init_args.max_points', '5000', '--data.init_args.outlier_k', '16'] + small)
    assert model.last_prediction is not None, 'no surface came out of the scan'
    mesh_a = tmp_path / 'out_a' / 'scan.las' / 'scan.las.ply'
    assert b'property double x' in open(mesh_a, 'rb').read(200)
    va, fa = meshio.read_ply_mesh(str(mesh_a), dtype=np.float64)

    npy = str(tmp_path / 'prepared.npy')
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'ppsurf_amd.cloud', las, npy, '--max_points', '5000', '--outlier_k', '16'], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=600).stdout
    report = json.loads(out.strip().split('\n')[-1])
    kept = np.load(npy)
    raw = meshio.load_pts(las)
    assert kept.dtype == np.float64 and kept.shape == (report['kept'], 3) and report['kept'] <= 5000 and report['rows'] == raw.shape[0]
    assert report['removed_outliers'] >= 1 and report['kept_voxel'] <= 5000 and report['G'] >= 1
    # the far points are gone.  50 stray points some 200 m apart put mu + 2 sigma at some tens of metres, so one that happens to lie that near
    # the 40 m object may stay (the filter's definition); the kept box is nowhere near the strays' 800 m
    print(json.dumps(report), 'kept box', (kept.max(axis=0) - kept.min(axis=0)).tolist())
    assert (raw.max(axis=0) - raw.min(axis=0)).max() > 700.0 and (kept.max(axis=0) - kept.min(axis=0)).max() < 200.0
    model = runner.main(['pps.py', 'rec', npy, str(tmp_path / 'out_b')] + small)
    assert model.last_prediction is not None
    mesh_b = tmp_path / 'out_b' / 'prepared.npy' / 'prepared.npy.ply'
    vb, fb = meshio.read_ply_mesh(str(mesh_b), dtype=np.float64)
    assert b'property double x' in open(mesh_b, 'rb').read(200)
    assert np.array_equal(fa, fb) and va.shape == vb.shape
    # the same de-normalisation v * scale + centre from the same kept points: at most one float64 rounding apart
    assert np.all(np.abs(va - vb) <= np.spacing(np.abs(vb)))
    lo, hi = kept.min(axis=0), kept.max(axis=0)
    grow = 0.05 * (hi - lo).max()
    print('{} vertices, {} faces; farthest vertex outside the kept box: {:.3g} of its longest edge'.format(
        va.shape[0], fa.shape[0], max(float((lo - va).max()), float((va - hi).max())) / (hi - lo).max()))
    assert np.all(va >= lo - grow) and np.all(va <= hi + grow)
    assert va[:, 0].min() > 5.0e5 and va[:, 1].min() > 5.0e6                       # UTM coordinates, not the unit cube
