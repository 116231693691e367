"""Host side of the mesh evaluation (ppsurf_amd/evaluation.py, meshio.read_ply_mesh): PLY mesh reading, the metric tables, the guards that
act before any device work, and the reference's IoU / F1 query points."""
import glob
import os

import numpy as np
import pytest
import torch

from eval_spec import ply_header_counts
from golden_util import REPO

GT_DIR = os.path.join(REPO, 'tests', 'golden', 'abc_minimal_gt', '03_meshes')
TESTSET = os.path.join(REPO, 'tests', 'golden', 'abc_minimal_testset', 'testset.txt')


def test_read_ply_mesh_on_the_ground_truth_fixtures():
    from ppsurf_amd import meshio
    names = [s.strip() for s in open(TESTSET) if s.strip()]
    files = sorted(glob.glob(os.path.join(GT_DIR, '*.ply')))
    assert sorted(os.path.basename(p)[:-4] for p in files) == sorted(names)
    for path in files:
        counts = ply_header_counts(path)
        verts, faces = meshio.read_ply_mesh(path)
        assert verts.dtype == np.float32 and faces.dtype == np.int32
        assert verts.shape == (counts['vertex'], 3) and faces.shape == (counts['face'], 3)     # trimesh writes triangles only
        assert faces.min() >= 0 and faces.max() < verts.shape[0]
        assert np.isfinite(verts).all() and np.abs(verts).max() < 1.0
        # the same vertices as the point reader, which has been used on trimesh files all along
        assert np.array_equal(verts, meshio.read_ply_vertices(path).astype(np.float32))


def test_read_ply_mesh_round_trip_of_write_ply_mesh(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.default_rng(3)
    verts = rng.standard_normal((57, 3)).astype(np.float32)
    faces = rng.integers(0, 57, size=(101, 3)).astype(np.int32)
    path = str(tmp_path / 'm.ply')
    meshio.write_ply_mesh(path, verts, faces)
    v, f = meshio.read_ply_mesh(path)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)


def test_read_ply_mesh_ascii_polygons_and_extra_properties(tmp_path):
    from ppsurf_amd import meshio
    path = tmp_path / 'quad.ply'
    path.write_text('ply\nformat ascii 1.0\ncomment written by hand\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n'
                    'property uchar red\nelement face 3\nproperty list uchar int vertex_indices\nend_header\n'
                    '0 0 0 255\n1 0 0 0\n1 1 0 7\n0 1 0 1\n0.5 0.5 1 9\n'
                    '4 0 1 2 3\n3 0 1 4\n5 0 1 2 3 4\n')
    v, f = meshio.read_ply_mesh(str(path))
    assert v.shape == (5, 3) and np.array_equal(v[4], np.array([0.5, 0.5, 1.0], dtype=np.float32))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]     # fans from the first corner


def test_read_ply_mesh_binary_quads_uint_counts(tmp_path):
    """list int uint vertex_indices (not trimesh's uchar int) with quads, double vertices and a skipped vertex property."""
    from ppsurf_amd import meshio
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1]], dtype='<f8')
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\nproperty float q\n'
              'element face 2\nproperty list int uint vertex_indices\nend_header\n')
    vrec = np.zeros(5, dtype=[('p', '<f8', (3,)), ('q', '<f4')])
    vrec['p'] = verts
    frec = np.array([(4, (0, 1, 2, 3)), (4, (0, 1, 4, 3))], dtype=[('n', '<i4'), ('v', '<u4', (4,))])
    path = tmp_path / 'b.ply'
    path.write_bytes(header.encode('ascii') + vrec.tobytes() + frec.tobytes())
    v, f = meshio.read_ply_mesh(str(path))
    assert np.array_equal(v, verts.astype(np.float32))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 4, 3]]


def test_read_ply_mesh_rejects_out_of_range_indices(tmp_path):
    from ppsurf_amd import meshio
    path = str(tmp_path / 'bad.ply')
    meshio.write_ply_mesh(path, np.zeros((3, 3), np.float32), np.array([[0, 1, 3]], np.int32))
    with pytest.raises(ValueError):
        meshio.read_ply_mesh(path)


def test_metric_table_layout_and_nan_ignoring_stats(tmp_path):
    from ppsurf_amd import evaluation
    path = str(tmp_path / 'iou.csv')
    evaluation.write_metric_table(path, ['a', 'b', 'c', 'd'], ['ppsurf'], [np.array([0.5, np.nan, 0.75, 1.0])])
    rows = [r.split(',') for r in open(path).read().strip().split('\n')]
    assert rows[0] == ['Shape', 'ppsurf']
    assert [r[0] for r in rows[1:]] == ['a', 'b', 'c', 'd', 'AVERAGE', 'MEDIAN', 'STDEV']
    assert float(rows[1][1]) == 0.5 and rows[2][1] == 'nan'
    vals = np.array([0.5, 0.75, 1.0])
    assert float(rows[5][1]) == pytest.approx(vals.mean(), abs=1e-15)
    assert float(rows[6][1]) == pytest.approx(0.75, abs=1e-15)
    assert float(rows[7][1]) == pytest.approx(vals.std(ddof=1), abs=1e-15)


def test_metric_table_two_columns_all_nan(tmp_path):
    from ppsurf_amd import evaluation
    path = str(tmp_path / 't.csv')
    evaluation.write_metric_table(path, ['a', 'b'], ['x', 'y'], [np.array([np.nan, np.nan]), np.array([1.0, 3.0])])
    rows = [r.split(',') for r in open(path).read().strip().split('\n')]
    assert rows[0] == ['Shape', 'x', 'y'] and len(rows) == 6
    assert rows[3] == ['AVERAGE', 'nan', '2.0'] and rows[4] == ['MEDIAN', 'nan', '2.0'] and rows[5][1] == 'nan'
    assert float(rows[5][2]) == pytest.approx(2 ** 0.5)


def test_single_file_guards_before_device_work(tmp_path, capsys):
    from ppsurf_amd import evaluation
    gt = os.path.join(GT_DIR, os.listdir(GT_DIR)[0])
    missing = str(tmp_path / 'none.ply')
    for metric in ('chamfer', 'iou', 'normals', 'f1'):
        val = evaluation.get_metric_mesh_single_file(gt_mesh_file=gt, mesh_file=missing, num_samples=100, metric=metric)
        assert np.isnan(val)
        assert 'WARNING: mesh missing: {}'.format(missing) in capsys.readouterr().out
    with pytest.raises(FileExistsError):
        evaluation.get_metric_mesh_single_file(gt_mesh_file=missing, mesh_file=gt, num_samples=100, metric='iou')
    from source.base import metrics
    assert np.isnan(metrics.get_metric_mesh_single_file(gt, missing, 100, 'chamfer'))


def test_iou_query_points_are_the_references():
    from ppsurf_amd import evaluation
    for n in (1, 1000, 100000):
        ref = np.random.default_rng(seed=42).random(size=(n, 3)) - 0.5
        assert np.array_equal(evaluation.iou_query_points(n), ref)


def test_host_tensors_are_refused():
    from ppsurf_amd import _lib, evaluation
    v = torch.zeros((3, 3))
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(_lib.PpsError):
        evaluation.mesh_metrics(v, f, v, f, 100)


def test_cli_without_ground_truth_skips(tmp_path, capsys):
    from ppsurf_amd import evaluation
    ds = tmp_path / 'ds'
    ds.mkdir()
    (ds / 'testset.txt').write_text('a\nb\n')
    evaluation.main(['--name', 'n', '--results_dir', str(tmp_path / 'res'), '--data_dir', str(ds), '--testset', 'testset.txt', '--workers', '3'])
    assert 'Warning: {} not found. Skipping evaluation.'.format(os.path.join(str(ds), '03_meshes')) in capsys.readouterr().out
    args = evaluation.parse_arguments([])
    assert (args.name, args.results_dir, args.num_samples, args.workers) == ('ppsurf', 'results', 10000, 8)
