"""GPU tier of the comparison: closest point and rasteriser against the numpy restatements of tests/vis_spec.py, determinism, and the
whole `python -m ppsurf_amd.comparison` run on a results tree built from the fixtures."""
import glob
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from ppsurf_amd import geometry, meshio, visualization
from ppsurf_amd.evaluation import write_metric_table
from tests import eval_spec, vis_spec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GT_DIR = os.path.join(HERE, 'golden', 'abc_minimal_gt', '03_meshes')
PTS_DIR = os.path.join(HERE, 'golden', 'abc_minimal_testset', '04_pts_vis')
GT_MESHES = sorted(glob.glob(os.path.join(GT_DIR, '*.ply')))
DEV = 'cuda:0'


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _queries(v, f, seed):
    """20k uniform points in the padded box and 20k points within 1e-3 of the surface."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0) - 0.1, v.max(0) + 0.1
    box = rng.uniform(lo, hi, size=(20000, 3))
    tri = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    fi = rng.choice(f.shape[0], size=20000, p=area / area.sum())
    r1, r2 = rng.random(20000), rng.random(20000)
    fold = r1 + r2 > 1
    r1, r2 = np.where(fold, 1 - r1, r1), np.where(fold, 1 - r2, r2)
    on = tri[fi, 0] + r1[:, None] * (tri[fi, 1] - tri[fi, 0]) + r2[:, None] * (tri[fi, 2] - tri[fi, 0])
    off = rng.normal(size=(20000, 3))
    off *= (rng.random(20000) * 1e-3 / np.linalg.norm(off, axis=1))[:, None]
    return np.concatenate([box, on + off]).astype(np.float32)


@pytest.mark.parametrize('k', range(3))
def test_closest_point_matches_spec(k):
    v, f = meshio.read_ply_mesh(GT_MESHES[k])
    q = _queries(v, f, k)
    pt, d, face = geometry.closest_point_on_mesh(_dev(v), _dev(f), _dev(q))
    pt, d, face = pt.cpu().numpy(), d.cpu().numpy(), face.cpu().numpy()
    sd, sf, sp, s2 = vis_spec.closest_point_spec(v, f, q)
    err = np.abs(d - sd) - (1e-6 + 1e-6 * sd)
    assert err.max() <= 0, 'distance off by {} at query {}'.format(np.abs(d - sd).max(), int(err.argmax()))
    clear = (s2 - sd) > 1e-6
    assert np.array_equal(face[clear], sf[clear]), '{} face ids differ'.format(int((face[clear] != sf[clear]).sum()))
    assert np.abs(pt[clear] - sp[clear]).max() <= 1e-5
    # every returned point lies on its returned face at the returned distance
    tri = v.astype(np.float64)[f[face]]
    qq, dd = vis_spec.closest_on_triangles(q.astype(np.float64), tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.abs(np.sqrt(dd) - d).max() <= 1e-6


def test_closest_point_icospheres():
    vi, _ = eval_spec.icosphere(3, 0.30)
    vo, fo = eval_spec.icosphere(3, 0.35)
    _, d, _ = geometry.closest_point_on_mesh(_dev(vo, torch.float32), _dev(fo, torch.int32), _dev(vi, torch.float32))
    edge = max(np.linalg.norm(vo[fo[:, 0]] - vo[fo[:, 1]], axis=1).max(), np.linalg.norm(vo[fo[:, 1]] - vo[fo[:, 2]], axis=1).max())
    # the flat faces of the outer sphere lie inside it by at most the sag of the circumscribed circle of a face
    sag = 0.35 - math.sqrt(0.35 ** 2 - (edge / math.sqrt(3.0)) ** 2)
    assert np.abs(d.cpu().numpy() - 0.05).max() <= sag + 1e-6


def test_closest_point_deterministic_and_slice_independent():
    v, f = meshio.read_ply_mesh(GT_MESHES[0])
    q = _dev(_queries(v, f, 7))
    vt, ft = _dev(v), _dev(f)
    a = geometry.closest_point_on_mesh(vt, ft, q)
    b = geometry.closest_point_on_mesh(vt, ft, q)
    one = geometry.closest_point_on_mesh(vt, ft, q, slices=1)
    odd = geometry.closest_point_on_mesh(vt, ft, q, slices=37)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for other in (one, odd):
        assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2]) and torch.equal(a[0], other[0])


def test_closest_point_degenerate_faces():
    # a zero-area face (collinear corners) and a collapsed one next to a regular face: no NaN, the segment distance
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 0.5, 0.5], [5, 5, 5], [6, 5, 5], [5, 6, 5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [3, 3, 3], [4, 5, 6]], dtype=np.int32)
    q = np.array([[1.5, 1.0, 0.0], [0.5, 0.5, 0.6], [-1, 0, 0]], dtype=np.float32)
    _, d, face = geometry.closest_point_on_mesh(_dev(v), _dev(f), _dev(q))
    d, face = d.cpu().numpy(), face.cpu().numpy()
    assert np.all(np.isfinite(d))
    assert np.allclose(d, [1.0, 0.1, 1.0], atol=1e-6) and face.tolist() == [0, 1, 0]


def _cam_for(v, size):
    return visualization.camera_array(*visualization.camera(v, size))


def _mesh_cases():
    v, f = meshio.read_ply_mesh(GT_MESHES[1])
    vi, fi = eval_spec.icosphere(3, 0.45)
    return [(v, f), (vi.astype(np.float32), fi.astype(np.int32))]


@pytest.mark.parametrize('k', range(2))
def test_raster_matches_spec(k):
    v, f = _mesh_cases()[k]
    size = 128
    cam = _cam_for(v, size)
    keys = visualization.raster_faces(_dev(v), _dev(f), cam, size, size).cpu().numpy()
    ids, depth = vis_spec.decode_keys(keys)
    sid, sdepth, amb = vis_spec.raster_spec(v, f, cam, size, size)
    covered = sid >= 0
    assert covered.sum() > 0.02 * size * size
    diff = (ids != sid) & ~amb
    assert not diff.any(), '{} pixels differ away from edges'.format(int(diff.sum()))
    assert ((ids != sid) & amb).sum() <= 0.005 * covered.sum()
    same = (ids == sid) & covered
    assert np.all(np.abs(depth[same] - sdepth[same]) <= 1e-6 * np.abs(sdepth[same]))


def test_screen_filling_quad_covers_every_pixel_once():
    size = 64
    # camera at the origin looking down -z; a quad at depth 1 exactly filling the view: x, y in [-1, 1] with f = size / 2
    cam = np.zeros(16, dtype=np.float32)
    cam[0:9] = np.eye(3, dtype=np.float32).reshape(9)
    cam[12] = size / 2
    v = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1]], dtype=np.float32)
    tris = [np.array([[0, 1, 2]], dtype=np.int32), np.array([[0, 2, 3]], dtype=np.int32)]
    masks = [visualization.raster_faces(_dev(v), _dev(t), cam, size, size).cpu().numpy() != -1 for t in tris]
    assert not (masks[0] & masks[1]).any(), 'pixels covered twice'
    assert (masks[0] | masks[1]).all(), 'pixels left uncovered'
    both = visualization.raster_faces(_dev(v), _dev(np.concatenate(tris)), cam, size, size).cpu().numpy()
    ids, depth = vis_spec.decode_keys(both)
    assert np.array_equal(ids == 0, masks[0]) and np.all(depth == 1.0)
    # the diagonal passes through pixel centres: the top-left rule gives every one of them to exactly one triangle
    assert masks[0].sum() + masks[1].sum() == size * size


def test_point_splats_cover_disc():
    size = 128
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.4, 0.4, size=(50, 3)).astype(np.float32)
    cam = _cam_for(pts, size)
    r = 2.0
    keys = visualization.raster_points(_dev(pts), cam, size, size, r).cpu().numpy()
    cov = vis_spec.points_spec(pts, cam, size, size, r)
    assert np.array_equal(keys != -1, cov)
    ids, _ = vis_spec.decode_keys(keys)
    assert ids.max() < 50


def test_renders_reproducible_and_shaded():
    v, f = _mesh_cases()[0]
    a = visualization.render(v, f)
    b = visualization.render(v, f)
    assert a.shape == (1024, 1024, 3) and np.array_equal(a, b)
    fg = np.any(a != 255, axis=2)
    assert fg[400:624, 400:624].any()
    vals = a[fg][:, 0]
    assert vals.min() >= int(102 * 0.3) - 1 and vals.max() <= 102 and np.all(a[fg][:, 0] == a[fg][:, 1])
    col = np.zeros((v.shape[0], 3), dtype=np.uint8)
    col[:, 2] = 200
    c = visualization.render(v, f, col)
    assert np.array_equal(np.any(c != 255, axis=2), fg) and np.all(c[fg][:, 0] == 0)
    pts = meshio.read_ply_vertices(sorted(glob.glob(os.path.join(PTS_DIR, '*.ply')))[1])[:, :3]
    p1, p2 = visualization.render(pts, None), visualization.render(pts, None)
    assert np.array_equal(p1, p2) and np.any(p1 != 255)


def _index_of_color(colors):
    """Smallest parula index of every colour row (-1 when the colour is not in the table)."""
    table = visualization.PARULA.astype(np.int64)
    code = (table[:, 0] << 16) | (table[:, 1] << 8) | table[:, 2]
    first = {}
    for i, c in enumerate(code.tolist()):
        first.setdefault(c, i)
    cc = (colors[:, 0].astype(np.int64) << 16) | (colors[:, 1].astype(np.int64) << 8) | colors[:, 2]
    return np.array([first.get(c, -1) for c in cc.tolist()])


def test_comparison_end_to_end(tmp_path):
    data = tmp_path / 'data'
    shapes = [os.path.basename(p)[:-4] for p in GT_MESHES]
    shutil.copytree(GT_DIR, data / '03_meshes')
    shutil.copytree(PTS_DIR, data / '04_pts_vis')
    (data / 'testset.txt').write_text('\n'.join(shapes) + '\n')
    res = tmp_path / 'results'
    paths = {m: res / m / 'data' for m in ('same', 'shifted', 'gone')}
    for s, p in zip(shapes, GT_MESHES):
        v, f = meshio.read_ply_mesh(p)
        meshio.write_ply_mesh(str(paths['same'] / 'meshes' / (s + '.xyz.ply')), v, f)
        meshio.write_ply_mesh(str(paths['shifted'] / 'meshes' / (s + '.xyz.ply')), v + np.array([0.02, 0, 0], dtype=np.float32), f)
    for m, vals in (('same', (0.0, 1.0, 1.0, 0.0)), ('shifted', (0.02, 0.8, 0.9, 1.0))):
        for metric, val in zip(('chamfer_distance', 'iou', 'f1', 'normal_error'), vals):
            write_metric_table(str(paths[m] / (metric + '.csv')), shapes, [m], [np.full(len(shapes), val)])
    comp_dir = tmp_path / 'comp'
    cmd = [sys.executable, '-m', 'ppsurf_amd.comparison', '--comp_name', 'data', '--comp_dir', str(comp_dir), '--data_dir', str(data),
           '--testset', 'testset.txt', '--result_headers', 'same', 'shifted', 'gone', '--result_paths'] + [str(paths[m]) for m in ('same', 'shifted', 'gone')]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run(['timeout', '-k', '10', '300'] + cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    comp = comp_dir / 'data'
    for name in ('chamfer_distance', 'iou', 'normal_error', 'f1', 'comp_mean'):
        assert (comp / (name + '.csv')).is_file()
    outputs = []
    for m in ('same', 'shifted'):
        for s in shapes:
            p = comp / m / 'mesh_cd_vis' / (s + '.ply')
            outputs.append(p)
            v, _ = meshio.read_ply_mesh(str(p))
            assert v.shape[0] >= 10000
            idx = _index_of_color(meshio.read_ply_vertex_colors(str(p)))
            assert np.all(idx >= 0)
            if m == 'same':
                assert np.all(idx == 0)
            else:
                assert idx.max() > 0 and idx.max() <= int(0.4 * 255) + 1
    assert not (comp / 'gone').exists() or not any((comp / 'gone').rglob('*.ply'))
    pngs = sorted(comp.rglob('*.png'))
    assert len(pngs) == 3 + 3 + 2 * 3 + 2 * 3
    for p in pngs:
        img = visualization.read_png(str(p))
        assert img.shape == (1024, 1024, 3)
        assert np.any(img[256:768, 256:768] != 255), p
    assert all((comp / 'pc_rend' / (s + '.png')).is_file() for s in shapes)
    outputs += pngs
    html = (comp / 'comp_html.html').read_text()
    import re
    for src in re.findall(r'src="([^"]+)"', html):
        assert (comp / src).is_file()
    body = html.split('<tbody>')[1]
    assert body.count('<tr>') == 3 and body.count('missing') == 3
    mtimes = {p: os.stat(p).st_mtime_ns for p in outputs}
    r2 = subprocess.run(['timeout', '-k', '10', '300'] + cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r2.returncode == 0, r2.stdout[-4000:]
    assert {p: os.stat(p).st_mtime_ns for p in outputs} == mtimes
