"""GPU tier of make_dataset: the first-hit kernel bit for bit against tests/scan_spec.py, scans and query points against the spec, the
signed distance against the reference's recorded labels, and whole `python -m ppsurf_amd.make_dataset` builds that `pps.py fit` trains on."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from ppsurf_amd import geometry, make_dataset as md, meshio
from tests import eval_spec, scan_spec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GT_DIR = os.path.join(HERE, 'golden', 'abc_minimal_gt', '03_meshes')
GT_MESHES = sorted(glob.glob(os.path.join(GT_DIR, '*.ply')))
TESTSET = os.path.join(HERE, 'golden', 'abc_minimal_testset')
DEV = 'cuda:0'


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _cams(v, settings, name, seed=0):
    v = np.asarray(v, dtype=np.float32)
    return md.scan_cameras(v.min(0).astype(np.float64), v.max(0).astype(np.float64), md.resolve_settings(settings), md.shape_rng(seed, name))


def _nested_spheres():
    vo, fo = eval_spec.icosphere(3, 0.45)
    vi, fi = eval_spec.icosphere(2, 0.2)
    return np.concatenate([vo, vi]).astype(np.float32), np.concatenate([fo, fi + vo.shape[0]]).astype(np.int32), fo.shape[0]


@pytest.mark.parametrize('mesh', ['icosphere', 'abc'])
def test_first_hit_matches_spec_bitwise(mesh):
    if mesh == 'icosphere':
        v, f = eval_spec.icosphere(3, 0.4)
        v, f = v.astype(np.float32), f.astype(np.int32)
    else:
        v, f = meshio.read_ply_mesh(GT_MESHES[1])
    settings = {'num_scans_per_mesh_min': 3, 'num_scans_per_mesh_max': 3}
    cams = _cams(v, settings, mesh)
    orig, dirs = md.scan_rays(_dev(cams), 24)
    o_np, d_np = orig.cpu().numpy(), dirs.cpu().numpy()
    so, sd = scan_spec.rays_spec(cams, 24)
    assert np.array_equal(o_np, so) and np.abs(d_np - sd).max() <= 1.2e-7
    # rays through vertices and edge midpoints of the mesh too (the watertight cases)
    rng = np.random.default_rng(5)
    eye = cams[0, 0:3]
    pick = rng.choice(f.shape[0], 600)
    tgt = np.concatenate([v[f[pick, 0]], (v[f[pick, 0]].astype(np.float64) + v[f[pick, 1]]) * 0.5]).astype(np.float32)
    o_np = np.concatenate([o_np, np.repeat(eye[None], tgt.shape[0], axis=0)])
    d_np = np.concatenate([d_np, (tgt - eye[None]).astype(np.float32)])
    t_ref, f_ref = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), o_np, d_np)
    assert (f_ref >= 0).mean() > 0.2
    _, _, corners = geometry.face_stats(_dev(v), _dev(f))
    for s in (1, 37, None):
        t, face = geometry.first_hit(corners, _dev(o_np), _dev(d_np), slices=s)
        t, face = t.cpu().numpy(), face.cpu().numpy()
        assert np.array_equal(face, f_ref), 'S = {}: {} faces differ'.format(s, int((face != f_ref).sum()))
        assert np.array_equal(t.view(np.uint64), t_ref.view(np.uint64)), 'S = {}: t differs'.format(s)


def test_noise_free_scans_lie_on_the_mesh_and_their_rays():
    v, f = meshio.read_ply_mesh(GT_MESHES[0])
    settings = {'num_scans_per_mesh_min': 4, 'num_scans_per_mesh_max': 4, 'scanner_noise_sigma_max': 0.0, 'scan_resolution': 48}
    cams = _cams(v, settings, 'abc')
    L = float((v.max(0) - v.min(0)).max())
    _, _, corners = geometry.face_stats(_dev(v), _dev(f))
    cams_d = _dev(cams)
    orig, dirs = md.scan_rays(cams_d, 48)
    t, face = geometry.first_hit(corners, orig, dirs)
    pts_all = md.scan_points(corners, cams_d, 48, 0, 0, keep_misses=True)
    pts = md.scan_points(corners, cams_d, 48, 0, 0)
    hit = face >= 0
    assert pts.shape[0] == int(hit.sum()) > 1000
    assert torch.equal(pts, pts_all[hit]) and bool(torch.isnan(pts_all[~hit]).all())
    _, d, _ = geometry.closest_point_on_corners(corners, pts)
    assert float(d.max()) <= 1e-6 * L
    o, dd, p = orig[hit].double(), dirs[hit].double(), pts.double()
    off_ray = torch.linalg.norm(torch.cross(p - o, dd, dim=1), dim=1)
    assert float(off_ray.max()) <= 1e-6 * L
    # the nested sphere is never seen
    vn, fn, n_outer = _nested_spheres()
    pts = md.scan_mesh(_dev(vn), _dev(fn), 'nested', settings, 0)
    r = torch.linalg.norm(pts.double(), dim=1)
    assert pts.shape[0] > 1000 and float(r.min()) > 0.44 and float(r.max()) <= 0.45 + 1e-6


def test_noisy_plane_residuals_and_spec():
    v, f = scan_spec.plane(1.0)
    v, f = v.astype(np.float32), f.astype(np.int32)
    settings = {'num_scans_per_mesh_min': 12, 'num_scans_per_mesh_max': 12, 'scanner_noise_sigma_min': 0.01, 'scanner_noise_sigma_max': 0.01,
                'scan_resolution': 64}
    cams = _cams(v, settings, 'plane', seed=3)
    sigma = 0.01 * 2.0
    assert np.allclose(cams[:, 13], sigma)
    _, _, corners = geometry.face_stats(_dev(v), _dev(f))
    cams_d = _dev(cams)
    orig, dirs = md.scan_rays(cams_d, 64)
    t, face = geometry.first_hit(corners, orig, dirs)
    pts = md.scan_points(corners, cams_d, 64, 3, 77)
    hit = (face >= 0).cpu().numpy()
    assert hit.sum() > 5000
    o, d, tt = orig.cpu().numpy()[hit].astype(np.float64), dirs.cpu().numpy()[hit].astype(np.float64), t.cpu().numpy()[hit]
    res = ((pts.cpu().numpy().astype(np.float64) - o) * d).sum(1) - tt
    assert abs(res.std() / sigma - 1.0) <= 0.05 and abs(res.mean()) <= 0.05 * sigma
    ref = scan_spec.scan_points_spec(orig.cpu().numpy(), dirs.cpu().numpy(), t.cpu().numpy(), face.cpu().numpy(), cams, 64, 3, 77)
    assert ref.shape == pts.shape and np.abs(pts.cpu().numpy() - ref).max() <= 1e-6


def test_query_points_match_spec():
    v, f = meshio.read_ply_mesh(GT_MESHES[2])
    name = os.path.splitext(os.path.basename(GT_MESHES[2]))[0]
    q = md.query_points(_dev(v), _dev(f), name, 2001, 9).cpu().numpy()
    assert q.shape == (2001, 3) and q.dtype == np.float32
    area, normal, corners = geometry.face_stats(_dev(v), _dev(f))
    stream = md.shape_stream(name) << 2
    surf, sface = eval_spec.sample_spec(corners.cpu().numpy(), geometry.area_prefix(area).cpu().numpy(), 1001, 9, stream | 2)
    _, nrm, _ = eval_spec.face_stats_spec(v, f)
    ref = scan_spec.queries_spec(surf, sface, nrm, 1000, 9, stream | 1, md.DEFAULTS['query_near_radius'])
    assert np.array_equal(q[:1000], ref[:1000])
    assert (q[:1000] >= -0.5).all() and (q[:1000] < 0.5).all()
    assert np.abs(q[1000:] - ref[1000:]).max() <= 1e-6
    _, dist, _ = geometry.closest_point_on_corners(corners, _dev(q[1000:]))
    assert float(dist.max()) <= md.DEFAULTS['query_near_radius'] * (1 + 1e-5)


def test_signed_distance_reproduces_recorded_labels():
    worst = 0.0
    for p in GT_MESHES:
        name = os.path.splitext(os.path.basename(p))[0]
        v, f = meshio.read_ply_mesh(p)
        q = np.load(os.path.join(TESTSET, '05_query_pts', name + '.ply.npy'))
        ref = np.load(os.path.join(TESTSET, '05_query_dist', name + '.ply.npy'))
        sd = md.signed_distance(_dev(v), _dev(f), _dev(q))
        assert sd.dtype == torch.float32 and sd.shape == (2000,)
        sd = sd.cpu().numpy()
        assert np.array_equal(np.sign(sd), np.sign(ref))
        worst = max(worst, float(np.abs(sd - ref).max()))
    assert worst <= 2e-5


def test_signed_distance_signs_next_to_the_surface():
    """The labels of queries at the face centroids of icosphere(2, 0.3), offset along the normal by +-1e-2, +-1e-3 and +-1e-4, for both
    windings of the faces: the sign is the fp64 winding number's wherever that is further from +-0.5 than its fp32 error bound
    (eval_spec.winding_spec_bounded) -- by the reference alone at least 99 % of these queries -- and the magnitude is the offset to 1e-6."""
    v, f = eval_spec.icosphere(2, 0.3)
    v = v.astype(np.float32)
    _, nrm, corners = eval_spec.face_stats_spec(v, f)
    centroid = corners.reshape(-1, 3, 3).mean(axis=1)
    offs = np.array([1e-2, -1e-2, 1e-3, -1e-3, 1e-4, -1e-4])
    q = (centroid[None] + offs[:, None, None] * nrm[None]).reshape(-1, 3).astype(np.float32)
    off = np.repeat(offs, f.shape[0])
    w, bound = eval_spec.winding_spec_bounded(v, f, q)
    clear = np.abs(np.abs(w) - 0.5) > bound
    assert clear.mean() >= 0.99
    assert np.array_equal(np.abs(w) > 0.5, off < 0)                           # the normals point outwards: a negative offset is inside
    for faces in (f, f[:, ::-1].copy()):
        sd = md.signed_distance(_dev(v), _dev(faces.astype(np.int32)), _dev(q)).cpu().numpy()
        assert np.array_equal((sd > 0)[clear], (off < 0)[clear])              # positive inside, whichever way the faces wind
        assert np.abs(np.abs(sd.astype(np.float64)) - np.abs(off)).max() <= 1e-6


def _tree(root):
    out = {}
    for dp, _, fns in os.walk(root):
        for fn in fns:
            p = os.path.join(dp, fn)
            out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def test_make_dataset_end_to_end_and_fit(tmp_path, monkeypatch):
    from ppsurf_amd import runner
    from tests.test_gpu_cli import _fit_args
    names = [os.path.splitext(os.path.basename(p))[0] for p in GT_MESHES]
    a, b = tmp_path / 'a', tmp_path / 'b'
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cmd = [sys.executable, '-m', 'ppsurf_amd.make_dataset', '--meshes_dir', GT_DIR, '--out_dir', str(a)]
    r = subprocess.run(['timeout', '-k', '10', '300'] + cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    tree = _tree(str(a))
    expected = {'settings.ini', 'trainset.txt', 'valset.txt', 'testset.txt'}
    for n in names:
        expected |= {os.path.join('03_meshes', n + '.ply'), os.path.join('04_pts_vis', n + '.xyz.ply'),
                     os.path.join('05_query_pts', n + '.ply.npy'), os.path.join('05_query_dist', n + '.ply.npy')}
    assert set(tree) == expected
    test = open(a / 'testset.txt').read().split()
    train = open(a / 'trainset.txt').read().split()
    assert open(a / 'valset.txt').read().split() == test and len(test) == 1 and sorted(train + test) == names
    assert md.read_settings(str(a / 'settings.ini')) == md.DEFAULTS
    counts = {}
    for n in names:
        v, f = meshio.read_ply_mesh(str(a / '03_meshes' / (n + '.ply')))
        ext = v.max(0) - v.min(0)
        assert abs(float(ext.max()) - 1.0 / 1.05) <= 1e-6 and np.abs(v.max(0) + v.min(0)).max() <= 1e-6
        assert f.shape == meshio.read_ply_mesh(os.path.join(GT_DIR, n + '.ply'))[1].shape
        assert eval_spec.ply_header_counts(str(a / '04_pts_vis' / (n + '.xyz.ply'))) == {'vertex': meshio.read_ply_vertices(
            str(a / '04_pts_vis' / (n + '.xyz.ply'))).shape[0], 'face': 0}
        pts = meshio.read_ply_vertices(str(a / '04_pts_vis' / (n + '.xyz.ply')))
        counts[n] = pts.shape[0]
        assert pts.shape[1] == 3 and pts.shape[0] >= 5 * 64 * 64 * 0.1
        q = np.load(str(a / '05_query_pts' / (n + '.ply.npy')))
        d = np.load(str(a / '05_query_dist' / (n + '.ply.npy')))
        assert q.dtype == np.float32 and q.shape == (2000, 3) and d.dtype == np.float32 and d.shape == (2000,)
        assert (np.abs(q[:1000]) <= 0.5).all() and (np.abs(d[1000:]) <= 3 / 128 + 1e-6).all()
        assert 0 < (d > 0).sum() < 2000
    print('points per shape:', counts)
    # the Python API into another directory: byte-identical
    built = md.make_dataset(GT_DIR, str(b))
    assert sorted(built) == names and _tree(str(b)) == tree
    # a rerun does no work
    mtimes = {p: os.stat(os.path.join(str(b), p)).st_mtime_ns for p in tree if not p.endswith(('.txt', '.ini'))}
    assert md.make_dataset(GT_DIR, str(b)) == []
    assert {p: os.stat(os.path.join(str(b), p)).st_mtime_ns for p in mtimes} == mtimes
    # one shape alone: the same files for it
    one = tmp_path / 'one_mesh'
    one.mkdir()
    shutil.copyfile(GT_MESHES[2], str(one / os.path.basename(GT_MESHES[2])))
    md.make_dataset(str(one), str(tmp_path / 'c'))
    tree_c = _tree(str(tmp_path / 'c'))
    for p, data in tree_c.items():
        if names[2] in p:
            assert tree[p] == data, p
    assert open(tmp_path / 'c' / 'trainset.txt').read().split() == [names[2]]
    # pps.py fit trains on it
    monkeypatch.chdir(tmp_path)
    runner.main(_fit_args(tmp_path, str(a / 'testset.txt'), ['--trainer.precision', '32']))
    ckpt = tmp_path / 'models' / 'ppsurf_mini' / 'version_0' / 'checkpoints' / 'last.ckpt'
    state = torch.load(ckpt, map_location='cpu')
    assert state['epoch'] == 1 and state['global_step'] == 2
    assert all(torch.isfinite(v).all() for v in state['state_dict'].values() if torch.is_tensor(v) and v.is_floating_point())


def test_mesh_without_area_names_the_file(tmp_path):
    d = tmp_path / 'm'
    meshio.write_ply_mesh(str(d / 'flat.ply'), np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError, match='flat.ply'):
        md.make_dataset(str(d), str(tmp_path / 'out'), normalize=0)


def test_no_normalize_copies_the_mesh(tmp_path):
    d = tmp_path / 'm'
    d.mkdir()
    shutil.copyfile(GT_MESHES[1], str(d / os.path.basename(GT_MESHES[1])))
    md.make_dataset(str(d), str(tmp_path / 'out'), normalize=0, num_query_pts=100, scan_resolution=16)
    name = os.path.basename(GT_MESHES[1])
    assert open(GT_MESHES[1], 'rb').read() == open(tmp_path / 'out' / '03_meshes' / name, 'rb').read()
    assert np.load(str(tmp_path / 'out' / '05_query_dist' / (os.path.splitext(name)[0] + '.ply.npy'))).shape == (100,)
    assert md.read_settings(str(tmp_path / 'out' / 'settings.ini'))['normalize'] == 0
