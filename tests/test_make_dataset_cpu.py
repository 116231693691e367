"""CPU tier of make_dataset: the signed-distance convention against the reference's recorded labels, the first-hit rules of
tests/scan_spec.py on meshes with known answers, and the host logic (split, settings, per-shape seeds, ABI)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from ppsurf_amd import _lib, geometry, make_dataset as md, meshio
from tests import eval_spec, scan_spec, vis_spec

HERE = os.path.dirname(os.path.abspath(__file__))
GT_MESHES = sorted(glob.glob(os.path.join(HERE, 'golden', 'abc_minimal_gt', '03_meshes', '*.ply')))
TESTSET = os.path.join(HERE, 'golden', 'abc_minimal_testset')


@pytest.mark.parametrize('k', range(3))
def test_numpy_signed_distance_reproduces_recorded_labels(k):
    """|05_query_dist| is the exact distance to 03_meshes, positive inside (|winding number| > 0.5)."""
    name = os.path.splitext(os.path.basename(GT_MESHES[k]))[0]
    v, f = meshio.read_ply_mesh(GT_MESHES[k])
    q = np.load(os.path.join(TESTSET, '05_query_pts', name + '.ply.npy'))
    ref = np.load(os.path.join(TESTSET, '05_query_dist', name + '.ply.npy'))
    assert q.shape == (2000, 3) and q.dtype == np.float32 and ref.shape == (2000,) and ref.dtype == np.float32
    d = vis_spec.closest_point_spec(v, f, q)[0]
    w = eval_spec.winding_spec(v, f, q)
    sd = np.where(np.abs(w) > 0.5, d, -d)
    assert np.abs(sd - ref).max() <= 2e-5
    assert np.array_equal(np.sign(sd), np.sign(ref))


def test_first_hit_analytic_plane():
    v, f = scan_spec.plane(2.0, 0.25)
    rng = np.random.default_rng(0)
    xy = rng.uniform(-1.5, 1.5, size=(500, 2))
    h = rng.uniform(0.5, 3.0, size=500)
    orig = np.concatenate([xy, (0.25 + h)[:, None]], axis=1).astype(np.float32)
    up = orig.copy()
    up[:, 2] = 0.25 - h.astype(np.float32)                     # from below: both faces are hit
    dirs = np.tile(np.array([[0, 0, -1]], dtype=np.float32), (500, 1))
    t, face = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), orig, dirs)
    assert (face >= 0).all()
    assert np.abs(t - (orig[:, 2].astype(np.float64) - np.float32(0.25))).max() <= 1e-12
    t2, face2 = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), up, -dirs)
    assert (face2 >= 0).all() and np.abs(t2 - (np.float32(0.25) - up[:, 2].astype(np.float64))).max() <= 1e-12
    # pointing away, or outside the square: misses
    t3, face3 = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), orig, -dirs)
    assert (face3 == -1).all() and (t3 == -1).all()
    far = orig.copy()
    far[:, 0] += 10.0
    assert (scan_spec.first_hit_spec(scan_spec.corners_of(v, f), far, dirs)[1] == -1).all()


def test_first_hit_analytic_icosphere():
    v, f = eval_spec.icosphere(2, 0.4)
    rng = np.random.default_rng(1)
    d = rng.normal(size=(400, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    orig = np.zeros((400, 3), dtype=np.float32)
    t, face = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), orig, d)
    assert (face >= 0).all()
    tri = v.astype(np.float32).astype(np.float64)[f[face]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    t_plane = (n * tri[:, 0]).sum(1) / (n * d.astype(np.float64)).sum(1)
    assert np.abs(t - t_plane).max() <= 1e-12
    assert (t <= 0.4 + 1e-6).all() and (t >= 0.4 * 0.97).all()


def test_first_hit_is_watertight_at_vertices_and_edges():
    v, f = eval_spec.icosphere(2, 0.4)
    v32 = v.astype(np.float32)
    edges = {tuple(sorted(e)) for t in f.tolist() for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    mids = np.array([(v32[a].astype(np.float64) + v32[b]) * 0.5 for a, b in sorted(edges)], dtype=np.float32)
    dirs = np.concatenate([v32, mids])
    t, face = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), np.zeros_like(dirs), dirs)
    assert (face >= 0).all(), '{} rays through a vertex or an edge leak'.format(int((face < 0).sum()))
    assert np.abs(t[:v.shape[0]] - 1.0).max() <= 1e-6                 # a vertex is hit at t = 1 (dirs are the vertices themselves)


def test_nested_sphere_is_hidden():
    vo, fo = eval_spec.icosphere(2, 0.45)
    vi, fi = eval_spec.icosphere(1, 0.2)
    v = np.concatenate([vo, vi])
    f = np.concatenate([fo, fi + vo.shape[0]])
    rng = np.random.default_rng(2)
    u = rng.normal(size=(600, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    orig = (1.5 * u).astype(np.float32)
    target = rng.uniform(-0.1, 0.1, size=(600, 3))
    dirs = (target - orig).astype(np.float32)
    t, face = scan_spec.first_hit_spec(scan_spec.corners_of(v, f), orig, dirs)
    assert (face >= 0).all() and (face < fo.shape[0]).all()


def test_ties_go_to_the_lowest_face():
    v, f = scan_spec.plane(1.0)
    f2 = np.concatenate([f, f[::-1]])                          # the same two triangles again
    orig = np.array([[0.3, -0.2, 1.0], [-0.4, 0.5, 1.0]], dtype=np.float32)
    dirs = np.array([[0, 0, -1], [0, 0, -1]], dtype=np.float32)
    t, face = scan_spec.first_hit_spec(scan_spec.corners_of(v, f2), orig, dirs)
    assert face.tolist() == [0, 1] and t.tolist() == [1.0, 1.0]


def test_split_rules():
    names = ['s{:02d}'.format(i) for i in range(10)]
    train, test = md.split_names(names, 0.3, 42)
    assert len(test) == 3 and len(train) == 7 and sorted(train + test) == names and not set(train) & set(test)
    assert md.split_names(names[::-1], 0.3, 42) == (train, test)                # order of the input does not matter
    assert md.split_names(names, 0.3, 42) == (train, test)
    assert md.split_names(names, 0.3, 7) != (train, test)
    assert md.split_names(['only'], 0.3, 0) == (['only'], ['only'])
    tr, te = md.split_names(names[:3], 0.3, 0)
    assert len(te) == 1 and len(tr) == 2
    tr, te = md.split_names(names[:2], 1.0, 0)
    assert len(te) == 1 and len(tr) == 1


def test_settings_round_trip(tmp_path):
    s = md.resolve_settings(None, scan_resolution=32, seed=5, scanner_noise_sigma_max=0.02, normalize=0)
    p = str(tmp_path / 'settings.ini')
    md.write_settings(p, s)
    assert md.read_settings(p) == s
    assert open(p).read().startswith('[general]')
    # the reference's own settings.ini: its scanner keys are honoured, the others ignored
    (tmp_path / 'ref.ini').write_text('[general]\nonly_for_evaluation = 0\ngrid_resolution = 256\nepsilon = 5\nnum_scans_per_mesh_min = 5\n'
                                      'num_scans_per_mesh_max = 30\nscanner_noise_sigma_min = 0.0\nscanner_noise_sigma_max = 0.05')
    r = md.read_settings(str(tmp_path / 'ref.ini'))
    assert r == md.DEFAULTS
    assert md.resolve_settings(r, scan_resolution=16)['scan_resolution'] == 16
    with pytest.raises(KeyError):
        md.resolve_settings({'grid_resolution': 3})
    with pytest.raises(ValueError):
        md.resolve_settings(None, num_scans_per_mesh_min=6, num_scans_per_mesh_max=5)


def test_per_shape_generator_does_not_depend_on_order():
    s = dict(md.DEFAULTS)
    a = md.scan_cameras([-0.5] * 3, [0.5] * 3, s, md.shape_rng(3, 'shape_a'))
    md.scan_cameras([-0.5] * 3, [0.5] * 3, s, md.shape_rng(3, 'shape_b'))
    a2 = md.scan_cameras([-0.5] * 3, [0.5] * 3, s, md.shape_rng(3, 'shape_a'))
    assert np.array_equal(a, a2)
    assert not np.array_equal(md.scan_cameras([-0.5] * 3, [0.5] * 3, s, md.shape_rng(4, 'shape_a')), a)
    assert md.shape_stream('shape_a') != md.shape_stream('shape_b')
    assert 5 <= a.shape[0] <= 30 and a.dtype == np.float32 and a.shape[1] == 16


def test_scan_cameras_model():
    s = md.resolve_settings(None, num_scans_per_mesh_min=40, num_scans_per_mesh_max=40, scanner_noise_sigma_min=0.01,
                            scanner_noise_sigma_max=0.03)
    lo, hi = np.array([-0.2, -0.4, -0.1]), np.array([0.3, 0.4, 0.2])
    cams = md.scan_cameras(lo, hi, s, md.shape_rng(0, 'x')).astype(np.float64)
    c, rho = (lo + hi) / 2, 0.5 * np.linalg.norm(hi - lo)
    assert cams.shape == (40, 16)
    assert np.abs(np.linalg.norm(cams[:, 0:3] - c, axis=1) - 3 * rho).max() <= 1e-6
    fwd = cams[:, 9:12]
    assert np.abs((c - cams[:, 0:3]) / (3 * rho) - fwd).max() <= 1e-6       # looks at the centre
    for a, b in ((3, 6), (6, 9), (3, 9)):
        assert np.abs((cams[:, a:a + 3] * cams[:, b:b + 3]).sum(1)).max() <= 1e-6
    assert np.abs(cams[:, 12] - rho / np.sqrt(8.0 * rho * rho)).max() <= 1e-6
    L = (hi - lo).max()
    assert (cams[:, 13] >= 0.01 * L - 1e-7).all() and (cams[:, 13] <= 0.03 * L + 1e-7).all()


def test_rays_spec_cover_the_bounding_sphere():
    s = md.resolve_settings(None)
    cams = md.scan_cameras([-0.5] * 3, [0.5] * 3, s, md.shape_rng(0, 'y'))
    orig, dirs = scan_spec.rays_spec(cams, 8)
    assert orig.shape == (cams.shape[0] * 64, 3) and dirs.dtype == np.float32
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1).max() <= 1e-6
    # the bounding sphere just fits: rays inside the image's inscribed circle pass the centre within rho, the outermost of them near rho
    c, rho = np.zeros(3), 0.5 * np.sqrt(3.0)
    o, d = orig[:64].astype(np.float64), dirs[:64].astype(np.float64)
    miss = np.linalg.norm(np.cross(c - o, d), axis=1)
    p = np.arange(64)
    x, y = (2 * (p % 8) + 1) / 8 - 1, 1 - (2 * (p // 8) + 1) / 8
    disc = x * x + y * y <= 1
    assert miss[disc].max() <= rho and miss[disc].max() >= 0.85 * rho and miss[~disc].min() > 0.85 * rho


def test_device_functions_refuse_cpu_tensors():
    v, f = eval_spec.icosphere(1, 0.4)
    vt, ft = torch.from_numpy(v).float(), torch.from_numpy(f).int()
    with pytest.raises(_lib.PpsError):
        md.scan_mesh(vt, ft, 'x')
    with pytest.raises(_lib.PpsError):
        md.query_points(vt, ft, 'x', 10)
    with pytest.raises(_lib.PpsError):
        md.signed_distance(vt, ft, torch.zeros(4, 3))
    with pytest.raises(_lib.PpsError):
        geometry.first_hit(torch.zeros(1, 9), torch.zeros(1, 3), torch.ones(1, 3))


def test_scan_abi_declared():
    header = open(os.path.join(HERE, '..', 'include', 'ppsurf_amd.h')).read()
    declared = set(re.findall(r'^\w[\w\s\*]*?\b(pps_scan_\w+)\(', header, re.M))
    expected = {'pps_scan_hit_slices', 'pps_scan_first_hit', 'pps_scan_rays', 'pps_scan_points', 'pps_scan_queries'}
    assert declared == expected
    assert expected <= set(_lib.SIGNATURES)
    lib = _lib.lib()
    for name in expected:
        assert hasattr(lib, name)
    assert lib.pps_abi_version() == 2
    assert lib.pps_scan_hit_slices(0, 10) == -1 and lib.pps_scan_hit_slices(1000, 10) == 1
    s = lib.pps_scan_hit_slices(122880, 20480)
    assert 1 <= s <= 20480 // 64 + 1
