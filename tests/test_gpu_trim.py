"""GPU tier of the trim by support: the cell lists and the support kernel of csrc/pps_trim.hip against the brute-force
numpy specification tests/trim_spec.py, byte for byte; invariance under the grid and the table; exact thresholds; shapes that stress the
cell range; the argument rules of the C entry; the spacing; `trim_mesh`; `pps.py rec --model.init_args.gen_trim_factor` and
`python -m ppsurf_amd.trim` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_spec
import trim_spec as S
from golden_util import REPO
from test_cloud_cpu import ABC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RADII = (0.02, 0.1, 0.5)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def gpu_support(cloud, verts, faces, r, **kw):
    from ppsurf_amd import trim
    out = trim.face_support(dev(np.asarray(cloud, dtype=np.float32)), dev(np.asarray(verts, dtype=np.float32)), dev(np.asarray(faces, dtype=np.int64)), r, **kw)
    assert out.dtype == torch.bool and tuple(out.shape) == (np.asarray(faces).shape[0],)
    return out.cpu().numpy()


@pytest.fixture(scope='module')
def scene():
    """3 000 noisy points of the upper half of the unit sphere, the 1 280 faces of the icosphere and ONE brute-force pass (the smallest d2 of
    every face) shared by every case: a prefix of the faces has a prefix of the distances, and every radius thresholds the same distances."""
    rng = np.random.RandomState(51)
    d = rng.randn(3000, 3)
    d[:, 2] = np.abs(d[:, 2])
    cloud = (d / np.linalg.norm(d, axis=1, keepdims=True) + 0.005 * rng.randn(3000, 3)).astype(np.float32)
    verts, faces = eval_spec.icosphere(3)
    verts = verts.astype(np.float32)
    assert faces.shape == (1280, 3)
    d2 = S.face_d2(cloud, verts, faces)
    for r in RADII:
        kept = int((d2 <= np.float64(r) * np.float64(r)).sum())
        assert 0 < kept < 1280, (r, kept)                             # the spec keeps some but not all faces at every radius
    for a in (cloud, verts, faces, d2):
        a.setflags(write=False)
    return {'cloud': cloud, 'verts': verts, 'faces': faces, 'd2': d2}


@pytest.mark.parametrize('r', RADII)
@pytest.mark.parametrize('nf', [1, 63, 64, 65, 257, 1280])
def test_kernel_matches_the_spec_bytewise(scene, nf, r):
    want = scene['d2'][:nf] <= np.float64(r) * np.float64(r)
    first = gpu_support(scene['cloud'], scene['verts'], scene['faces'][:nf], r)
    again = gpu_support(scene['cloud'], scene['verts'], scene['faces'][:nf], r)
    assert np.array_equal(first, want), 'faces {} differ'.format(np.nonzero(first != want)[0][:10])
    assert first.tobytes() == again.tobytes()


def test_result_does_not_depend_on_grid_or_table(scene):
    r = 0.1
    want = scene['d2'] <= np.float64(r) * np.float64(r)
    ext = float((scene['cloud'].max(axis=0) - scene['cloud'].min(axis=0)).max())
    for cell in (r, 2 * r, 7 * r, ext):
        for capacity in (4096, 1 << 16):
            got = gpu_support(scene['cloud'], scene['verts'], scene['faces'], r, cell=cell, capacity=capacity)
            assert np.array_equal(got, want), (cell, capacity)


@pytest.mark.parametrize('name,tri,p,dist', S.threshold_cases(), ids=[c[0] for c in S.threshold_cases()])
def test_exact_thresholds(name, tri, p, dist):
    face = np.array([[0, 1, 2]], dtype=np.int64)
    below = float(np.nextafter(np.float64(dist), 0.0))
    far = np.array([[40, 40, 40], [-30, 8, 2]], dtype=np.float32)
    for cloud in (p[None], np.concatenate([far, p[None]])):
        assert gpu_support(cloud, tri, face, dist).tolist() == [True] == S.face_support_spec(cloud, tri, face, dist).tolist()
        assert gpu_support(cloud, tri, face, below).tolist() == [False] == S.face_support_spec(cloud, tri, face, below).tolist()


def _same_as_spec(cloud, verts, faces, r, want=None):
    spec = S.face_support_spec(cloud, verts, faces, r)
    if want is not None:
        assert spec.tolist() == want
    got = gpu_support(cloud, verts, faces, r)
    assert np.array_equal(got, spec), (got.tolist()[:16], spec.tolist()[:16])


def test_shapes_that_stress_the_cell_range():
    rng = np.random.RandomState(52)
    # two triangles over a 10 x 10 square, 500 points near one corner, tiny r: 100 x 100 x 10 cells in the range against 500 points
    square = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 10, 0]], dtype=np.float32)
    corner = np.concatenate([rng.rand(500, 2) * 0.01, (rng.rand(500, 1) - 0.5) * 1e-3], axis=1).astype(np.float32)
    _same_as_spec(corner, square, np.array([[0, 1, 2], [1, 3, 2]]), 1e-4, want=[True, False])
    # a face far outside the cloud's box, faces whose box holds the whole cloud (one through it, one tilted past it), one next to it
    cloud = (rng.rand(700, 3) * 2.0 - 1.0).astype(np.float32)
    verts = np.array([[1e6, 1e6, 1e6], [1e6 + 1, 1e6, 1e6], [1e6, 1e6 + 1, 1e6],
                      [-300, -300, 0.5], [300, -300, 0.5], [0, 300, 0.5],
                      [-300, -300, -400], [300, -300, -400], [0, 300, 600],
                      [1.5, 0, 0], [2.5, 0, 0], [1.5, 1, 0]], dtype=np.float32)
    _same_as_spec(cloud, verts, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]), 0.05, want=[False, True, False, False])
    _same_as_spec(cloud, verts, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]), 0.75)
    # 2 000 copies of one point: one cell holds them all
    copies = np.tile(np.array([[0.25, 0.5, 0.125]], dtype=np.float32), (2000, 1))
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], dtype=np.float32)
    _same_as_spec(copies, tri, np.array([[0, 1, 2], [3, 4, 5]]), 0.125, want=[True, False])
    _same_as_spec(copies, tri, np.array([[0, 1, 2], [3, 4, 5]]), float(np.nextafter(0.125, 0.0)), want=[False, False])
    # n = 1
    _same_as_spec(copies[:1], tri, np.array([[0, 1, 2], [3, 4, 5]]), 0.125, want=[True, False])
    _same_as_spec(copies[:1], tri, np.array([[0, 1, 2], [3, 4, 5]]), 2.0, want=[True, True])
    # indices outside [0, nv) are unsupported however large r is, and never read through; zero-area faces are their longest edge
    nv = tri.shape[0]
    faces = np.array([[0, 1, 2], [-1, 1, 2], [0, nv, 2], [0, 1, 1 << 40], [-(1 << 40), 1, 2], [0, 0, 0], [0, 1, 1], [3, 3, 5], [2, 1, 0]], dtype=np.int64)
    _same_as_spec(cloud, tri, faces, 100.0, want=[True, False, False, False, False, True, True, True, True])
    _same_as_spec(cloud, tri, faces, 0.05)
    line = np.array([[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [0.25, 0.25, 0.25]], dtype=np.float32)
    _same_as_spec(cloud, line, np.array([[0, 1, 2], [3, 3, 3], [0, 2, 1]]), 0.06)
    # a non-finite corner
    bad = np.concatenate([tri, np.array([[np.nan, 0, 0], [np.inf, 0, 0]], dtype=np.float32)])
    _same_as_spec(cloud, bad, np.array([[0, 1, 6], [0, 7, 2], [0, 1, 2]]), 10.0, want=[False, False, True])


def test_bad_arguments_are_an_error_return_and_write_nothing(scene):
    from ppsurf_amd import _lib, trim
    r = 0.1
    cloud, verts, faces = dev(scene['cloud']), dev(scene['verts']), dev(scene['faces'])
    n, nv, nf = cloud.shape[0], verts.shape[0], faces.shape[0]
    g = trim.SupportGrid(cloud)
    g.build(g.edge_for(r))
    out = torch.full((nf,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(verts=verts, nv=nv, faces=faces, nf=nf, pts=g.pts, n=n, h=float(g.h), table=g._table, capacity=g.capacity, order=g.order,
             offsets=g.offsets, r=r, support=out):
        rc = _lib.call('ppsx_trim_face_support', verts, nv, faces, nf, pts, n, g._vec3(g.lo), g._vec3(g.hi), h, float(g.inv_h), table, capacity,
                       order, offsets, r, support, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    below = float(np.nextafter(np.float32(r), np.float32(0)))         # a cell edge below r
    assert below < r
    bad = [dict(r=0.0), dict(r=-1.0), dict(r=float('nan')), dict(r=float('inf')), dict(r=-float('inf')), dict(h=below), dict(nf=-1), dict(nv=-1),
           dict(n=-1), dict(verts=None), dict(faces=None), dict(pts=None), dict(table=None), dict(order=None), dict(offsets=None),
           dict(capacity=g.capacity - 1), dict(capacity=n)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert bool((out == 0xA5).all()), kw
    assert call(support=None) == 1
    assert call(nf=0) == 0 and call(nf=0, verts=None, faces=None, support=None) == 0       # nothing launched, nothing written
    assert bool((out == 0xA5).all())
    with pytest.raises(_lib.PpsError, match='ppsx_trim_face_support failed with status 1'):
        _lib.call('ppsx_trim_face_support', verts, nv, faces, nf, g.pts, n, g._vec3(g.lo), g._vec3(g.hi), float(g.h), float(g.inv_h), g._table,
                  g.capacity, g.order, g.offsets, 0.0, out)
    slot = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    for kw in (dict(n=0), dict(capacity=n), dict(h=0.0)):
        a = dict(n=n, capacity=g.capacity, h=float(g.h))
        a.update(kw)
        rc = _lib.call('ppsx_trim_cell_slots', g.pts, a['n'], g._vec3(g.lo), g._vec3(g.hi), a['h'], float(g.inv_h), g._table, a['capacity'], slot,
                       unchecked=True)
        torch.cuda.synchronize()
        assert rc == 1 and bool((slot == -7).all()), kw
    assert call() == 0                                                # the table is untouched by the refused calls
    assert np.array_equal(out.cpu().numpy().astype(bool), scene['d2'] <= np.float64(r) * np.float64(r))
    out.fill_(0xA5)
    assert call(n=0) == 0 and bool((out == 0).all())                  # an empty cloud supports nothing: zeros
    out.fill_(0xA5)
    assert call(n=0, pts=None, table=None, order=None, offsets=None, verts=None, faces=None) == 0 and bool((out == 0).all())
    # the Python layer
    with pytest.raises(ValueError):
        trim.face_support(cloud, verts, faces, 0.0)
    with pytest.raises(ValueError):
        trim.face_support(cloud, verts, faces, float('nan'))
    assert trim.face_support(cloud, verts, faces[:0], r).shape == (0,)
    assert not bool(trim.face_support(cloud[:0], verts, faces, r).any())
    for broken in (cloud[:0], torch.cat([cloud[:5], torch.full((1, 3), float('nan'), device=DEV)]), torch.cat([cloud[:5], torch.full((1, 3), float('inf'), device=DEV)])):
        with pytest.raises(ValueError):
            trim.trim_mesh(broken, verts, faces, r)


@pytest.mark.parametrize('k', [1, 8])
def test_cloud_spacing_matches_the_spec(scene, k):
    from ppsurf_amd import trim
    cloud = scene['cloud'][:2000]
    got = trim.cloud_spacing(dev(cloud), k)
    assert type(got) is float and got == S.spacing_spec(cloud, k) and got > 0
    for n in (k, 1):
        with pytest.raises(ValueError):
            trim.cloud_spacing(dev(cloud[:n]), k)
    with pytest.raises(ValueError):
        trim.cloud_spacing(dev(cloud), 0)


def test_trim_mesh_is_the_spec_mask_and_the_small_component_rule(scene):
    from ppsurf_amd import reconstruct, trim
    r = 0.1
    # two islands on top of the sphere: four faces around one extra vertex and a single face, all within r of the cloud and dropped by the
    # 6-face rule; an unreferenced vertex in the middle of the list
    nv0 = scene['verts'].shape[0]
    top = np.array([[0, 0, 1.05], [0.03, 0, 1.02], [0, 0.03, 1.02], [-0.03, 0, 1.02], [0, -0.03, 1.02], [9, 9, 9], [0.5, 0, 0.9], [0.53, 0, 0.9],
                    [0.5, 0.03, 0.9]], dtype=np.float32)
    verts = np.concatenate([scene['verts'], top])
    isl = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [6, 7, 8]], dtype=np.int64) + nv0
    faces = np.concatenate([scene['faces'][:700], isl, scene['faces'][700:]])
    mask = S.face_support_spec(scene['cloud'], verts, faces, r)
    assert mask[700:705].all() and 0 < mask.sum() < faces.shape[0]
    want_v, want_f = reconstruct.small_components_removed(dev(verts), dev(faces[mask]))
    got_v, got_f, info = trim.trim_mesh(dev(scene['cloud']), dev(verts), dev(faces), r, spacing=0.25)
    assert got_v.dtype == torch.float32 and got_f.dtype == torch.int64
    assert np.array_equal(got_v.cpu().numpy(), want_v.cpu().numpy()) and np.array_equal(got_f.cpu().numpy(), want_f.cpu().numpy())
    assert info == {'faces_in': faces.shape[0], 'faces_supported': int(mask.sum()), 'faces_out': int(got_f.shape[0]), 'vertices_in': verts.shape[0],
                    'vertices_out': int(got_v.shape[0]), 'radius': r, 'spacing': 0.25}
    assert info['faces_out'] == info['faces_supported'] - 5           # the islands left
    # referenced vertices in their order, faces re-indexed: the corners are the corners of the surviving faces of the input, in order
    gv, gf = got_v.cpu().numpy(), got_f.cpu().numpy()
    survivors = faces[mask]
    survivors = survivors[(survivors < nv0).all(axis=1)]
    assert np.array_equal(gv[gf], verts[survivors])
    used = np.unique(survivors)
    assert np.array_equal(gv, verts[used]) and np.array_equal(np.unique(gf), np.arange(gv.shape[0]))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rec_runs(tmp_path_factory):
    """`pps.py rec` on a coloured PLY of a golden ABC cloud (resolution 33, max_points 3000) three times -- plain (mesh A), with
    gen_trim_factor (mesh B), with gen_trim_factor and gen_color_k -- and `python -m ppsurf_amd.trim --dist` on A's file.  The factor comes
    from the specification: the lower median D of A's per-face distances to the model-space cloud over the cloud's spacing."""
    from ppsurf_amd import cloud as cloud_mod, meshio, reconstruct, runner, trim
    from test_gpu_cloud import _rec_workdir
    tmp = tmp_path_factory.mktemp('trim_rec')
    pts = meshio.load_pts(ABC)[:, :3].astype(np.float32)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    rgb = np.rint(255.0 * (pts - lo[None]) / (hi - lo)[None]).astype(np.uint8)
    scan = str(tmp / 'scan.ply')
    meshio.write_ply_mesh_colored(scan, pts, np.zeros((0, 3), dtype=np.int32), rgb)
    seen = []
    export = reconstruct.export_mesh_and_refine_vertices_region_growing_v3

    def spy(**kw):                                                    # the model-space cloud the network saw
        seen.append(kw['latent']['pts'][0].t().contiguous().cpu().numpy())
        return export(**kw)

    cwd = os.getcwd()
    os.chdir(tmp)
    reconstruct.export_mesh_and_refine_vertices_region_growing_v3 = spy
    try:
        _rec_workdir(tmp)
        common = ['--data.init_args.max_points', '3000', '--model.init_args.gen_resolution_global', '33']
        model = runner.main(['pps.py', 'rec', scan, str(tmp / 'out_a')] + common)
        assert model.gen_trim_factor is None and model.last_prediction is not None
        va, fa = model.last_prediction
        cloud_ms = seen[-1]
        d2 = S.face_d2(cloud_ms, va, fa)
        D = float(np.sort(np.sqrt(d2))[(d2.shape[0] - 1) // 2])
        spacing = trim.cloud_spacing(dev(cloud_ms))
        factor = D / spacing
        model = runner.main(['pps.py', 'rec', scan, str(tmp / 'out_b'), '--model.init_args.gen_trim_factor', repr(factor)] + common)
        assert model.gen_trim_factor == factor and model.last_prediction is not None
        vb, fb = model.last_prediction
        assert np.array_equal(seen[-1], cloud_ms)
        model = runner.main(['pps.py', 'rec', scan, str(tmp / 'out_c'), '--model.init_args.gen_trim_factor', repr(factor),
                             '--model.init_args.gen_color_k', '4'] + common)
        vc, fc = model.last_prediction
        colors = model.last_colors
        padding = float(model.padding_factor)
    finally:
        reconstruct.export_mesh_and_refine_vertices_region_growing_v3 = export
        os.chdir(cwd)
    kept, _ = cloud_mod.prepare_cloud(meshio.load_pts(scan), max_points=3000, device=DEV)
    assert kept.shape[0] == cloud_ms.shape[0]
    kept_scan = str(tmp / 'kept.ply')                              # the cloud predict_step saw, in the file frame
    meshio.write_ply_points(kept_scan, pts[kept])
    scale = float(np.max(pts[kept].max(axis=0).astype(np.float64) - pts[kept].min(axis=0).astype(np.float64)) * (1.0 + padding))
    r = float(np.float64(factor) * np.float64(spacing))
    file_a = str(tmp / 'out_a' / 'scan.ply' / 'scan.ply.ply')
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    cli = subprocess.run([sys.executable, '-m', 'ppsurf_amd.trim', file_a, kept_scan, str(tmp / 'cli.ply'), '--dist', repr(r * scale)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    return {'tmp': tmp, 'a': (va, fa), 'b': (vb, fb), 'c': (vc, fc), 'colors': colors, 'd2': d2, 'r': r, 'cloud_ms': cloud_ms, 'cli': cli,
            'file_a': file_a, 'file_b': str(tmp / 'out_b' / 'scan.ply' / 'scan.ply.ply'), 'file_c': str(tmp / 'out_c' / 'scan.ply' / 'scan.ply.ply')}


def test_rec_with_gen_trim_factor_writes_the_spec_trim_of_the_plain_mesh(rec_runs):
    from ppsurf_amd import meshio, reconstruct
    R = rec_runs
    (va, fa), (vb, fb), r = R['a'], R['b'], R['r']
    mask = R['d2'] <= np.float64(r) * np.float64(r)
    want_v, want_f = reconstruct.small_components_removed(dev(va), dev(fa.astype(np.int64))[dev(mask)])
    print('mesh A {} faces, supported at r = {:.6g}: {}, mesh B {} faces'.format(fa.shape[0], r, int(mask.sum()), fb.shape[0]))
    assert 0 < fb.shape[0] < fa.shape[0]
    assert np.array_equal(vb, want_v.cpu().numpy()) and np.array_equal(fb, want_f.cpu().numpy())
    # the files: A and B differ, B's holds mesh B
    assert meshio.read_ply_mesh(R['file_a'])[1].shape[0] == fa.shape[0]
    assert np.array_equal(meshio.read_ply_mesh(R['file_b'])[1], fb)


def test_trim_and_colours_combine(rec_runs):
    from ppsurf_amd import meshio
    R = rec_runs
    (vb, fb), (vc, fc) = R['b'], R['c']
    assert np.array_equal(vc, vb) and np.array_equal(fc, fb)
    head = open(R['file_c'], 'rb').read(400)
    for name in (b'red', b'green', b'blue', b'alpha'):
        assert b'property uchar ' + name in head and b'property uchar ' + name not in open(R['file_b'], 'rb').read(400)
    assert np.array_equal(meshio.read_ply_mesh(R['file_c'])[1], fb)
    q = meshio.read_ply_vertex_colors(R['file_c'])
    assert q.shape == (vb.shape[0], 3) and np.array_equal(q, R['colors'][:, :3])


def test_trim_command_keeps_the_faces_of_predict(rec_runs):
    from ppsurf_amd import meshio
    R = rec_runs
    assert R['cli'].returncode == 0, R['cli'].stderr
    report = json.loads(R['cli'].stdout.strip().split('\n')[-1])
    r, d = R['r'], np.sqrt(R['d2'])
    supported = int((R['d2'] <= np.float64(r) * np.float64(r)).sum())
    # the command works in the file frame, predict in the model frame: a face whose distance is within 1e-6 r of r may fall either way
    near = int((np.abs(d - r) <= 1e-6 * r).sum())
    print('command: {} supported, {} out; spec: {} supported, {} within 1e-6 r of r; predict: {} out'.format(
        report['faces_supported'], report['faces_out'], supported, near, R['b'][1].shape[0]))
    assert report['faces_in'] == R['a'][1].shape[0] and report['points'] == R['cloud_ms'].shape[0] and report['spacing'] is None
    assert abs(report['faces_supported'] - supported) <= near
    v, f = meshio.read_ply_mesh(str(R['tmp'] / 'cli.ply'))
    assert f.shape[0] == report['faces_out'] and v.shape[0] == report['vertices_out']
    if near == 0:
        assert np.array_equal(f, R['b'][1])
