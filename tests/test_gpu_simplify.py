"""GPU tier of the mesh simplification: the kernels of csrc/pps_simplify.hip and the driver ppsurf_amd/simplify.py against
the numpy specification tests/simplify_spec.py, bit for bit; the geometric conditions with the device's closest-point query; and
`pps.py rec --model.init_args.gen_max_faces N` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import simplify_spec as S
from golden_util import REPO
from test_simplify_cpu import CUBE_FACES, abc_mesh, awkward_mesh, check_geometry, on_wall_mesh, sphere_volume

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
INTS = ('faces_in', 'verts_in', 'cells', 'survivors', 'faces_out', 'verts_out', 'fallback', 'flipped')


def _sphere(R=65):
    from ppsurf_amd import mcubes
    v, f = mcubes.marching_cubes_torch(torch.from_numpy(sphere_volume(R)).to(DEV), 0.0)
    return (v * (1.0 / (R - 1)) - 0.5).cpu().numpy(), f.cpu().numpy()


def _cases():
    """name -> (verts, faces, [grids]); a grid is ('G', G) or ('h', h)."""
    return {'cube': (S.cube_mesh(97), [('G', 1), ('G', 8), ('G', 16), ('G', 24)]),
            'abc': (abc_mesh(1), [('G', 1), ('G', 11), ('G', 37), ('G', 150)]),
            'sphere': (_sphere(65), [('G', 1), ('G', 7), ('G', 30)]),
            'duplicates_and_degenerates': (awkward_mesh(), [('h', 0.25), ('h', 0.125), ('G', 3), ('G', 1)]),
            'on_a_wall': (on_wall_mesh(), [('G', 4), ('G', 2), ('h', 0.25)])}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got_v, got_f, rep, want, where):
    assert {k: rep[k] for k in INTS} == {k: want[k] for k in INTS}, where
    assert got_f.dtype == torch.int64 and np.array_equal(got_f.cpu().numpy(), want['faces']), where
    assert got_v.dtype == torch.float64 and np.array_equal(_bits(got_v.cpu().numpy()), _bits(want['verts'])), where
    if want['h'] is not None:
        assert rep['h'] == want['h'], where
    if '_debug' in rep:
        dbg = rep['_debug']
        assert np.array_equal(dbg['leader'].cpu().numpy(), want['leader']) and np.array_equal(dbg['cid'].cpu().numpy(), want['cid']), where
        for key in ('A', 'b', 'xhat', 'pos'):
            assert np.array_equal(_bits(dbg[key].cpu().numpy()), _bits(want[key])), (where, key)
        assert np.array_equal(dbg['fallback'].cpu().numpy().astype(bool), want['fallback_mask']), where
        assert np.array_equal(dbg['used'].cpu().numpy(), want['used']), where


@pytest.mark.parametrize('name', ['cube', 'abc', 'sphere', 'duplicates_and_degenerates', 'on_a_wall'])
def test_kernels_match_the_spec_bitwise(name):
    from ppsurf_amd import simplify
    (verts, faces), grids = _cases()[name]
    nv = verts.shape[0]
    dv, df = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    small = 64
    while small <= nv:
        small *= 2                                               # the smallest legal table: long probe sequences
    runs = [simplify.ClusterGrid(dv, df), simplify.ClusterGrid(dv, df, capacity=small), simplify.ClusterGrid(dv, df, capacity=8 * small)]
    lo, hi, ext = S.box(verts)
    assert np.array_equal(runs[0].lo, lo) and np.array_equal(runs[0].hi, hi) and runs[0].ext == ext
    for kind, val in grids:
        for placement in ('mean', 'quadric'):
            kw = {'G': val} if kind == 'G' else {'h': val}
            want = S.simplify(verts, faces, placement=placement, **kw)           # nothing from the device
            for grid in runs:
                for _ in range(2):
                    got_v, got_f, rep = grid.run(placement=placement, keep=True, **kw)
                    _same(got_v, got_f, rep, want, (name, kind, val, placement, grid.capacity))
                if kind == 'G':
                    assert grid.count(val) == want['survivors']
        print('{} {}={}: {} cells, {} survivors, {} faces, {} vertices, fallback {}, flipped {}'.format(
            name, kind, val, want['cells'], want['survivors'], want['faces_out'], want['verts_out'], want['fallback'], want['flipped']))
    if name in ('abc', 'sphere'):                                # one axis is strictly the longest: two cells, no face
        got_v, got_f, rep = runs[0].run(G=1)
        assert got_v.shape == (0, 3) and got_f.shape == (0, 3) and rep['faces_out'] == 0


@pytest.mark.parametrize('G', [8, 16, 24])
def test_cube_fixture(G):
    """Condition 3 of DESIGN section 13 on the device's output."""
    from ppsurf_amd import simplify
    verts, faces = S.cube_mesh(97)
    grid = simplify.ClusterGrid(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV))
    qv, qf, qrep = grid.run(G=G)
    mv, mf, mrep = grid.run(G=G, placement='mean')
    dq, dm = S.cube_surface_distance(qv.cpu().numpy()).max(), S.cube_surface_distance(mv.cpu().numpy()).max()
    print('cube G={}: quadric {:.5f} h, mean {:.5f} h from the surface; fallback {}, flipped {}'.format(G, dq / qrep['h'], dm / qrep['h'],
                                                                                                 qrep['fallback'], qrep['flipped']))
    assert qrep['fallback'] == 0 and qrep['flipped'] == 0
    assert qrep['faces_out'] == mrep['faces_out'] == CUBE_FACES[G] and torch.equal(qf, mf)
    assert dq <= dm / 100.0


@pytest.mark.parametrize('name,G', [('cube', 16), ('abc', 37), ('sphere', 30)])
@pytest.mark.parametrize('placement', ['quadric', 'mean'])
def test_geometric_conditions(name, G, placement):
    """Conditions 1 and 2 with geometry.closest_point_on_mesh."""
    from ppsurf_amd import geometry, simplify
    (verts, faces), _ = _cases()[name]
    dv, df = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    got_v, got_f, rep = simplify.ClusterGrid(dv, df).run(G=G, placement=placement, keep=True)
    assert rep['faces_out'] > 0
    out = {'h': rep['h'], 'verts': got_v.cpu().numpy(), 'cid': rep['_debug']['cid'].cpu().numpy(), 'used': rep['_debug']['used'].cpu().numpy()}
    check_geometry(verts, faces, out, lambda q: geometry.closest_point_on_mesh(dv, df, torch.from_numpy(q).to(DEV))[1].cpu().numpy())


def test_too_fine_a_grid_is_an_error_return_and_writes_nothing():
    from ppsurf_amd import simplify
    verts, faces = S.cube_mesh(12)
    grid = simplify.ClusterGrid(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV))
    grid._scratch()
    grid._table.fill_(5)
    grid._best.fill_(6)
    grid._leader.fill_(7)
    grid._count.fill_(77)
    h = np.float64(grid.ext) / (1 << 21)                         # 2^21 cells along the longest edge
    rc, _, _ = grid.leaders_rc(h, 1.0 / h)
    torch.cuda.synchronize()
    untouched = lambda: int(grid._count.item()) == 77 and bool((grid._table == 5).all()) and bool((grid._best == 6).all()) and bool((grid._leader == 7).all())
    assert rc == 1 and untouched()
    with pytest.raises(simplify._lib.PpsError):
        grid.run(h=h)
    assert untouched()
    with pytest.raises(simplify._lib.PpsError):
        grid.run(G=1 << 21)
    assert grid.count(50) == S.count(verts, faces, 50)


def test_degenerate_meshes():
    from ppsurf_amd import simplify
    one = np.tile(np.array([[1.0, 2.0, 3.0]]), (5, 1))
    v, f, rep = simplify.simplify_mesh(one, np.array([[0, 1, 2], [2, 3, 4]]), max_faces=1, device=DEV)
    assert v.shape == (0, 3) and f.shape == (0, 3) and rep['faces_out'] == 0
    v, f, rep = simplify.simplify_mesh(one, np.zeros((0, 3), dtype=np.int64), voxel_size=0.5, device=DEV)
    assert f.shape == (0, 3) and rep['faces_out'] == 0
    with pytest.raises(ValueError, match='index'):
        simplify.simplify_mesh(np.random.RandomState(0).rand(5, 3), np.array([[0, 1, 5]]), voxel_size=0.5, device=DEV)


@pytest.mark.parametrize('name', ['cube', 'abc'])
def test_budget_search_and_simplify_mesh_match_the_spec(name):
    from ppsurf_amd import simplify
    (verts, faces), _ = _cases()[name]
    dv, df = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    small = 64
    while small <= verts.shape[0]:
        small *= 2
    for budget in (500, 5000, 50000):
        G = S.budget_search(verts, faces, budget)
        want = S.simplify(verts, faces, G)
        assert simplify.ClusterGrid(dv, df).search(budget) == G
        for cap in (None, small):
            got_v, got_f, rep = simplify.simplify_mesh(dv, df, max_faces=budget, _capacity=cap)
            assert rep['G'] == G and rep['faces_out'] <= rep['survivors'] <= budget
            _same(got_v, got_f, rep, want, (name, budget, cap))
        print('{} budget {}: G = {}, {} faces'.format(name, budget, G, want['faces_out']))
    # float32 at the edge: float32 in, float32 out, the same as the float64 result of the float32 values rounded once; host arrays are uploaded
    v32 = verts.astype(np.float32)
    want = S.simplify_budget(v32.astype(np.float64), faces, 5000, 'mean')
    got_v, got_f, rep = simplify.simplify_mesh(v32, faces.astype(np.int32), max_faces=5000, placement='mean', device=DEV)
    assert isinstance(got_v, np.ndarray) and got_v.dtype == np.float32 and got_f.dtype == np.int64
    assert np.array_equal(got_v, want['verts'].astype(np.float32)) and np.array_equal(got_f, want['faces'])
    got_v, got_f, rep = simplify.simplify_mesh(torch.from_numpy(v32).to(DEV), df, voxel_size=0.05)
    want = S.simplify(v32.astype(np.float64), faces, h=0.05)
    assert got_v.dtype == torch.float32 and np.array_equal(got_v.cpu().numpy(), want['verts'].astype(np.float32)) and rep['G'] is None
    assert np.array_equal(got_f.cpu().numpy(), want['faces'])
    # within the budget: the input comes back unchanged
    same_v, same_f, rep = simplify.simplify_mesh(dv, df, max_faces=faces.shape[0])
    assert same_v is dv and same_f is df and rep['faces_out'] == faces.shape[0] and rep['G'] is None


def test_a_budget_below_the_coarsest_grid_is_an_error():
    """The cube's three longest edges tie, so its G = 1 grid has the 8 cells of the top layers and 12 faces: the one grid accepted uncounted."""
    from ppsurf_amd import simplify
    verts, faces = S.cube_mesh(12)
    assert S.count(verts, faces, 1) == 12
    with pytest.raises(simplify._lib.PpsError, match='coarsest'):
        simplify.simplify_mesh(verts, faces, max_faces=11, device=DEV)
    assert simplify.simplify_mesh(verts, faces, max_faces=12, device=DEV)[2]['faces_out'] == 12


def _identity_scan(path):
    """A golden ABC cloud as float64 .npy whose box is centred exactly and whose longest edge T satisfies T * (1.0 + 0.05) == 1.0 exactly: `rec`
    de-normalises with scale 1 and centre 0, so the file holds the model-space float32 vertices themselves."""
    from ppsurf_amd import meshio
    from test_cloud_cpu import ABC
    pts = meshio.load_pts(ABC)[:, :3].astype(np.float64)
    pts = pts - (pts.min(axis=0) + pts.max(axis=0)) * 0.5
    T = 1.0 / 1.05
    for cand in [T] + [np.nextafter(T, s) for s in (0.0, 2.0)]:
        if cand * (1.0 + 0.05) == 1.0:
            T = cand
    assert T * (1.0 + 0.05) == 1.0
    pts = pts * (T / (pts.max(axis=0) - pts.min(axis=0)).max())
    longest = int(np.argmax(pts.max(axis=0) - pts.min(axis=0)))
    for a in range(3):
        e = T * 0.5 if a == longest else max(-pts[:, a].min(), pts[:, a].max())
        i_hi, i_lo = int(np.argmax(pts[:, a])), int(np.argmin(pts[:, a]))
        pts[i_hi, a], pts[i_lo, a] = e, -e
    bb_min, bb_max = pts.min(axis=0), pts.max(axis=0)
    assert np.max(bb_max - bb_min) * (1.0 + 0.05) == 1.0 and np.all((bb_min + bb_max) * 0.5 == 0.0)
    np.save(path, pts)


def test_rec_with_a_face_budget(tmp_path, monkeypatch):
    """(a) `rec --model.init_args.gen_max_faces N`; (b) plain `rec`, `python -m ppsurf_amd.simplify --max_faces N` on its file, then the
    small-component rule.  The input is made so that `rec` de-normalises with scale 1 and centre 0 (see _identity_scan): both routes then
    simplify the same float32 vertices and must agree.  With another scale the written vertices are rounded once more before (b) simplifies
    them, and the two meshes agree only as far as the clustering is insensitive to that rounding."""
    from ppsurf_amd import meshio, reconstruct, runner
    from test_gpu_cloud import _rec_workdir
    monkeypatch.chdir(tmp_path)
    _rec_workdir(tmp_path)
    npy = str(tmp_path / 'scan.npy')
    _identity_scan(npy)
    small = ['--model.init_args.gen_resolution_global', '33']
    model = runner.main(['pps.py', 'rec', npy, str(tmp_path / 'out_full')] + small)
    assert model.last_prediction is not None, 'no surface came out of the scan'
    full = str(tmp_path / 'out_full' / 'scan.npy' / 'scan.npy.ply')
    vf, ff = meshio.read_ply_mesh(full)
    assert np.array_equal(vf, model.last_prediction[0])          # scale 1, centre 0: the file holds the model-space vertices
    N = max(ff.shape[0] // 5, 100)
    model = runner.main(['pps.py', 'rec', npy, str(tmp_path / 'out_a'), '--model.init_args.gen_max_faces', str(N)] + small)
    assert model.gen_max_faces == N and model.last_prediction is not None
    va, fa = meshio.read_ply_mesh(str(tmp_path / 'out_a' / 'scan.npy' / 'scan.npy.ply'))
    print('{} faces -> budget {} -> {} faces, {} vertices'.format(ff.shape[0], N, fa.shape[0], va.shape[0]))
    assert 0 < fa.shape[0] <= N < ff.shape[0]

    simp = str(tmp_path / 'simplified.ply')
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'ppsurf_amd.simplify', full, simp, '--max_faces', str(N)], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=600).stdout
    report = json.loads(out.strip().split('\n')[-1])
    assert set(report) == {'faces_in', 'verts_in', 'G', 'h', 'cells', 'survivors', 'faces_out', 'verts_out', 'fallback', 'flipped'}
    assert report['faces_in'] == ff.shape[0] and report['faces_out'] <= report['survivors'] <= N and report['G'] >= 1
    assert b'property float x' in open(simp, 'rb').read(200)
    vs, fs = meshio.read_ply_mesh(simp)
    assert fs.shape[0] == report['faces_out'] and vs.shape[0] == report['verts_out']
    vb, fb = reconstruct.small_components_removed(torch.from_numpy(vs).to(DEV), torch.from_numpy(fs.astype(np.int64)).to(DEV))
    vb, fb = vb.cpu().numpy(), fb.cpu().numpy()
    assert np.array_equal(fa, fb) and va.shape == vb.shape
    assert np.all(np.abs(va.astype(np.float64) - vb.astype(np.float64)) <= np.spacing(np.abs(vb)).astype(np.float64))
    # the simplified mesh stays on the reconstruction: every vertex within sqrt(3) h of it
    from ppsurf_amd import geometry
    d = geometry.closest_point_on_mesh(torch.from_numpy(vf).to(DEV), torch.from_numpy(ff.astype(np.int64)).to(DEV), torch.from_numpy(va).to(DEV))[1]
    assert float(d.max()) <= np.sqrt(3.0) * report['h']
