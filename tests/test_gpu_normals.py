"""GPU tier of the oriented normals: the three kernels of csrc/pps_normals.hip and ppsurf_amd/normals.py against the numpy
specification tests/normals_spec.py, byte for byte and twice; awkward meshes; the corner keys alone; hand-made bad rows; the blend alone; the
argument rules of the C entries; `pps.py rec --model.init_args.gen_normals` and `python -m ppsurf_amd.normals` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import eval_spec
import normals_spec as N
from test_cloud_cpu import ABC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PREFIXES = (1, 63, 64, 65, 257, 1280)
ZERO = (639, 597, 597, 596, 489, 0)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def gpu_normals(verts, faces, weight):
    from ppsurf_amd import normals
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    out, info = normals.vertex_normals(dev(v), dev(np.asarray(faces, dtype=np.int64).reshape(-1, 3)), weight)
    assert out.dtype == torch.float32 and tuple(out.shape) == (v.shape[0], 3)
    return out.cpu().numpy(), info


def same_as_spec(verts, faces, weight, want=None):
    """The device result equals the spec's bytes and info, twice."""
    if want is None:
        want = N.vertex_normals(verts, faces, weight)
    got, info = gpu_normals(verts, faces, weight)
    again, info2 = gpu_normals(verts, faces, weight)
    diff = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))[0]
    assert got.tobytes() == want.tobytes(), 'vertices {} differ: {} against {}'.format(diff[:8], got[diff[:2]], want[diff[:2]])
    assert again.tobytes() == got.tobytes() and info2 == info
    assert info == N.vertex_info(verts, faces, weight)
    return got, info


@pytest.fixture(scope='module')
def sphere():
    """The noisy icosphere(3) and ONE run of the spec per (prefix, weight), shared by every test that needs it."""
    verts, faces = N.noisy_sphere(3)
    assert verts.shape == (642, 3) and faces.shape == (1280, 3)
    want = {(nf, w): N.vertex_normals(verts, faces[:nf], w) for nf in PREFIXES for w in N.WEIGHTS}
    for a in [verts, faces] + list(want.values()):
        a.setflags(write=False)
    return {'verts': verts, 'faces': faces, 'want': want}


@pytest.mark.parametrize('weight', N.WEIGHTS)
@pytest.mark.parametrize('nf,zero', list(zip(PREFIXES, ZERO)))
def test_normals_match_the_spec_bytewise(sphere, nf, zero, weight):
    verts, faces = sphere['verts'], sphere['faces'][:nf]
    got, info = same_as_spec(verts, faces, weight, want=sphere['want'][(nf, weight)])
    unused = np.setdiff1d(np.arange(642), np.unique(faces))
    assert not got[unused].any() and info['zero_normals'] == zero == unused.shape[0] and info['faces_valid'] == nf


@pytest.mark.parametrize('subdiv', [0, 1, 2])
def test_whole_icospheres_around_the_wave_and_workgroup_sizes(subdiv):
    verts, faces = N.noisy_sphere(subdiv)
    assert verts.shape[0] == (12, 42, 162)[subdiv]
    for weight in N.WEIGHTS:
        got, info = same_as_spec(verts, faces, weight)
        assert info['zero_normals'] == 0
        flipped, _ = same_as_spec(verts, faces[:, ::-1], weight)
        assert np.array_equal(flipped, -got)                          # reversed winding: exactly the negated normals


def test_awkward_meshes():
    for weight in N.WEIGHTS:
        # the valence-300 fan, open and closed: the hub sums 300 faces in order
        for closed in (False, True):
            verts, faces = N.fan(300, closed=closed)
            _, info = same_as_spec(verts, faces, weight)
            assert info['zero_normals'] == 0 and info['faces_valid'] == (600 if closed else 300)
        # duplicated faces count twice: a square whose first face comes twice, and every face twice
        sq = np.array([[0, 0, 0.1], [4, 0, 0], [4, 4, 0.3], [0, 4, 0]], dtype=np.float32)
        two = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
        once, _ = same_as_spec(sq, two, weight)
        dup, info = same_as_spec(sq, np.concatenate([two, two[:1]]), weight)
        assert info['faces_valid'] == 3 and dup[1].tobytes() == once[1].tobytes() and dup[0].tobytes() != once[0].tobytes()
        same_as_spec(sq, np.concatenate([two, two]), weight)
        # indices -1, nv and far outside, repeated indices: invalid, never read through, and they leave the other normals alone
        verts, faces = N.noisy_sphere(1)
        nv = verts.shape[0]
        bad = np.array([[-1, 1, 2], [0, nv, 2], [0, 1, 1 << 40], [-(1 << 40), 1, 2], [3, 3, 5], [4, 5, 4], [6, 6, 6], [0, 1, (1 << 32) + 2]], dtype=np.int64)
        mixed = np.concatenate([bad[:4], faces[:30], bad[4:]])
        got, info = same_as_spec(verts, mixed, weight)
        assert info['faces_valid'] == 30 and got.tobytes() == gpu_normals(verts, faces[:30], weight)[0].tobytes()
        got, info = same_as_spec(verts, bad, weight)
        assert not got.any() and info['faces_valid'] == 0 and info['zero_normals'] == nv
        # degenerate and cancelling faces: two corners at one position, a face of no area, two coincident faces of opposite winding
        deg_v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 0, 0], [2, 0, 0], [1, 1, 1]], dtype=np.float32)
        same_as_spec(deg_v, np.array([[0, 1, 3], [0, 1, 2]], dtype=np.int64), weight)
        got, _ = same_as_spec(deg_v, np.array([[0, 1, 4]], dtype=np.int64), weight)
        assert not got.any()
        got, _ = same_as_spec(deg_v, np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64), weight)
        assert not got.any()
        huge = np.array([[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0], [1e-30, 0, 0], [0, 1e-30, 0]], dtype=np.float32)
        same_as_spec(huge, np.array([[0, 1, 2], [0, 3, 4], [1, 2, 3]], dtype=np.int64), weight)
        # nv = 1, nv = 0, nf = 0
        one = np.array([[1.5, -2.25, 1e-30]], dtype=np.float32)
        got, _ = same_as_spec(one, np.array([[0, 0, 0], [0, 1, 2]], dtype=np.int64), weight)
        assert got.tolist() == [[0, 0, 0]]
        same_as_spec(np.zeros((0, 3), dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int64), weight)
        got, info = same_as_spec(verts, np.zeros((0, 3), dtype=np.int64), weight)
        assert not got.any() and info['zero_normals'] == nv


@pytest.mark.parametrize('nf', [1, 255, 256, 257, 1280])
def test_corner_keys_alone(sphere, nf):
    from ppsurf_amd import _lib
    faces = np.array(sphere['faces'][:nf])
    faces[::7, 1] = -1                                                 # every seventh face invalid, one way or another
    faces[3::7, 2] = 642
    faces[5::7, 0] = faces[5::7, 1]
    want = N.corner_keys(faces, 642)
    keys = torch.full((3 * nf + 3,), -7, dtype=torch.int64, device=DEV)
    _lib.call('ppsx_normals_corner_keys', dev(faces), nf, 642, keys)
    got = keys.cpu().numpy()
    assert (got[3 * nf:] == -7).all()                                 # nothing written past the end
    assert np.array_equal(got[:3 * nf], want)                         # the order within a face is part of the declaration
    live = got[:3 * nf][got[:3 * nf] != N.SENTINEL]
    assert int((got == N.SENTINEL).sum()) == 3 * int((~N.valid_faces(faces, 642)).sum())
    assert (live >= 0).all() and np.unique(live).shape[0] == live.shape[0]          # distinct: the sorted order is unique


def test_incidence_matches_the_spec(sphere):
    from ppsurf_amd import normals
    faces = np.concatenate([sphere['faces'][:700], sphere['faces'][:5], np.array([[0, 0, 1], [-1, 2, 3]])])
    offsets, inc = normals.vertex_incidence(dev(faces), 642)
    assert offsets.dtype == torch.int64 and inc.dtype == torch.int32
    so, si = N.incidence(faces, 642)
    assert np.array_equal(offsets.cpu().numpy(), so) and np.array_equal(inc.cpu().numpy(), si)
    row = si[so[faces[0, 0]]:so[faces[0, 0] + 1]].tolist()
    assert row == sorted(row) and 0 in row and 700 in row             # face 0 and its duplicate 700, ascending
    o0, i0 = normals.vertex_incidence(dev(np.zeros((0, 3), dtype=np.int64)), 5)
    assert o0.tolist() == [0] * 6 and i0.shape[0] == 0
    verts, ffaces = N.fan(300)
    o, i = normals.vertex_incidence(dev(ffaces), 301)
    assert i[int(o[0]):int(o[1])].tolist() == list(range(300))


def test_the_vertex_kernel_skips_bad_rows_and_bad_entries():
    from ppsurf_amd import _lib
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4], [1, 1, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [1, 1, 2], [0, 5, 2], [2, 3, 4]], dtype=np.int64)         # faces 2 and 3 are invalid
    # row 0: face 0, face -1, face 5 (= nf), face 2 (invalid), face 3 (invalid), face 4 (does not hold 0), face 1
    # row 1: runs backwards; row 2: face 0 alone; row 3: ends past ni; row 4: empty
    inc = np.array([0, -1, 5, 2, 3, 4, 1, 0], dtype=np.int32)
    offsets = np.array([0, 7, 6, 8, 9, 9], dtype=np.int64)
    for weight in (0, 1):
        out = torch.full((5, 3), -7.0, dtype=torch.float32, device=DEV)
        _lib.call('ppsx_normals_vertex', dev(verts), 5, dev(faces), 5, dev(offsets), dev(inc), 8, weight, out)
        x = verts.astype(np.float64)
        g0, g1 = np.cross(x[1] - x[0], x[2] - x[0]), np.cross(x[1] - x[0], x[3] - x[0])
        if weight == 1:
            g0, g1 = g0 / (16.0 * 16.0), g1 / (16.0 * 16.0)
        acc = (np.zeros(3) + g0) + g1
        want = np.zeros((5, 3), dtype=np.float32)
        want[0] = (acc / np.sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2])).astype(np.float32)
        want[2] = [0, 0, 1]
        assert out.cpu().numpy().tobytes() == want.tobytes()


@pytest.fixture(scope='module')
def blend_case():
    """The 642 'area' normals of the noisy sphere and neighbour tables of 257 rows x 256 columns with out-of-range indices, rows without a valid
    neighbour and exact hits (d2 = 0)."""
    verts, faces = N.noisy_sphere(3)
    nrm = N.vertex_normals(verts, faces, 'area')
    rng = np.random.default_rng(11)
    idx = rng.integers(0, 642, size=(257, 256)).astype(np.int64)
    d2 = (rng.random((257, 256)) ** 2).astype(np.float32)
    idx[rng.random(idx.shape) < 0.1] = -1
    idx[rng.random(idx.shape) < 0.05] = 642
    idx[5, 3], idx[6, 0] = 1 << 40, -(1 << 40)
    idx[2], idx[64] = -1, 642                                          # rows without a valid neighbour
    d2[::9, 0] = 0.0                                                   # exact hits in the first column
    d2[7, 1] = 0.0
    return {'normals': nrm, 'idx': idx, 'd2': d2}


@pytest.mark.parametrize('k', [1, 8, 256])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 257])
def test_the_blend_alone(blend_case, m, k):
    from ppsurf_amd import normals
    c = blend_case
    idx, d2 = np.ascontiguousarray(c['idx'][:m, :k]), np.ascontiguousarray(c['d2'][:m, :k])
    want = N.blend(idx, d2, c['normals'])
    runs = [normals.blend_normals(dev(idx), dev(d2), dev(c['normals'])).cpu().numpy() for _ in range(2)]
    assert runs[0].dtype == np.float32 and runs[0].tobytes() == want.tobytes() and runs[1].tobytes() == runs[0].tobytes()
    if m > 2:
        assert not runs[0][2].any()                                    # no valid neighbour: zeros


@pytest.mark.parametrize('weight', N.WEIGHTS)
def test_point_normals_match_the_spec(sphere, weight):
    from ppsurf_amd import normals
    rng = np.random.default_rng(3)
    p = rng.standard_normal((300, 3))
    pts = (p / np.linalg.norm(p, axis=1)[:, None] * (1.0 + 0.01 * rng.standard_normal(300))[:, None]).astype(np.float32)
    pts[:5] = sphere['verts'][:5]                                      # points that sit on a vertex
    for k, nf in ((1, 1280), (8, 1280), (8, 257), (256, 1280)):
        faces = sphere['faces'][:nf]
        want = N.point_normals(pts, sphere['verts'], faces, k, weight)
        runs = [normals.point_normals(dev(pts), dev(sphere['verts']), dev(faces), k=k, weight=weight) for _ in range(2)]
        got = runs[0][0].cpu().numpy()
        assert got.tobytes() == want.tobytes() and runs[1][0].cpu().numpy().tobytes() == got.tobytes()
        assert runs[0][1] == runs[1][1] == N.point_info(pts, sphere['verts'], faces, k, weight)
    assert got[:5].tobytes() != np.zeros((5, 3), np.float32).tobytes()
    got, info = normals.point_normals(dev(pts), dev(sphere['verts'][:3]), dev(sphere['faces'][:0]), k=8, weight=weight)       # k is cut to nv
    assert info == {'points': 300, 'vertices': 3, 'k': 3, 'zero_normals': 300, 'weight': weight} and not got.cpu().numpy().any()
    got, info = normals.point_normals(dev(pts[:0]), dev(sphere['verts']), dev(sphere['faces']), weight=weight)
    assert tuple(got.shape) == (0, 3) and info['points'] == 0 and info['k'] == 8


def test_bad_arguments_are_an_error_return_and_write_nothing(sphere, blend_case):
    from ppsurf_amd import _lib, normals
    verts, faces = dev(sphere['verts']), dev(sphere['faces'])
    nv, nf = 642, 1280
    offsets, inc = normals.vertex_incidence(faces, nv)
    ni = int(inc.shape[0])
    out = torch.full((nv, 3), -7.0, dtype=torch.float32, device=DEV)
    keys = torch.full((3 * nf,), -7, dtype=torch.int64, device=DEV)
    idx, d2, nrm = dev(blend_case['idx'][:, :8].copy()), dev(blend_case['d2'][:, :8].copy()), dev(blend_case['normals'])
    m = 257
    bout = torch.full((m, 3), -7.0, dtype=torch.float32, device=DEV)

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def vertex(verts=verts, nv=nv, faces=faces, nf=nf, offsets=offsets, inc=inc, ni=ni, weight=0, out=out):
        return run('ppsx_normals_vertex', verts, nv, faces, nf, offsets, inc, ni, weight, out)

    def corner_keys(faces=faces, nf=nf, nv=nv, keys=keys):
        return run('ppsx_normals_corner_keys', faces, nf, nv, keys)

    def blend(idx=idx, d2=d2, m=m, k=8, normals=nrm, nv=nv, eps=1e-30, out=bout):
        return run('ppsx_normals_blend', idx, d2, m, k, normals, nv, eps, out)

    for kw in (dict(nv=-1), dict(nf=-1), dict(ni=-1), dict(nv=2 ** 31), dict(nf=2 ** 31), dict(weight=2), dict(weight=-1), dict(verts=None),
               dict(faces=None), dict(offsets=None), dict(inc=None)):
        assert vertex(**kw) == 1, kw
        assert bool((out == -7.0).all()), kw
    assert vertex(out=None) == 1
    assert vertex(nv=0) == 0 and vertex(nv=0, verts=None, faces=None, offsets=None, inc=None, out=None) == 0
    assert bool((out == -7.0).all())
    for kw in (dict(nf=-1), dict(nv=-1), dict(nv=2 ** 31), dict(nf=2 ** 31), dict(faces=None)):
        assert corner_keys(**kw) == 1, kw
        assert bool((keys == -7).all()), kw
    assert corner_keys(keys=None) == 1
    assert corner_keys(nf=0) == 0 and corner_keys(nf=0, faces=None, keys=None) == 0
    assert bool((keys == -7).all())
    for kw in (dict(m=-1), dict(nv=-1), dict(k=0), dict(k=257), dict(eps=0.0), dict(eps=-1.0), dict(eps=float('nan')), dict(idx=None),
               dict(d2=None), dict(normals=None)):
        assert blend(**kw) == 1, kw
        assert bool((bout == -7.0).all()), kw
    assert blend(out=None) == 1
    assert blend(m=0) == 0 and blend(m=0, idx=None, d2=None, normals=None, out=None) == 0
    assert bool((bout == -7.0).all())
    with pytest.raises(_lib.PpsError, match='ppsx_normals_vertex failed with status 1'):
        _lib.call('ppsx_normals_vertex', verts, nv, faces, nf, offsets, inc, ni, 2, out)
    # the good calls after the refused ones
    assert corner_keys(nv=2 ** 31 - 1) == 0 and bool((keys >= 0).all())  # the largest nv: every key positive
    assert vertex(weight=1) == 0 and out.cpu().numpy().tobytes() == sphere['want'][(1280, 'max')].tobytes()
    assert blend() == 0 and bout.cpu().numpy().tobytes() == N.blend(blend_case['idx'][:, :8], blend_case['d2'][:, :8], blend_case['normals']).tobytes()
    # NULL inc with ni = 0, NULL faces with nf = 0, NULL normals with nv = 0: the output is all zeros
    zero = torch.zeros(nv + 1, dtype=torch.int64, device=DEV)
    out.fill_(-7.0)
    assert vertex(offsets=zero, inc=None, ni=0) == 0 and not bool(out.any())
    out.fill_(-7.0)
    assert vertex(faces=None, nf=0) == 0 and not bool(out.any())
    assert blend(normals=None, nv=0) == 0 and not bool(bout.any())
    # the Python layer
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='non-finite'):
            normals.vertex_normals(torch.cat([verts[:5], torch.full((1, 3), bad, device=DEV)]), faces[:1])
        with pytest.raises(ValueError, match='non-finite'):
            normals.point_normals(torch.full((1, 3), bad, device=DEV), verts, faces)
    with pytest.raises(ValueError, match='weight'):
        normals.vertex_normals(verts, faces, 'angle')
    with pytest.raises(ValueError, match='k must be'):
        normals.point_normals(verts, verts, faces, k=257)
    with pytest.raises(ValueError, match='no vertices'):
        normals.point_normals(verts, verts[:0], faces)
    with pytest.raises(ValueError):
        normals.vertex_incidence(faces, 2 ** 31)
    with pytest.raises(_lib.PpsError, match='no CPU'):
        normals.vertex_normals(verts.cpu(), faces)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rec_runs(tmp_path_factory):
    """`pps.py rec` on a golden ABC cloud (resolution 33, max_points 3000) three times: plain (mesh A), with gen_normals area (mesh B) and, on a
    coloured copy of the cloud, with gen_normals max, gen_trim_factor, gen_smooth_iters, gen_max_faces and gen_color_k together (mesh C)."""
    from ppsurf_amd import meshio, normals, runner
    from test_gpu_cloud import _rec_workdir
    tmp = tmp_path_factory.mktemp('normals_rec')
    calls = []
    vertex_normals = normals.vertex_normals

    def counted(verts, faces, *a, **kw):
        calls.append((int(verts.shape[0]), int(faces.shape[0]), kw.get('weight', a[0] if a else 'area')))
        return vertex_normals(verts, faces, *a, **kw)

    pts = meshio.load_pts(ABC)[:, :3].astype(np.float32)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    rgb = np.rint(255.0 * (pts - lo[None]) / (hi - lo)[None]).astype(np.uint8)
    scan = str(tmp / 'scan.ply')
    meshio.write_ply_mesh_colored(scan, pts, np.zeros((0, 3), dtype=np.int32), rgb)
    cwd = os.getcwd()
    os.chdir(tmp)
    normals.vertex_normals = counted
    try:
        _rec_workdir(tmp)
        common = ['--data.init_args.max_points', '3000', '--model.init_args.gen_resolution_global', '33']
        model = runner.main(['pps.py', 'rec', ABC, str(tmp / 'out_a')] + common)
        assert model.gen_normals is None and model.last_prediction is not None and model.last_normals is None
        va, fa = model.last_prediction
        assert calls == []                                             # without the switch the stage is not reached at all
        model = runner.main(['pps.py', 'rec', ABC, str(tmp / 'out_b'), '--model.init_args.gen_normals', 'area'] + common)
        assert model.gen_normals == 'area' and model.last_prediction is not None
        (vb, fb), nb = model.last_prediction, model.last_normals
        assert calls == [(va.shape[0], fa.shape[0], 'area')]
        model = runner.main(['pps.py', 'rec', scan, str(tmp / 'out_c'), '--model.init_args.gen_normals', 'max', '--model.init_args.gen_smooth_iters', '2',
                             '--model.init_args.gen_trim_factor', '1', '--model.init_args.gen_max_faces', '500',
                             '--model.init_args.gen_color_k', '4'] + common)
        assert len(calls) == 2 and model.last_prediction is not None
        c = model.last_prediction + (model.last_normals, model.last_colors)
    finally:
        normals.vertex_normals = vertex_normals
        os.chdir(cwd)
    name = os.path.basename(ABC)
    return {'a': (va, fa), 'b': (vb, fb, nb), 'c': c, 'calls': calls, 'file_a': str(tmp / 'out_a' / name / (name + '.ply')),
            'file_b': str(tmp / 'out_b' / name / (name + '.ply')), 'file_c': str(tmp / 'out_c' / 'scan.ply' / 'scan.ply.ply')}


def test_rec_with_gen_normals_writes_the_specs_normals(rec_runs):
    from ppsurf_amd import meshio
    (va, fa), (vb, fb, nb) = rec_runs['a'], rec_runs['b']
    head_a, head_b = open(rec_runs['file_a'], 'rb').read(400), open(rec_runs['file_b'], 'rb').read(400)
    assert b'property float nx' not in head_a and meshio.read_ply_vertices(rec_runs['file_a']).shape[1] == 3
    for name in (b'nx', b'ny', b'nz'):
        assert b'property float ' + name in head_b
    assert vb.dtype == np.float32 and np.array_equal(fb, fa) and vb.tobytes() == va.tobytes()          # the mesh itself is the plain run's
    want = N.vertex_normals(vb, fb, 'area')
    assert nb.dtype == np.float32 and nb.tobytes() == want.tobytes()
    stored = meshio.read_ply_vertices(rec_runs['file_b'])
    assert stored.shape == (vb.shape[0], 6) and stored[:, 3:].astype(np.float32).tobytes() == want.tobytes()
    ma, mb = meshio.read_ply_mesh(rec_runs['file_a'], dtype=np.float64), meshio.read_ply_mesh(rec_runs['file_b'], dtype=np.float64)
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1]) and meshio.read_ply_vertex_colors(rec_runs['file_b']) is None
    volume = eval_spec.mesh_volume(va, fa)
    outward = float(np.einsum('ij,ij->i', want.astype(np.float64), va.astype(np.float64) - va.astype(np.float64).mean(axis=0)).mean())
    print('mesh A: {} vertices, {} faces, signed volume {:+.6f}, mean n . (v - centroid) {:+.4f}, {} zero normals'.format(
        va.shape[0], fa.shape[0], volume, outward, int((want == 0).all(axis=1).sum())))
    assert np.isfinite(want).all() and np.all(np.abs(np.linalg.norm(want.astype(np.float64), axis=1)[(want != 0).any(axis=1)] - 1.0) <= 1e-7)


def test_normals_combine_with_trim_smoothing_budget_and_colours(rec_runs):
    from ppsurf_amd import meshio
    vc, fc, nc, cc = rec_runs['c']
    nv_in, nf_in, weight = rec_runs['calls'][1]
    assert weight == 'max' and (nv_in, nf_in) == (vc.shape[0], fc.shape[0]) and 0 < fc.shape[0] <= 500          # on the final mesh
    assert nc.tobytes() == N.vertex_normals(vc, fc, 'max').tobytes() and cc is not None and cc.shape == (vc.shape[0], 4)
    head = open(rec_runs['file_c'], 'rb').read(500).split(b'end_header')[0].decode('ascii')
    props = [line.split()[-1] for line in head.split('\n') if line.startswith('property') and 'list' not in line]
    assert props == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'alpha']
    assert meshio.read_ply_vertices(rec_runs['file_c'])[:, 3:].astype(np.float32).tobytes() == nc.tobytes()
    assert np.array_equal(meshio.read_ply_vertex_colors(rec_runs['file_c']), cc[:, :3])
    assert np.array_equal(meshio.read_ply_mesh(rec_runs['file_c'])[1], fc)


@pytest.mark.parametrize('double', [False, True])
def test_the_command_writes_normals_for_a_coloured_ply_and_a_scan(tmp_path, capsys, double):
    from ppsurf_amd import meshio, normals
    verts, faces = N.noisy_sphere(2)
    faces = faces[:250]                                               # an open mesh: some vertices have no face
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) * 3.0 + offset[None]
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    p = rng.standard_normal((200, 3))
    scan = 3.03 * p / np.linalg.norm(p, axis=1)[:, None] + offset[None]
    src, dst, psrc, pdst = (str(tmp_path / n) for n in ('in.ply', 'out.ply', 'scan.ply', 'scan_out.ply'))
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    meshio.write_ply_points_normals(psrc, scan, np.zeros_like(scan), double=double)
    info = normals.main([src, dst, '--weight', 'max', '--points', psrc, '--points_out', pdst, '--k', '5'])
    assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == info
    stored = meshio.read_ply_mesh(src, dtype=np.float64)[0]            # what the files hold (float32 values unless double)
    pstored = meshio.read_ply_vertices(psrc)[:, :3]
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local, plocal = (stored - centre[None]).astype(np.float32), (pstored - centre[None]).astype(np.float32)
    want = N.vertex_normals(local, faces, 'max')
    pwant = N.point_normals(plocal, local, faces, 5, 'max')
    vi, pi = N.vertex_info(local, faces, 'max'), N.point_info(plocal, local, faces, 5, 'max')
    assert info == dict(vi, points=200, k=5, zero_point_normals=pi['zero_normals']) and 0 < vi['zero_normals'] < local.shape[0]
    got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
    assert np.array_equal(got_f, faces) and np.array_equal(meshio.read_ply_vertex_colors(dst), rgb) and np.array_equal(got_v, stored)
    got = meshio.read_ply_vertices(dst)
    assert got.shape[1] == 6 and got[:, 3:].astype(np.float32).tobytes() == want.tobytes()
    pgot = meshio.read_ply_vertices(pdst)
    assert np.array_equal(pgot[:, :3], pstored) and pgot[:, 3:].astype(np.float32).tobytes() == pwant.tobytes()
    for path in (dst, pdst):
        head = open(path, 'rb').read(300)
        assert (b'property double x' in head) == double and b'property float nx' in head
    # the mesh alone, area weights, no scan
    info = normals.main([src, dst])
    assert info == N.vertex_info(local, faces, 'area')
    assert meshio.read_ply_vertices(dst)[:, 3:].astype(np.float32).tobytes() == N.vertex_normals(local, faces, 'area').tobytes()
