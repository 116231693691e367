"""GPU tier of the feature-preserving denoising: the three kernels of csrc/pps_denoise.hip and ppsurf_amd/denoise.py
against the numpy specification tests/denoise_spec.py, byte for byte; awkward topologies; each kernel alone on hand-made tables with bad
rows and entries; the argument rules of the C entries; `python -m ppsurf_amd.denoise` end to end."""
import json

import numpy as np
import pytest
import torch

import denoise_spec as S
import smooth_spec
from test_denoise_cpu import PYR_F, PYR_V, loop_filter_pass, loop_vertex_pass

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# (threshold, normal_iters, vertex_iters): every value of {0.0, 0.5, 0.9} x {0, 1, 5} x {0, 1, 10} in three cases, and the defaults
GRID = ((0.0, 0, 1), (0.0, 1, 10), (0.0, 5, 0), (0.5, 0, 10), (0.5, 1, 0), (0.5, 5, 1), (0.9, 0, 0), (0.9, 1, 1), (0.9, 5, 10), (0.5, 5, 10))
PYR_ROWS = [[0, 1, 2, 3], [0, 3], [0, 1], [1, 2], [2, 3]]            # the incidence rows of the pyramid


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def gpu_denoise(verts, faces, T=0.5, normal_iters=5, vertex_iters=10):
    from ppsurf_amd import denoise
    f = dev(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    out, out_f, info = denoise.denoise_mesh(dev(np.asarray(verts, dtype=np.float32).reshape(-1, 3)), f, T, normal_iters, vertex_iters)
    assert out.dtype == torch.float32 and tuple(out.shape) == (np.asarray(verts).reshape(-1, 3).shape[0], 3) and out_f is f
    return out.cpu().numpy(), info


def gpu_normals(verts, faces, T, normal_iters):
    from ppsurf_amd import denoise
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = denoise.filtered_face_normals(dev(np.asarray(verts, dtype=np.float32).reshape(-1, 3)), dev(f), T, normal_iters)
    assert n.dtype == torch.float64 and tuple(n.shape) == (f.shape[0], 3)
    return n.cpu().numpy()


def same_as_spec(verts, faces, T=0.5, normal_iters=5, vertex_iters=10):
    """The device's vertices, info and filtered normals equal the spec's, the vertices twice."""
    want = S.denoise_spec(verts, faces, T, normal_iters, vertex_iters)
    got, info = gpu_denoise(verts, faces, T, normal_iters, vertex_iters)
    again, info2 = gpu_denoise(verts, faces, T, normal_iters, vertex_iters)
    diff = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))[0]
    assert got.tobytes() == want.tobytes(), 'vertices {} differ: {} against {}'.format(diff[:8], got[diff[:2]], want[diff[:2]])
    assert again.tobytes() == got.tobytes() and info2 == info
    assert info == S.info_spec(verts, faces, T, normal_iters, vertex_iters)
    want_n = S.filtered_normals_spec(verts, faces, T, normal_iters)
    got_n = gpu_normals(verts, faces, T, normal_iters)
    diff = np.nonzero((got_n != want_n).any(axis=1))[0]
    assert got_n.tobytes() == want_n.tobytes(), 'normals {} differ: {} against {}'.format(diff[:8], got_n[diff[:2]], want_n[diff[:2]])
    assert gpu_normals(verts, faces, T, normal_iters).tobytes() == got_n.tobytes()
    return got, info


def noisy_cube(n):
    verts, faces, _ = S.cube(n)
    return (verts + np.random.default_rng(7).normal(0, 0.1, verts.shape)).astype(np.float32), faces


def mesh(name):
    if name in ('cube4', 'cube5'):                                    # 192 faces: under one workgroup; 300: a second, partly filled
        return noisy_cube(int(name[4:]))
    if name.startswith('cube8'):                                      # 768 = 3 x 256 faces; the prefixes 255, 257 and 766 are open meshes
        verts, faces = noisy_cube(8)
        return verts, faces[:int(name[6:] or 768)]
    if name == 'sphere':
        return smooth_spec.noisy_sphere()
    assert name == 'fan300'                                           # one vertex whose row makes every neighbourhood 300 faces
    return smooth_spec.fan(300)


@pytest.mark.parametrize('name', ['cube4', 'cube5', 'cube8', 'cube8:255', 'cube8:257', 'cube8:766', 'sphere', 'fan300'])
def test_denoise_matches_the_spec_bytewise(name):
    verts, faces = mesh(name)
    assert faces.shape[0] == {'cube4': 192, 'cube5': 300, 'cube8': 768, 'cube8:255': 255, 'cube8:257': 257, 'cube8:766': 766, 'sphere': 1280, 'fan300': 300}[name]
    for T, normal_iters, vertex_iters in GRID:
        got, info = same_as_spec(verts, faces, T, normal_iters, vertex_iters)
        assert info['faces_valid'] == faces.shape[0] and info['degenerate_faces'] == 0
        # without the filter a vertex lies in the planes of its own faces and moves by rounding errors at the most
        assert info['moved_vertices'] == 0 if vertex_iters == 0 else info['moved_vertices'] > 0 or normal_iters == 0
        unused = np.setdiff1d(np.arange(verts.shape[0]), np.unique(faces))
        assert got[unused].tobytes() == verts[unused].tobytes()       # unreferenced vertices come back byte-identical
    if name == 'fan300':
        assert np.diff(S.neighbourhoods(faces, 301)[0]).tolist() == [300] * 300


@pytest.mark.parametrize('n', [5, 8])
def test_the_exact_cubes(n):
    verts, faces, normals = S.cube(n)
    got, info = same_as_spec(verts, faces)
    assert got.tobytes() == verts.astype(np.float32).tobytes() and info['moved_vertices'] == 0          # nothing to denoise
    assert np.array_equal(gpu_normals(verts, faces, 0.5, 5), normals)


def test_awkward_topologies():
    verts, faces = smooth_spec.noisy_sphere(1)
    nv = verts.shape[0]
    # indices -1, nv and far outside, a repeated index: invalid, never read through, their vertices keep their bytes
    bad = np.array([[-1, 1, 2], [0, nv, 2], [0, 1, 1 << 40], [-(1 << 40), 1, 2], [3, 3, 5], [4, 5, 4], [6, 6, 6], [0, 1, (1 << 32) + 2]], dtype=np.int64)
    mixed = np.concatenate([bad[:4], faces[:30], bad[4:]])
    got, info = same_as_spec(verts, mixed, 0.5, 3, 4)
    assert info['faces_valid'] == 30 and got.tobytes() == gpu_denoise(verts, faces[:30], 0.5, 3, 4)[0].tobytes()
    got, info = same_as_spec(verts, bad, 0.5, 3, 4)
    assert got.tobytes() == verts.tobytes() and info['faces_valid'] == 0 and info['moved_vertices'] == 0
    # a duplicated face is two faces; an area-free face has a zero normal, keeps it and is counted
    same_as_spec(PYR_V, np.concatenate([PYR_F, PYR_F[:1]]), 0.5, 2, 3)
    flat_v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [1, 1, 1]], dtype=np.float32)
    flat_f = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 4]], dtype=np.int64)
    for T in (0.0, 0.5):
        got, info = same_as_spec(flat_v, flat_f, T, 2, 2)
        assert info['degenerate_faces'] == 1 and got[3].tobytes() == flat_v[3].tobytes()
        assert (gpu_normals(flat_v, flat_f, T, 2)[1] == 0).all()
    # three faces on one edge
    wing_v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0.1], [0.5, -1, 0.2], [0.5, 0.1, 1]], dtype=np.float32)
    same_as_spec(wing_v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64), 0.0, 2, 2)
    # nv = 1, nv = 0, nf = 0: an empty mesh comes back as given
    one = np.array([[1.5, -2.25, 1e-30]], dtype=np.float32)
    got, _ = same_as_spec(one, np.array([[0, 0, 0], [0, 1, 2]], dtype=np.int64), 0.5, 2, 2)
    assert got.tobytes() == one.tobytes()
    same_as_spec(np.zeros((0, 3), dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int64), 0.5, 2, 2)
    same_as_spec(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int64), 0.5, 2, 2)
    got, _ = same_as_spec(verts, np.zeros((0, 3), dtype=np.int64), 0.5, 2, 2)
    assert got.tobytes() == verts.tobytes()


def guarded(rows, dtype=torch.float64):
    """(buffer [rows + 2, 3] filled with -7, its rows 1 .. rows as the output): a guard row on either side."""
    buf = torch.full((rows + 2, 3), -7.0, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1]


def guards_intact(buf):
    return bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())


@pytest.mark.parametrize('nf', [1, 255, 256, 257, 1280])
def test_face_normals_alone(nf):
    from ppsurf_amd import _lib
    verts, faces = smooth_spec.noisy_sphere()
    faces = np.array(faces[:nf])
    faces[::7, 1] = -1                                                 # every seventh face invalid, one way or another
    faces[3::7, 2] = 642
    faces[5::7, 0] = faces[5::7, 1]
    buf, out = guarded(nf)
    _lib.call('ppsx_denoise_face_normals', dev(verts), 642, dev(faces), nf, out)
    want = S.face_normals(verts, faces)
    assert guards_intact(buf) and out.cpu().numpy().tobytes() == want.tobytes()
    assert (want[~S.valid_faces(faces, 642)] == 0).all()


# hand-made incidence tables over the pyramid (nv = 5, nf = 4, ni = 12): (offsets, inc, the rows they stand for once the bad ones are dropped)
CLEAN_INC = [0, 1, 2, 3, 0, 3, 0, 1, 1, 2, 2, 3]
TABLES = {
    'as built': ([0, 4, 6, 8, 10, 12], CLEAN_INC, PYR_ROWS),
    'a descending row, a row past ni, a row that starts past ni': ([2, 4, 0, 4, 13, 12], CLEAN_INC, [[2, 3], [], [0, 1, 2, 3], [], []]),
    'a negative offset': ([-1, 4, 6, 8, 10, 12], CLEAN_INC, [[], [0, 3], [0, 1], [1, 2], [2, 3]]),
    'offsets far outside': ([0, 4, 1 << 40, 8, -(1 << 40), 12], CLEAN_INC, [[0, 1, 2, 3], [], [], [], []]),
    'entries below 0 and from nf on': ([0, 4, 6, 8, 10, 12], [0, -1, 2, 4, 0, 3, -5, 1, 1, 2 ** 31 - 1, 2, 3],
                                       [[0, 2], [0, 3], [1], [1], [2, 3]]),
}


@pytest.mark.parametrize('table', sorted(TABLES))
def test_the_filter_pass_alone_skips_bad_rows_and_entries(table):
    from ppsurf_amd import _lib
    offsets, inc, rows = TABLES[table]
    # faces 4 and 5 have vertex indices out of range: invalid, zeros, their rows are never opened
    faces = np.concatenate([PYR_F, np.array([[0, 1, 9], [-1, 2, 3]], dtype=np.int64)])
    normals = np.concatenate([S.face_normals(PYR_V, PYR_F), np.zeros((2, 3))])
    buf, out = guarded(6)
    _lib.call('ppsx_denoise_filter_pass', dev(faces), 6, 5, dev(np.array(offsets, dtype=np.int64)), dev(np.array(inc, dtype=np.int32)), 12,
              dev(normals), 0.5, out)
    # a face visits the union of the cleaned rows of its corners, every face once, in ascending index
    valid = [sorted(set(j for v in face for j in rows[v] if 0 <= j < 6)) for face in PYR_F.tolist()] + [[], []]
    want = np.array(loop_filter_pass(normals.tolist(), valid, 0.5))
    assert guards_intact(buf) and out.cpu().numpy().tobytes() == want.tobytes()
    assert (want[4:] == 0).all()
    if table == 'as built':
        assert want[:4].tobytes() == S.filter_pass(normals[:4], *S.neighbourhoods(PYR_F, 5), 0.5).tobytes()


@pytest.mark.parametrize('table', sorted(TABLES))
def test_the_vertex_pass_alone_skips_bad_rows_and_entries(table):
    from ppsurf_amd import _lib
    offsets, inc, rows = TABLES[table]
    faces = np.concatenate([PYR_F, np.array([[0, 1, 9], [-1, 2, 3]], dtype=np.int64)])
    normals = np.concatenate([S.filtered_normals_spec(PYR_V, PYR_F, 0.5, 2), np.full((2, 3), 0.5)])
    x = PYR_V.astype(np.float64) + np.random.default_rng(1).normal(0, 0.05, PYR_V.shape)
    buf, out = guarded(5)
    _lib.call('ppsx_denoise_vertex_pass', dev(x), 5, dev(faces), 6, dev(normals), dev(np.array(offsets, dtype=np.int64)),
              dev(np.array(inc, dtype=np.int32)), 12, out)
    # a vertex counts the entries of its row, in row order, that are faces, valid ones, and hold it
    clean = [[k for k in rows[v] if 0 <= k < 4 and v in PYR_F[k]] for v in range(5)]
    want = np.array(loop_vertex_pass(x.tolist(), faces.tolist(), normals.tolist(), clean))
    assert guards_intact(buf) and out.cpu().numpy().tobytes() == want.tobytes()
    if table == 'as built':
        assert clean == PYR_ROWS and want.tobytes() == S.vertex_pass(x, PYR_F, normals[:4], *S.incidence(PYR_F, 5)).tobytes()
    kept = [v for v in range(5) if not clean[v]]
    assert want[kept].tobytes() == x[kept].tobytes()                  # a vertex without a counted face keeps its value


def test_the_vertex_pass_alone_skips_invalid_faces_in_its_rows():
    from ppsurf_amd import _lib
    # the rows list faces 4 (an index out of range), 5 (a repeated index) and, at vertex 1, face 1, which does not hold it
    faces = np.concatenate([PYR_F, np.array([[0, 1, 9], [2, 2, 0]], dtype=np.int64)])
    normals = np.concatenate([S.face_normals(PYR_V, PYR_F), np.full((2, 3), 0.5)])
    x = PYR_V.astype(np.float64) + np.random.default_rng(2).normal(0, 0.05, PYR_V.shape)
    offsets, inc = [0, 6, 10, 13, 15, 17], [0, 1, 2, 3, 4, 5, 0, 1, 3, 4, 0, 1, 5, 1, 2, 2, 3]
    buf, out = guarded(5)
    _lib.call('ppsx_denoise_vertex_pass', dev(x), 5, dev(faces), 6, dev(normals), dev(np.array(offsets, dtype=np.int64)),
              dev(np.array(inc, dtype=np.int32)), 17, out)
    want = np.array(loop_vertex_pass(x.tolist(), faces.tolist(), normals.tolist(), PYR_ROWS))
    assert guards_intact(buf) and out.cpu().numpy().tobytes() == want.tobytes()


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, denoise, topology
    hv, hf = smooth_spec.noisy_sphere()
    verts, faces = dev(hv), dev(hf)
    nv, nf = 642, 1280
    offsets, inc = topology.vertex_incidence(faces, nv)
    ni = int(inc.shape[0])
    x = verts.double()
    normals = denoise.filtered_face_normals(verts, faces, 0.5, 0)
    out_n = torch.full((nf, 3), -7.0, dtype=torch.float64, device=DEV)
    out_x = torch.full((nv, 3), -7.0, dtype=torch.float64, device=DEV)
    big = 2 ** 31

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def face_normals(verts=verts, nv=nv, faces=faces, nf=nf, normals=out_n):
        return run('ppsx_denoise_face_normals', verts, nv, faces, nf, normals)

    def filter_pass(faces=faces, nf=nf, nv=nv, offsets=offsets, inc=inc, ni=ni, normals=normals, T=0.5, out=out_n):
        return run('ppsx_denoise_filter_pass', faces, nf, nv, offsets, inc, ni, normals, T, out)

    def vertex_pass(x=x, nv=nv, faces=faces, nf=nf, normals=normals, offsets=offsets, inc=inc, ni=ni, out=out_x):
        return run('ppsx_denoise_vertex_pass', x, nv, faces, nf, normals, offsets, inc, ni, out)

    for kw in (dict(nv=-1), dict(nf=-1), dict(nv=big), dict(nf=big), dict(verts=None), dict(faces=None)):
        assert face_normals(**kw) == 1, kw
        assert bool((out_n == -7.0).all()), kw
    assert face_normals(normals=None) == 1
    assert face_normals(nf=0) == 0 and face_normals(nf=0, verts=None, faces=None, normals=None) == 0 and bool((out_n == -7.0).all())
    for kw in (dict(nv=-1), dict(nf=-1), dict(ni=-1), dict(nv=big), dict(nf=big), dict(T=float('nan')), dict(T=1.0), dict(T=-0.1), dict(T=float('inf')),
               dict(T=-float('inf')), dict(T=1.5), dict(faces=None), dict(offsets=None), dict(inc=None), dict(normals=None), dict(normals=out_n)):
        assert filter_pass(**kw) == 1, kw
        assert bool((out_n == -7.0).all()), kw
    assert filter_pass(out=None) == 1 and filter_pass(out=normals) == 1 and filter_pass(normals=out_n, out=out_n) == 1   # out == normals is refused
    assert filter_pass(nf=0) == 0 and filter_pass(nf=0, faces=None, offsets=None, inc=None, normals=None, out=None) == 0
    assert bool((out_n == -7.0).all())
    for kw in (dict(nv=-1), dict(nf=-1), dict(ni=-1), dict(nv=big), dict(nf=big), dict(x=None), dict(faces=None), dict(normals=None),
               dict(offsets=None), dict(inc=None), dict(x=out_x)):
        assert vertex_pass(**kw) == 1, kw
        assert bool((out_x == -7.0).all()), kw
    assert vertex_pass(out=None) == 1 and vertex_pass(out=x) == 1         # out == x is refused
    assert vertex_pass(nv=0) == 0 and vertex_pass(nv=0, x=None, faces=None, normals=None, offsets=None, inc=None, out=None) == 0
    assert bool((out_x == -7.0).all())
    with pytest.raises(_lib.PpsError, match='ppsx_denoise_filter_pass failed with status 1'):
        _lib.call('ppsx_denoise_filter_pass', faces, nf, nv, offsets, inc, ni, normals, float('nan'), out_n)
    # the good calls after the refused ones
    want_n = S.filtered_normals_spec(hv, hf, 0.5, 1)
    assert filter_pass() == 0 and out_n.cpu().numpy().tobytes() == want_n.tobytes()
    assert filter_pass(T=0.0) == 0 and filter_pass(T=float(np.nextafter(1.0, 0.0))) == 0                 # the ends of [0, 1)
    assert vertex_pass() == 0
    assert out_x.cpu().numpy().tobytes() == S.vertex_pass(hv.astype(np.float64), hf, S.face_normals(hv, hf), *S.incidence(hf, nv)).tobytes()
    # no faces: NULL faces, normals and inc with nf = ni = 0 is a copy
    zero = torch.zeros(nv + 1, dtype=torch.int64, device=DEV)
    assert vertex_pass(faces=None, nf=0, normals=None, offsets=zero, inc=None, ni=0) == 0 and torch.equal(out_x, x)
    # the Python layer
    for fn in (denoise.denoise_mesh, denoise.filtered_face_normals):
        with pytest.raises(ValueError, match='non-finite'):
            fn(torch.cat([verts[:5], torch.full((1, 3), float('nan'), device=DEV)]), faces[:1])
    with pytest.raises(ValueError, match='non-finite'):
        denoise.denoise_mesh(torch.cat([verts[:5], torch.full((1, 3), float('inf'), device=DEV)]), faces[:1], 0.5, 0, 0)
    with pytest.raises(ValueError, match='threshold'):
        denoise.denoise_mesh(verts.cpu(), faces, 1.0)                      # the parameters come first
    with pytest.raises(denoise.CpuTensorError, match='no CPU'):
        denoise.denoise_mesh(verts.cpu(), faces)


@pytest.mark.parametrize('double', [False, True])
def test_the_command_denoises_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import denoise, meshio
    verts, faces = noisy_cube(5)
    faces = faces[:140]                                               # an open mesh
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) * 3.0 + offset[None]
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    info = denoise.main([src, dst, '--threshold', '0.4', '--normal_iters', '3', '--vertex_iters', '4'])
    assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == info
    stored = meshio.read_ply_mesh(src, dtype=np.float64)[0]            # what the file holds (float32 values unless double)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    assert info == S.info_spec(local, faces, 0.4, 3, 4) and info['moved_vertices'] > 0 and info['faces_valid'] == 140
    assert info['threshold'] == 0.4 and info['normal_iters'] == 3 and info['vertex_iters'] == 4
    direct = denoise.denoise_mesh(dev(local), dev(faces), 0.4, 3, 4)[0].cpu().numpy()
    assert direct.tobytes() == S.denoise_spec(local, faces, 0.4, 3, 4).tobytes()
    want = direct.astype(np.float64) + centre[None]
    got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
    assert np.array_equal(got_f, faces) and np.array_equal(meshio.read_ply_vertex_colors(dst), rgb)
    assert (b'property double x' in open(dst, 'rb').read(300)) == double
    assert np.array_equal(got_v, want if double else want.astype(np.float32).astype(np.float64))
    # the defaults
    info = denoise.main([src, dst])
    assert (info['threshold'], info['normal_iters'], info['vertex_iters']) == (0.5, 5, 10) and info == S.info_spec(local, faces)
