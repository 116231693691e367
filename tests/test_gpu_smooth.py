"""GPU tier of the Taubin smoothing: the two kernels of csrc/pps_smooth.hip and ppsurf_amd/smooth.py against the numpy
specification tests/smooth_spec.py, byte for byte; awkward topologies; the half-edge keys alone; purity; the argument rules of the C
entries; `pps.py rec --model.init_args.gen_smooth_iters` and `python -m ppsurf_amd.smooth` end to end."""
import json
import os

import numpy as np
import pytest
import torch

import smooth_spec as S
from test_cloud_cpu import ABC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PREFIXES = (1, 63, 64, 65, 257, 1280)
ITERS = (1, 2, 10)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def gpu_smooth(verts, faces, iters, lam=0.5, mu=-0.53):
    from ppsurf_amd import smooth
    f = dev(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    out, out_f, info = smooth.smooth_mesh(dev(np.asarray(verts, dtype=np.float32).reshape(-1, 3)), f, iters, lam, mu)
    assert out.dtype == torch.float32 and tuple(out.shape) == (np.asarray(verts).reshape(-1, 3).shape[0], 3) and out_f is f
    return out.cpu().numpy(), info


def same_as_spec(verts, faces, iters, lam=0.5, mu=-0.53, want=None):
    """The device result equals the spec's bytes and info, twice."""
    if want is None:
        want = S.smooth_spec(verts, faces, iters, lam, mu)
    got, info = gpu_smooth(verts, faces, iters, lam, mu)
    again, info2 = gpu_smooth(verts, faces, iters, lam, mu)
    diff = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))[0]
    assert got.tobytes() == want.tobytes(), 'vertices {} differ: {} against {}'.format(diff[:8], got[diff[:2]], want[diff[:2]])
    assert again.tobytes() == got.tobytes() and info2 == info
    assert info == S.info_spec(verts, faces, iters, lam, mu)
    return got, info


@pytest.fixture(scope='module')
def sphere():
    """The noisy icosphere(3) and ONE run of the spec per (prefix, iters), shared by every test that needs it."""
    verts, faces = S.noisy_sphere(3)
    assert verts.shape == (642, 3) and faces.shape == (1280, 3)
    want = {(nf, it): S.smooth_spec(verts, faces[:nf], it) for nf in PREFIXES for it in ITERS}
    for a in [verts, faces] + list(want.values()):
        a.setflags(write=False)
    return {'verts': verts, 'faces': faces, 'want': want}


def test_the_prefixes_are_open_meshes(sphere):
    borders = [int(S.neighbours(sphere['faces'][:nf], 642)[2].sum()) for nf in PREFIXES]
    assert borders == [3, 27, 24, 25, 47, 0]
    used = [int(np.unique(sphere['faces'][:nf]).shape[0]) for nf in PREFIXES]
    assert used[0] == 3 and used[-1] == 642 and all(a <= b for a, b in zip(used, used[1:]))


@pytest.mark.parametrize('iters', ITERS)
@pytest.mark.parametrize('nf', PREFIXES)
def test_smooth_matches_the_spec_bytewise(sphere, nf, iters):
    verts, faces = sphere['verts'], sphere['faces'][:nf]
    got, info = same_as_spec(verts, faces, iters, want=sphere['want'][(nf, iters)])
    unused = np.setdiff1d(np.arange(642), np.unique(faces))
    assert got[unused].tobytes() == verts[unused].tobytes()           # unreferenced vertices come back byte-identical
    assert info['faces_valid'] == nf and info['moved_vertices'] <= 642 - unused.shape[0] and info['moved_vertices'] > 0


@pytest.mark.parametrize('subdiv', [0, 1, 2])
def test_whole_icospheres_around_the_wave_and_workgroup_sizes(subdiv):
    verts, faces = S.noisy_sphere(subdiv)
    assert verts.shape[0] == (12, 42, 162)[subdiv]
    for iters in (1, 3):
        _, info = same_as_spec(verts, faces, iters)
        assert info['border_vertices'] == 0
    same_as_spec(verts, faces, 2, lam=1.0, mu=0.0)
    got, info = same_as_spec(verts, faces, 0)
    assert got.tobytes() == verts.tobytes() and info['moved_vertices'] == 0


def test_awkward_topologies():
    # the valence-300 fan, open (the hub sums 300 neighbours in order, the ring relaxes along itself) and closed
    for closed in (False, True):
        verts, faces = S.fan(300, closed=closed)
        for iters in (1, 4):
            _, info = same_as_spec(verts, faces, iters)
            assert info['border_vertices'] == (0 if closed else 300)
    # three faces on one edge
    wing_v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0.1], [0.5, -1, 0.2], [0.5, 0.1, 1]], dtype=np.float32)
    wing = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)
    same_as_spec(wing_v, wing, 2)
    # duplicated faces: a square whose first face comes twice, and every face twice (no border left)
    sq = np.array([[0, 0, 0.1], [4, 0, 0], [4, 4, 0.3], [0, 4, 0]], dtype=np.float32)
    two = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    _, info = same_as_spec(sq, np.concatenate([two, two[:1]]), 2)
    assert info['border_vertices'] == 3
    _, info = same_as_spec(sq, np.concatenate([two, two]), 2)
    assert info['border_vertices'] == 0 and info['faces_valid'] == 4
    # indices -1, nv and far outside, a repeated index: invalid, never read through, their vertices keep their bytes
    verts, faces = S.noisy_sphere(1)
    nv = verts.shape[0]
    bad = np.array([[-1, 1, 2], [0, nv, 2], [0, 1, 1 << 40], [-(1 << 40), 1, 2], [3, 3, 5], [4, 5, 4], [6, 6, 6], [0, 1, (1 << 32) + 2]], dtype=np.int64)
    mixed = np.concatenate([bad[:4], faces[:30], bad[4:]])
    got, info = same_as_spec(verts, mixed, 3)
    assert info['faces_valid'] == 30 and got.tobytes() == gpu_smooth(verts, faces[:30], 3)[0].tobytes()
    got, info = same_as_spec(verts, bad, 3)
    assert got.tobytes() == verts.tobytes() and info['faces_valid'] == 0 and info['moved_vertices'] == 0
    # nv = 1, nv = 0, nf = 0
    one = np.array([[1.5, -2.25, 1e-30]], dtype=np.float32)
    got, _ = same_as_spec(one, np.array([[0, 0, 0], [0, 1, 2]], dtype=np.int64), 2)
    assert got.tobytes() == one.tobytes()
    same_as_spec(np.zeros((0, 3), dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int64), 2)
    got, _ = same_as_spec(verts, np.zeros((0, 3), dtype=np.int64), 2)
    assert got.tobytes() == verts.tobytes()


@pytest.mark.parametrize('nf', [1, 255, 256, 257, 1280])
def test_half_edge_keys_alone(sphere, nf):
    from ppsurf_amd import _lib
    faces = np.array(sphere['faces'][:nf])
    faces[::7, 1] = -1                                                 # every seventh face invalid, one way or another
    faces[3::7, 2] = 642
    faces[5::7, 0] = faces[5::7, 1]
    want = S.half_edge_keys(faces, 642)
    keys = torch.full((6 * nf + 6,), -7, dtype=torch.int64, device=DEV)
    _lib.call('ppsx_smooth_half_edges', dev(faces), nf, 642, keys)
    got = keys.cpu().numpy()
    assert (got[6 * nf:] == -7).all()                                 # nothing written past the end
    assert np.array_equal(got[:6 * nf], want)                         # the order within a face is part of the declaration
    assert np.array_equal(np.sort(got[:6 * nf]), np.sort(want)) and int((got == S.SENTINEL).sum()) == 6 * int((~S.valid_faces(faces, 642)).sum())
    assert (got[:6 * nf][got[:6 * nf] != S.SENTINEL] >= 0).all()


def test_adjacency_matches_the_spec_and_ignores_the_order_of_the_faces(sphere):
    from ppsurf_amd import smooth
    verts, faces = sphere['verts'], np.concatenate([sphere['faces'][:700], sphere['faces'][:5], np.array([[0, 0, 1], [-1, 2, 3]])])
    offsets, nbr, mult = smooth.mesh_adjacency(dev(faces), 642)
    assert offsets.dtype == torch.int64 and nbr.dtype == torch.int32 and mult.dtype == torch.int32
    so, sn, sm = S.adjacency(faces, 642)
    assert np.array_equal(offsets.cpu().numpy(), so) and np.array_equal(nbr.cpu().numpy(), sn) and np.array_equal(mult.cpu().numpy(), sm)
    perm = np.random.default_rng(3).permutation(faces.shape[0])
    o2, n2, m2 = smooth.mesh_adjacency(dev(faces[perm]), 642)
    assert torch.equal(o2, offsets) and torch.equal(n2, nbr) and torch.equal(m2, mult)
    assert gpu_smooth(verts, faces[perm], 3)[0].tobytes() == gpu_smooth(verts, faces, 3)[0].tobytes()
    o0, n0, m0 = smooth.mesh_adjacency(dev(np.zeros((0, 3), dtype=np.int64)), 5)
    assert o0.tolist() == [0] * 6 and n0.shape[0] == 0 and m0.shape[0] == 0


def test_the_pass_skips_bad_rows_and_bad_neighbours():
    from ppsurf_amd import _lib
    x = np.array([[1, 2, 3], [5, 7, 11], [-2, 0.5, 4], [8, -6, 0.25]], dtype=np.float64)
    offsets = np.array([0, 2, 1, 5, 6], dtype=np.int64)               # row 1 runs backwards, row 3 ends past ne = 5
    nbr = np.array([1, -1, 4, 3, 0], dtype=np.int32)                  # -1 and nv = 4 are no vertices
    mult = np.full(5, 2, dtype=np.int32)
    out = torch.full((4, 3), -7.0, dtype=torch.float64, device=DEV)
    _lib.call('ppsx_smooth_pass', dev(x), 4, dev(offsets), dev(nbr), dev(mult), 5, 0.5, out)
    want = x.copy()
    want[0] = x[0] + 0.5 * ((0.0 + x[1]) / 1.0 - x[0])                # row 0: entries 1, -1
    want[2] = x[2] + 0.5 * (((0.0 + x[3]) + x[0]) / 2.0 - x[2])      # row 2: entries -1, 4, 3, 0 in row order
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_bad_arguments_are_an_error_return_and_write_nothing(sphere):
    from ppsurf_amd import _lib, smooth
    verts, faces = dev(sphere['verts']), dev(sphere['faces'])
    nv, nf = 642, 1280
    offsets, nbr, mult = smooth.mesh_adjacency(faces, nv)
    ne = int(nbr.shape[0])
    x = verts.double()
    out = torch.full((nv, 3), -7.0, dtype=torch.float64, device=DEV)
    keys = torch.full((6 * nf,), -7, dtype=torch.int64, device=DEV)

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def one_pass(x=x, nv=nv, offsets=offsets, nbr=nbr, mult=mult, ne=ne, s=0.5, out=out):
        return run('ppsx_smooth_pass', x, nv, offsets, nbr, mult, ne, s, out)

    def half_edges(faces=faces, nf=nf, nv=nv, keys=keys):
        return run('ppsx_smooth_half_edges', faces, nf, nv, keys)

    for kw in (dict(nv=-1), dict(ne=-1), dict(s=float('nan')), dict(s=float('inf')), dict(s=-float('inf')), dict(x=None), dict(offsets=None),
               dict(nbr=None), dict(mult=None), dict(x=out)):
        assert one_pass(**kw) == 1, kw
        assert bool((out == -7.0).all()), kw
    assert one_pass(out=None) == 1 and one_pass(out=x) == 1               # out == x is refused
    assert one_pass(nv=0) == 0 and one_pass(nv=0, x=None, offsets=None, nbr=None, mult=None, out=None) == 0
    assert bool((out == -7.0).all())
    for kw in (dict(nf=-1), dict(nv=-1), dict(nv=2 ** 31), dict(faces=None)):
        assert half_edges(**kw) == 1, kw
        assert bool((keys == -7).all()), kw
    assert half_edges(keys=None) == 1
    assert half_edges(nf=0) == 0 and half_edges(nf=0, faces=None, keys=None) == 0
    assert bool((keys == -7).all())
    assert half_edges(nv=2 ** 31 - 1) == 0 and bool((keys >= 0).all())   # the largest nv: every key positive
    with pytest.raises(_lib.PpsError, match='ppsx_smooth_pass failed with status 1'):
        _lib.call('ppsx_smooth_pass', x, nv, offsets, nbr, mult, ne, float('nan'), out)
    assert one_pass() == 0                                                # the good call after the refused ones
    assert out.cpu().numpy().tobytes() == S.one_pass(sphere['verts'].astype(np.float64), *S.neighbours(sphere['faces'], nv)[:2], 0.5).tobytes()
    # an empty adjacency: NULL nbr / mult with ne = 0 is a copy
    zero = torch.zeros(nv + 1, dtype=torch.int64, device=DEV)
    assert one_pass(offsets=zero, nbr=None, mult=None, ne=0) == 0 and torch.equal(out, x)
    # the Python layer
    with pytest.raises(ValueError, match='non-finite'):
        smooth.smooth_mesh(torch.cat([verts[:5], torch.full((1, 3), float('nan'), device=DEV)]), faces[:1], 1)
    with pytest.raises(ValueError, match='non-finite'):
        smooth.smooth_mesh(torch.cat([verts[:5], torch.full((1, 3), float('inf'), device=DEV)]), faces[:1], 0)
    with pytest.raises(ValueError):
        smooth.mesh_adjacency(faces, 2 ** 31)
    with pytest.raises(_lib.PpsError, match='no CPU'):
        smooth.smooth_mesh(verts.cpu(), faces, 1)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rec_runs(tmp_path_factory):
    """`pps.py rec` on a golden ABC cloud (resolution 33, max_points 3000) three times: plain (mesh A), with gen_smooth_iters 2 (mesh B) and
    with gen_trim_factor, gen_smooth_iters and gen_max_faces together (mesh C)."""
    from ppsurf_amd import reconstruct, runner, smooth
    from test_gpu_cloud import _rec_workdir
    tmp = tmp_path_factory.mktemp('smooth_rec')
    seen, calls = [], []
    export, smooth_mesh = reconstruct.export_mesh_and_refine_vertices_region_growing_v3, smooth.smooth_mesh

    def spy(**kw):
        seen.append(sorted(k for k in kw if k in ('trim_factor', 'smooth_iters', 'max_faces')))
        return export(**kw)

    def counted(verts, faces, iters, *a, **kw):
        calls.append((int(verts.shape[0]), int(faces.shape[0]), iters))
        return smooth_mesh(verts, faces, iters, *a, **kw)

    cwd = os.getcwd()
    os.chdir(tmp)
    reconstruct.export_mesh_and_refine_vertices_region_growing_v3 = spy
    smooth.smooth_mesh = counted
    try:
        _rec_workdir(tmp)
        common = ['--data.init_args.max_points', '3000', '--model.init_args.gen_resolution_global', '33']
        model = runner.main(['pps.py', 'rec', ABC, str(tmp / 'out_a')] + common)
        assert model.gen_smooth_iters is None and model.last_prediction is not None
        va, fa = model.last_prediction
        assert seen[-1] == [] and calls == []                          # without the switch the smoothing is not reached at all
        model = runner.main(['pps.py', 'rec', ABC, str(tmp / 'out_b'), '--model.init_args.gen_smooth_iters', '2'] + common)
        assert model.gen_smooth_iters == 2 and model.last_prediction is not None
        vb, fb = model.last_prediction
        assert seen[-1] == ['smooth_iters'] and calls == [(va.shape[0], fa.shape[0], 2)]
        model = runner.main(['pps.py', 'rec', ABC, str(tmp / 'out_c'), '--model.init_args.gen_smooth_iters', '2',
                             '--model.init_args.gen_trim_factor', '1', '--model.init_args.gen_max_faces', '500'] + common)
        assert seen[-1] == ['max_faces', 'smooth_iters', 'trim_factor'] and len(calls) == 2
        c = model.last_prediction
    finally:
        reconstruct.export_mesh_and_refine_vertices_region_growing_v3 = export
        smooth.smooth_mesh = smooth_mesh
        os.chdir(cwd)
    name = os.path.basename(ABC)
    return {'a': (va, fa), 'b': (vb, fb), 'c': c, 'calls': calls, 'file_b': str(tmp / 'out_b' / name / (name + '.ply'))}


def test_rec_with_gen_smooth_iters_smooths_the_plain_mesh(rec_runs):
    from ppsurf_amd import meshio, smooth
    (va, fa), (vb, fb) = rec_runs['a'], rec_runs['b']
    assert va.dtype == np.float32 and vb.dtype == np.float32 and fa.dtype == np.int64
    assert np.array_equal(fb, fa) and vb.shape == va.shape
    want = smooth.smooth_mesh(dev(va), dev(fa), 2)[0].cpu().numpy()
    assert vb.tobytes() == want.tobytes() and vb.tobytes() != va.tobytes()
    assert vb.tobytes() == S.smooth_spec(va, fa, 2).tobytes()
    assert np.array_equal(meshio.read_ply_mesh(rec_runs['file_b'])[1], fb)


def test_smoothing_combines_with_trim_and_budget(rec_runs):
    assert rec_runs['c'] is not None
    vc, fc = rec_runs['c']
    nv_in, nf_in, iters = rec_runs['calls'][1]
    print('mesh A {} faces; smoothed after the trim at {} faces; mesh C {} faces'.format(rec_runs['a'][1].shape[0], nf_in, fc.shape[0]))
    assert iters == 2 and 0 < nf_in <= rec_runs['a'][1].shape[0]       # the smoothing saw the trimmed mesh, before the budget
    assert 0 < fc.shape[0] <= 500 and vc.dtype == np.float32 and np.isfinite(vc).all()
    assert fc.min() >= 0 and fc.max() < vc.shape[0]


@pytest.mark.parametrize('double', [False, True])
def test_the_command_smooths_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import meshio, smooth
    verts, faces = S.noisy_sphere(2)
    faces = faces[:250]                                               # an open mesh
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) * 3.0 + offset[None]
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    info = smooth.main([src, dst, '--iters', '3', '--lam', '0.5', '--mu', '-0.6'])
    assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == info
    stored = meshio.read_ply_mesh(src, dtype=np.float64)[0]            # what the file holds (float32 values unless double)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    assert info == S.info_spec(local, faces, 3, 0.5, -0.6) and info['border_vertices'] > 0 and info['moved_vertices'] > 0
    want = S.smooth_spec(local, faces, 3, 0.5, -0.6).astype(np.float64) + centre[None]
    got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
    assert np.array_equal(got_f, faces) and np.array_equal(meshio.read_ply_vertex_colors(dst), rgb)
    assert (b'property double x' in open(dst, 'rb').read(300)) == double
    assert np.array_equal(got_v, want if double else want.astype(np.float32).astype(np.float64))
