"""CPU tier of the Taubin smoothing: hand-checked cases and properties of the numpy specification
tests/smooth_spec.py, the argument rules of `smooth_mesh`, the models' `gen_smooth_iters`, the command's argument errors and the extension
entries of the C ABI."""
import ctypes
import inspect

import numpy as np
import pytest

import smooth_spec as S
import call_sites

TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32)
FACE = np.array([[0, 1, 2]], dtype=np.int64)
TET_V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], dtype=np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int64)


def test_a_single_triangle_relaxes_along_its_border():
    offsets, nbr, border = S.neighbours(FACE, 3)
    assert border.tolist() == [True] * 3 and offsets.tolist() == [0, 2, 4, 6] and nbr.tolist() == [1, 2, 0, 2, 0, 1]
    got = S.smooth_spec(TRI, FACE, 1, lam=0.5, mu=0.0)
    assert got.dtype == np.float32 and got.tolist() == [[1, 1, 0], [2, 1, 0], [1, 2, 0]]
    assert S.smooth_spec(TRI, FACE, 0).tobytes() == TRI.tobytes()
    # the inflating pass: from (1,1,0) (2,1,0) (1,2,0) with s = -1 every corner moves AWAY from the mean of the other two by its distance
    assert S.smooth_spec(TRI, FACE, 1, lam=0.5, mu=-1.0).tolist() == [[0.5, 0.5, 0], [3, 0.5, 0], [0.5, 3, 0]]


def test_a_closed_tetrahedron_has_no_border():
    offsets, nbr, border = S.neighbours(TET_F, 4)
    assert not border.any() and np.diff(offsets).tolist() == [3] * 4 and nbr.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert S.adjacency(TET_F, 4)[2].tolist() == [2] * 12
    # every vertex moves halfway to the mean m of the other three (thirds are not dyadic: the same operations, then the values)
    got = S.smooth_spec(TET_V, TET_F, 1, lam=0.5, mu=0.0)
    m = np.array([[4, 4, 4], [0, 4, 4], [4, 0, 4], [4, 4, 0]], dtype=np.float64) / 3.0
    want = TET_V.astype(np.float64) + 0.5 * (m - TET_V.astype(np.float64))
    assert got.tobytes() == want.astype(np.float32).tobytes()
    t = 2.0 / 3.0
    assert np.allclose(got, [[t, t, t], [2, t, t], [t, 2, t], [t, t, 2]], rtol=0, atol=1e-6)
    # with lam = 0.75 and three neighbours x + 0.75 (m - x) is the centroid of all four
    assert np.allclose(S.smooth_spec(TET_V, TET_F, 1, lam=0.75, mu=0.0), 1.0, rtol=0, atol=1e-6)


def test_unreferenced_vertices_and_invalid_faces_keep_their_bytes():
    verts = np.concatenate([TRI, np.array([[7, 7, 7], [-0.0, 1e-30, 3], [5, 5, 5], [6, 6, 6], [8, 8, 9]], dtype=np.float32)])
    faces = np.array([[0, 1, 2], [3, 4, -1], [4, 5, 8], [5, 6, 6], [7, 7, 7], [1 << 40, 5, 6]], dtype=np.int64)
    assert S.valid_faces(faces, 8).tolist() == [True, False, False, False, False, False]
    keys = S.half_edge_keys(faces, 8)
    assert (keys[6:] == S.SENTINEL).all() and keys[:6].tolist() == [1, 1 << 32, (1 << 32) | 2, (2 << 32) | 1, 2 << 32, 2]
    got = S.smooth_spec(verts, faces, 3)
    assert got[3:].tobytes() == verts[3:].tobytes() and not np.array_equal(got[:3], verts[:3])
    assert S.info_spec(verts, faces, 3) == {'vertices': 8, 'faces_valid': 1, 'border_vertices': 3, 'moved_vertices': 3, 'iters': 3, 'lam': 0.5,
                                            'mu': -0.53}
    assert S.smooth_spec(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 2).shape == (0, 3)
    assert S.smooth_spec(verts, np.zeros((0, 3), np.int64), 2).tobytes() == verts.tobytes()


def test_a_duplicated_face_makes_its_edges_interior():
    # two triangles over a square: the diagonal is interior, the rim a border; doubling face 0 makes its two rim edges interior too
    sq = np.array([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]], dtype=np.float32)
    two = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    offsets, nbr, border = S.neighbours(two, 4)
    assert border.all() and nbr.tolist() == [1, 3, 0, 2, 1, 3, 0, 2]              # along the rim only, never over the diagonal
    dup = np.concatenate([two, two[:1]])
    off, n_, mult = S.adjacency(dup, 4)
    assert n_.tolist() == [1, 2, 3, 0, 2, 0, 1, 3, 0, 2] and mult.tolist() == [2, 3, 1, 2, 2, 3, 2, 1, 1, 1]
    offsets, nbr, border = S.neighbours(dup, 4)
    assert border.tolist() == [True, False, True, True]                        # vertex 1 lies on doubled edges only: interior
    assert nbr[offsets[1]:offsets[2]].tolist() == [0, 2] and nbr[offsets[0]:offsets[1]].tolist() == [3]
    # three faces on one edge: that edge is interior
    wing = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)
    off, n_, mult = S.adjacency(wing, 5)
    assert mult[0] == 3 and n_[0] == 1
    offsets, nbr, border = S.neighbours(wing, 5)
    assert border.all() and nbr[offsets[0]:offsets[1]].tolist() == [2, 3, 4]       # vertex 0: its border edges, not the triple edge


def test_the_open_fan():
    verts, faces = S.fan(300)
    assert verts.shape == (301, 3) and faces.shape == (300, 3)
    offsets, nbr, border = S.neighbours(faces, 301)
    assert not border[0] and border[1:].all()
    assert nbr[offsets[0]:offsets[1]].tolist() == list(range(1, 301))
    for i in (1, 2, 150, 300):
        ring = sorted([1 + (i - 2) % 300, 1 + i % 300])
        assert nbr[offsets[i]:offsets[i + 1]].tolist() == ring and 0 not in ring
    assert np.diff(offsets)[1:].tolist() == [2] * 300
    # the hub's sum runs in ascending order: one pass equals the hand-written loop
    x = verts.astype(np.float64)
    acc = np.zeros(3)
    for j in range(1, 301):
        acc = acc + x[j]
    want = x[0] + 0.5 * (acc / 300.0 - x[0])
    assert np.array_equal(S.one_pass(x, offsets, nbr, 0.5)[0], want)
    cv, cf = S.fan(300, closed=True)
    assert not S.neighbours(cf, 302)[2].any() and np.diff(S.neighbours(cf, 302)[0]).tolist() == [300] + [4] * 300 + [300]


def test_smoothing_shrinks_the_noise_and_taubin_keeps_the_volume():
    verts, faces = S.noisy_sphere(3)
    assert verts.shape == (642, 3) and faces.shape == (1280, 3) and verts.dtype == np.float32
    rad = lambda v: np.linalg.norm(v.astype(np.float64), axis=1)
    r0 = rad(verts)
    for iters in (1, 2, 10):
        taubin, laplace = rad(S.smooth_spec(verts, faces, iters)), rad(S.smooth_spec(verts, faces, iters, 0.5, 0.0))
        print('iters {}: std {:.4f} -> {:.4f}; |dmean| taubin {:.4f} laplace {:.4f}'.format(
            iters, r0.std(), taubin.std(), abs(taubin.mean() - r0.mean()), abs(laplace.mean() - r0.mean())))
        assert taubin.std() < r0.std()
        assert abs(taubin.mean() - r0.mean()) < abs(laplace.mean() - r0.mean())


def test_smooth_mesh_argument_rules():
    import torch
    from ppsurf_amd import smooth
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in (-1, 1001, 2.5, float('nan'), '3', None, True):
        with pytest.raises(ValueError, match='iters'):
            smooth.smooth_mesh(v, f, bad)
    for bad in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='lam'):
            smooth.smooth_mesh(v, f, 1, lam=bad)
    for bad in (0.1, -0.5, -0.3, float('nan'), -float('inf')):
        with pytest.raises(ValueError, match='mu'):
            smooth.smooth_mesh(v, f, 1, lam=0.5, mu=bad)
    assert smooth._checked_params(0, 1.0, 0) == (0, 1.0, 0.0) and smooth._checked_params(np.int64(1000), 0.5, -0.53) == (1000, 0.5, -0.53)
    # good scalars, CPU tensors: the device guard of the other modules
    for fn in (lambda: smooth.smooth_mesh(v, f, 1), lambda: smooth.smooth_mesh(v, f, 0), lambda: smooth.mesh_adjacency(f, 3)):
        with pytest.raises(PpsError, match='no CPU'):
            fn()
    with pytest.raises(ValueError, match='smooth_mesh: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        smooth.smooth_mesh(v, f, 1)                                    # a ValueError like the other argument errors, with the guard's message


def test_models_take_gen_smooth_iters():
    from source.poco_model import PocoModel
    from source.ppsurf_model import PPSurfModel
    from ppsurf_amd import reconstruct
    kw = dict(output_names=['imp_surf_sign'], in_channels=3, out_channels=2, k=64, lambda_l1=0.0, debug=False,
              in_file='datasets/abc_minimal/testset.txt', results_dir='results', padding_factor=0.05, name='m', network_latent_size=32,
              gen_subsample_manifold_iter=10, gen_subsample_manifold=10000, gen_resolution_global=129, rec_batch_size=25000, gen_refine_iter=10,
              workers=0)
    pps = dict(kw, pointnet_latent_size=32, num_pts_local=50)
    assert PocoModel(**kw).gen_smooth_iters is None and PPSurfModel(**pps).gen_smooth_iters is None
    assert PocoModel(gen_smooth_iters=1, **kw).gen_smooth_iters == 1 and PocoModel(gen_smooth_iters=1000, **kw).gen_smooth_iters == 1000
    m = PPSurfModel(gen_smooth_iters='3', gen_trim_factor=2, gen_max_faces=100, gen_color_k=4, **pps)
    assert m.gen_smooth_iters == 3 and type(m.gen_smooth_iters) is int and m.gen_trim_factor == 2.0 and m.gen_max_faces == 100 and m.gen_color_k == 4
    for bad in (0, -1, 1001, 2.5, float('nan')):
        with pytest.raises(ValueError, match='gen_smooth_iters'):
            PocoModel(gen_smooth_iters=bad, **kw)
        with pytest.raises(ValueError, match='gen_smooth_iters'):
            PPSurfModel(gen_smooth_iters=bad, **pps)
    params = inspect.signature(reconstruct.export_mesh_and_refine_vertices_region_growing_v3).parameters
    assert params['smooth_iters'].default is None and list(params)[-3:] == ['trim_factor', 'smooth_iters', 'max_faces']
    for cls in (PocoModel, PPSurfModel):
        assert list(inspect.signature(cls.__init__).parameters)[-2:] == ['gen_trim_factor', 'gen_smooth_iters']


@pytest.mark.parametrize('argv', [['m.ply', 'o.ply'], ['m.ply', '--iters', '2'], ['m.ply', 'o.ply', '--iters', '-1'],
                                  ['m.ply', 'o.ply', '--iters', '1001'], ['m.ply', 'o.ply', '--iters', '2.5'], ['m.ply', 'o.ply', '--iters', 'nan'],
                                  ['m.ply', 'o.ply', '--iters', '2', '--lam', '0'], ['m.ply', 'o.ply', '--iters', '2', '--lam', '1.5'],
                                  ['m.ply', 'o.ply', '--iters', '2', '--lam', 'nan'], ['m.ply', 'o.ply', '--iters', '2', '--mu', '-0.4'],
                                  ['m.ply', 'o.ply', '--iters', '2', '--mu', '0.1'], ['m.ply', 'o.ply', '--iters', '2', '--mu', '-inf'],
                                  ['m.ply', 'o.obj', '--iters', '2']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import smooth
    with pytest.raises(SystemExit) as e:
        smooth.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_smooth_entries_are_declared_and_every_call_site_has_their_argument_count():
    from ppsurf_amd import _lib, build
    I, I64, P, D = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_smooth_half_edges'] == (I, [P, I64, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_smooth_pass'] == (I, [P, I64, P, P, P, I64, D, P, P])
    assert _lib.EXT_PARAMS['ppsx_smooth_half_edges'] == ['faces', 'nf', 'nv', 'keys', 'stream']
    assert _lib.EXT_PARAMS['ppsx_smooth_pass'] == ['x', 'nv', 'offsets', 'nbr', 'mult', 'ne', 's', 'out', 'stream']
    assert not any(n.startswith('pps_smooth') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_smooth')                    # every ppsurf_amd/*.py: the key entries are called from topology.py
    for name, where in sites.items():
        for path, line, nargs in where:
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    seen = {name: len(where) for name, where in sites.items()}
    assert seen == {'ppsx_smooth_half_edges': 1, 'ppsx_smooth_pass': 1}
    assert 'pps_smooth.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and {'ppsx_smooth_half_edges', 'ppsx_smooth_pass'} <= set(_lib._ext_entries)
