"""CPU tier of the hole filling: hand-checkable cases and invariants of the numpy specification tests/fill_spec.py, the
argument rules of `fill_holes`, the models' `gen_fill_holes`, `reconstruct`'s keyword, the command's argument errors and the extension
entries of the C ABI."""
import ctypes
import inspect

import numpy as np
import pytest

import fill_spec as S
import topology_spec as T
import call_sites

N = 12
GRID_V, GRID_F = S.height_grid(N)
P, Q = 3 * N + 3, 8 * N + 7                        # two interior vertices far apart: their fans leave two six-edge holes
TWO = S.without_fans(GRID_F, [P, Q])
BOW = S.without_fans(GRID_F, [4 * N + 4, 4 * N + 6])   # two fans whose rims share the vertex (4, 5)
LOOSE_V = np.concatenate([GRID_V, np.array([[20, 20, 0.3], [21, 20, 0.1], [20, 21, 0.2]], dtype=np.float32)])
LOOSE_F = np.concatenate([TWO, np.array([[144, 145, 146]], dtype=np.int64)])
ONE = np.delete(GRID_F, 77, axis=0)                # one interior face removed
TET_V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], dtype=np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int64)
# (name, verts, faces, max_edges): shared with the GPU tier
CASES = [('two-5', GRID_V, TWO, 5), ('two-6', GRID_V, TWO, 6), ('two-43', GRID_V, TWO, 43), ('two-44', GRID_V, TWO, 44), ('grid-44', GRID_V, GRID_F, 44),
         ('grid-43', GRID_V, GRID_F, 43), ('bow-6', GRID_V, BOW, 6), ('bow-44', GRID_V, BOW, 44), ('loose-6', LOOSE_V, LOOSE_F, 6),
         ('one-3', GRID_V, ONE, 3), ('tet-3', TET_V, TET_F, 3), ('tet-4096', TET_V, TET_F, 4096),
         ('triangle', TET_V[:3], TET_F[:1], 3), ('empty', np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 7),
         ('no-faces', GRID_V, np.zeros((0, 3), np.int64), 7)]


def border_edges(faces, nv):
    return int((T.adjacency(faces, nv)[2] == 1).sum()) // 2


def test_the_grid_is_the_one_the_cases_assume():
    assert GRID_V.shape == (144, 3) and GRID_F.shape == (242, 3) and GRID_V.dtype == np.float32
    assert S.loop_lengths(GRID_F, 144) == [44] and sorted(S.loop_lengths(TWO, 144)) == [6, 6, 44]
    assert S.directed_half_edge_counts(GRID_F, 144).max() == 1                       # consistently wound
    assert T.adjacency(GRID_F, 144)[0][P + 1] - T.adjacency(GRID_F, 144)[0][P] == 6  # an interior vertex has six neighbours


def test_the_two_fans_are_filled_at_six_and_not_at_five():
    v, f, info = S.fill_spec(GRID_V, TWO, 5)
    assert v.tobytes() == GRID_V.tobytes() and f.tobytes() == TWO.tobytes()
    assert info == {'vertices': 144, 'faces_valid': 230, 'border_edges': 56, 'loose_triangles': 0, 'rim_vertices': 56, 'nonsimple_rim_vertices': 0,
                    'loops_filled': 0, 'new_vertices': 0, 'new_faces': 0, 'border_edges_left': 56, 'max_edges': 5}
    v, f, info = S.fill_spec(GRID_V, TWO, 6)
    assert info == dict(info, loops_filled=2, new_vertices=2, new_faces=12, border_edges_left=44, max_edges=6)
    assert v.shape == (146, 3) and f.shape == (242, 3)
    # the loops come in ascending leader: the ring of P = (3, 3) first; its leader is (2, 2), and the walk runs with the faces around the hole
    ring = [2 * N + 2, 3 * N + 2, 4 * N + 3, 4 * N + 4, 3 * N + 4, 2 * N + 3]
    assert f[230:236].tolist() == [[ring[(j + 1) % 6], ring[j], 144] for j in range(6)]
    assert (f[236:, 2] == 145).all() and f[236, 1] == 7 * N + 6
    # the centroid by the written-out operations: not the removed vertex, and not exactly representable
    acc = np.zeros(3)
    for j in ring:
        acc = acc + GRID_V[j].astype(np.float64)
    assert v[144].tobytes() == (acc / 6.0).astype(np.float32).tobytes() and v[144, :2].tolist() == [3.0, 3.0] and v[144, 2] != GRID_V[P, 2]
    assert float(v[144, 2]) != float(acc[2] / 6.0)
    # the new fan has the winding of the fan that was removed: every half-edge once, no border left but the outer rim
    assert S.directed_half_edge_counts(f, 146).max() == 1 and S.loop_lengths(f, 146) == [44]


def test_the_outer_rim_is_filled_only_at_its_length():
    assert S.fill_spec(GRID_V, GRID_F, 43)[2]['loops_filled'] == 0
    v, f, info = S.fill_spec(GRID_V, GRID_F, 44)
    assert (info['loops_filled'], info['new_vertices'], info['new_faces'], info['border_edges_left']) == (1, 1, 44, 0)
    assert S.fill_spec(GRID_V, TWO, 43)[2]['loops_filled'] == 2 and S.fill_spec(GRID_V, TWO, 44)[2]['loops_filled'] == 3
    assert border_edges(f, 145) == 0 and f[242].tolist() == [1, 0, 144]              # face (0, 1, 13) holds 0 -> 1: the rim runs 0, 1, 2 .., the new faces against it
    assert f[-1].tolist() == [0, N, 144]


def test_a_bow_tie_and_a_loose_triangle_are_left_alone():
    for m in (6, 43):
        v, f, info = S.fill_spec(GRID_V, BOW, m)
        assert f.tobytes() == BOW.tobytes() and v.tobytes() == GRID_V.tobytes()
        assert info['nonsimple_rim_vertices'] == 1 and info['rim_vertices'] == 55 and info['loops_filled'] == 0
    assert S.fill_spec(GRID_V, BOW, 44)[2]['loops_filled'] == 1                      # the outer rim does not touch the bow-tie
    v, f, info = S.fill_spec(LOOSE_V, LOOSE_F, 6)
    assert info['loose_triangles'] == 1 and info['border_edges'] == 59 and info['border_edges_left'] == 47 and info['loops_filled'] == 2
    assert not (f[LOOSE_F.shape[0]:] >= 144).all(axis=1).any() and info['rim_vertices'] == 56     # nothing hangs on the free triangle
    v, f, info = S.fill_spec(TET_V[:3], TET_F[:1], 3)
    assert f.tobytes() == TET_F[:1].tobytes() and info['loose_triangles'] == 1 and info['border_edges_left'] == 3 and info['rim_vertices'] == 0


def test_a_one_face_hole_gets_its_face_back():
    v, f, info = S.fill_spec(GRID_V, ONE, 3)
    assert info['loops_filled'] == 1 and info['new_vertices'] == 0 and info['new_faces'] == 1 and v.tobytes() == GRID_V.tobytes()
    removed = GRID_F[77].tolist()
    assert f[-1].tolist() in [removed[k:] + removed[:k] for k in range(3)] and f[-1, 0] == min(removed)


def test_a_closed_tetrahedron_comes_back_as_given():
    for m in (3, 4096):
        v, f, info = S.fill_spec(TET_V, TET_F, m)
        assert v.tobytes() == TET_V.tobytes() and f.tobytes() == TET_F.tobytes()
        assert info == {'vertices': 4, 'faces_valid': 4, 'border_edges': 0, 'loose_triangles': 0, 'rim_vertices': 0, 'nonsimple_rim_vertices': 0,
                        'loops_filled': 0, 'new_vertices': 0, 'new_faces': 0, 'border_edges_left': 0, 'max_edges': m}


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_invariants_of_the_output(case):
    _, verts, faces, m = case
    nv, nf = verts.shape[0], faces.shape[0]
    v, f, info = S.fill_spec(verts, faces, m)
    assert v.dtype == np.float32 and f.dtype == np.int64
    assert v[:nv].tobytes() == verts.tobytes() and f[:nf].tobytes() == faces.tobytes()                 # the old rows, byte for byte
    assert v.shape[0] == nv + info['new_vertices'] and f.shape[0] == nf + info['new_faces']
    counts = S.directed_half_edge_counts(f, v.shape[0])
    assert counts.size == 0 or counts.max() == 1                                                       # every directed half-edge at most once
    assert info['border_edges_left'] == border_edges(f, v.shape[0])                                    # recomputed from scratch
    assert T.valid_faces(f[nf:], v.shape[0]).all() and np.isfinite(v).all()
    perm = np.random.default_rng(11).permutation(nf)
    v2, f2, info2 = S.fill_spec(verts, faces[perm], m)
    assert v2.tobytes() == v.tobytes() and f2[nf:].tobytes() == f[nf:].tobytes() and info2 == info     # the order of the faces does not matter
    assert S.fill_spec(v, f, m)[2]['loops_filled'] == 0                                                # nothing fillable is left


def test_invalid_and_duplicated_faces():
    # invalid faces are kept and ignored; a duplicated face next to the hole makes its rim edge an edge of two faces: the hole no longer closes
    bad = np.array([[-1, 1, 2], [0, 144, 2], [5, 5, 6], [1 << 40, 3, 4]], dtype=np.int64)
    v, f, info = S.fill_spec(GRID_V, np.concatenate([bad[:2], ONE, bad[2:]]), 3)
    assert info['faces_valid'] == 241 and info['loops_filled'] == 1 and f[-1].tolist() == S.fill_spec(GRID_V, ONE, 3)[1][-1].tolist()
    assert f[:2].tolist() == bad[:2].tolist() and f[243:245].tolist() == bad[2:].tolist()
    rim_face = [t for t in range(ONE.shape[0]) if len(set(ONE[t]) & set(GRID_F[77])) == 2][0]
    v, f, info = S.fill_spec(GRID_V, np.concatenate([ONE, ONE[rim_face:rim_face + 1]]), 3)
    assert info['loops_filled'] == 0 and info['nonsimple_rim_vertices'] == 2


def test_fill_holes_argument_rules():
    import torch
    from ppsurf_amd import fill, topology
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in (2, 0, -1, 4097, 2.5, 6.0, float('nan'), '6', None, True):
        with pytest.raises(ValueError, match='max_edges'):
            fill.fill_holes(v, f, bad)
    assert fill._checked_max_edges(3) == 3 and fill._checked_max_edges(np.int64(4096)) == 4096 and fill.MAX_EDGES == S.MAX_EDGES == 4096
    assert fill.CpuTensorError is topology.CpuTensorError
    with pytest.raises(fill.CpuTensorError, match='fill_holes: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        fill.fill_holes(v, f, 6)
    with pytest.raises(PpsError, match='no CPU'):
        fill.fill_holes(v, f, 3)
    with pytest.raises(ValueError, match='got ndarray'):
        fill.fill_holes(v.numpy(), f, 3)


def test_the_colour_of_a_new_vertex_is_the_rounded_integer_mean_of_its_loop():
    from ppsurf_amd import fill
    rgb = np.random.default_rng(2).integers(0, 256, size=(144, 3)).astype(np.uint8)
    v, f, info = S.fill_spec(GRID_V, TWO, 6)
    got = fill.loop_colors(rgb, f[TWO.shape[0]:], 144)
    assert got.dtype == np.uint8 and got.shape == (2, 3)
    for c in (144, 145):
        loop = f[f[:, 2] == c][:, 1]
        assert loop.shape[0] == 6
        assert got[c - 144].tolist() == [(int(rgb[loop, k].astype(np.int64).sum()) + 3) // 6 for k in range(3)]
    assert fill.loop_colors(rgb, S.fill_spec(GRID_V, ONE, 3)[1][ONE.shape[0]:], 144).shape == (0, 3)
    assert fill.loop_colors(np.full((144, 3), 255, np.uint8), f[TWO.shape[0]:], 144).tolist() == [[255] * 3] * 2


def test_models_take_gen_fill_holes():
    from source.poco_model import PocoModel
    from source.ppsurf_model import PPSurfModel
    from ppsurf_amd import reconstruct
    kw = dict(output_names=['imp_surf_sign'], in_channels=3, out_channels=2, k=64, lambda_l1=0.0, debug=False,
              in_file='datasets/abc_minimal/testset.txt', results_dir='results', padding_factor=0.05, name='m', network_latent_size=32,
              gen_subsample_manifold_iter=10, gen_subsample_manifold=10000, gen_resolution_global=129, rec_batch_size=25000, gen_refine_iter=10,
              workers=0)
    pps = dict(kw, pointnet_latent_size=32, num_pts_local=50)
    assert PocoModel(**kw).gen_fill_holes is None and PPSurfModel(**pps).gen_fill_holes is None
    assert PocoModel(gen_fill_holes=3, **kw).gen_fill_holes == 3 and PocoModel(gen_fill_holes=4096, **kw).gen_fill_holes == 4096
    m = PPSurfModel(gen_fill_holes='16', gen_normals='max', gen_smooth_iters='3', gen_trim_factor=2, gen_max_faces=100, gen_color_k=4, **pps)
    assert m.gen_fill_holes == 16 and type(m.gen_fill_holes) is int
    assert (m.gen_normals, m.gen_smooth_iters, m.gen_trim_factor, m.gen_max_faces, m.gen_color_k) == ('max', 3, 2.0, 100, 4)
    for bad in (2, 0, -1, 4097, 6.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='gen_fill_holes'):
            PocoModel(gen_fill_holes=bad, **kw)
        with pytest.raises(ValueError, match='gen_fill_holes'):
            PPSurfModel(gen_fill_holes=bad, **pps)
    for cls in (PocoModel, PPSurfModel):
        params = list(inspect.signature(cls.__init__).parameters)
        assert params[params.index('workers') + 1] == 'gen_fill_holes' and params[params.index('gen_fill_holes') + 1] == 'gen_max_faces'
        assert inspect.signature(cls.__init__).parameters['gen_fill_holes'].default is None
    params = inspect.signature(reconstruct.export_mesh_and_refine_vertices_region_growing_v3).parameters
    assert params['fill_holes'].default is None and list(params)[-4:] == ['fill_holes', 'trim_factor', 'smooth_iters', 'max_faces']


@pytest.mark.parametrize('argv', [['m.ply', 'o.ply'], ['m.ply', '--max_edges', '6'], ['m.ply', 'o.ply', '--max_edges', '2'],
                                  ['m.ply', 'o.ply', '--max_edges', '-1'], ['m.ply', 'o.ply', '--max_edges', '4097'],
                                  ['m.ply', 'o.ply', '--max_edges', '6.5'], ['m.ply', 'o.ply', '--max_edges', 'nan'],
                                  ['m.ply', 'o.obj', '--max_edges', '6'], ['m.ply', 'o.ply', '--max_edges', '6', '--iters', '2']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import fill
    with pytest.raises(SystemExit) as e:
        fill.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_fill_entries_are_declared_and_every_call_site_has_their_argument_count():
    from ppsurf_amd import _lib, build
    I, I64, P_ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.EXT_SIGNATURES['ppsx_fill_rim_keys'] == (I, [P_, I64, I64, P_, P_, P_, I64, P_, P_])
    assert _lib.EXT_SIGNATURES['ppsx_fill_loops'] == (I, [P_, I64, P_, I64, I, P_, P_])
    assert _lib.EXT_SIGNATURES['ppsx_fill_emit'] == (I, [P_, I64, P_, P_, P_, P_, P_, I64, P_, I64, P_, I64, P_])
    assert _lib.EXT_PARAMS['ppsx_fill_rim_keys'] == ['faces', 'nf', 'nv', 'offsets', 'nbr', 'mult', 'ne', 'keys', 'stream']
    assert _lib.EXT_PARAMS['ppsx_fill_loops'] == ['cand', 'nc', 'succ', 'nv', 'max_edges', 'len', 'stream']
    assert _lib.EXT_PARAMS['ppsx_fill_emit'] == ['verts', 'nv', 'succ', 'leader', 'len', 'vslot', 'foff', 'nl', 'new_verts', 'nnew', 'new_faces',
                                                 'nfnew', 'stream']
    assert not any(n.startswith('pps_fill') or n.startswith('ppsx_') for n in _lib.SIGNATURES)            # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_fill')                      # every ppsurf_amd/*.py: the key entry is called from topology.py
    for name, where in sites.items():
        for path, line, nargs in where:
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: [w[0] for w in where] for name, where in sites.items()} == {
        'ppsx_fill_rim_keys': ['topology.py'], 'ppsx_fill_loops': ['fill.py'], 'ppsx_fill_emit': ['fill.py']}
    assert 'pps_fill.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and {'ppsx_fill_rim_keys', 'ppsx_fill_loops', 'ppsx_fill_emit'} <= set(_lib._ext_entries)
