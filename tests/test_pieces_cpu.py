"""CPU tier of the removal of isolated pieces: the numpy specification tests/pieces_spec.py against values written out
by hand and against oracle.mesh_oracle.components_union_find, its edge cases, the argument rules of `remove_pieces` and of the command, and
the extension entries of the C ABI."""
import ctypes

import numpy as np
import pytest

import call_sites
import pieces_spec as S
from oracle import mesh_oracle


def test_the_scene_by_hand():
    verts, faces = S.scene()
    assert verts.shape == (642, 3) and verts.dtype == np.float32 and faces.shape == (1260, 3)
    t = S.table_spec(verts, faces)
    assert t['label'].dtype == np.int32 and t['leader'].tolist() == sorted(S.SCENE_FACES)
    assert dict(zip(t['leader'].tolist(), t['faces'].tolist())) == S.SCENE_FACES
    assert dict(zip(t['leader'].tolist(), t['diag2'].tolist())) == S.SCENE_DIAG2 and t['box_diag2'] == 768.0
    assert t['lo'].dtype == np.float32 and t['lo'][5].tolist() == [12, 0, 12] and t['hi'][5].tolist() == [14, 2, 14]
    assert t['lo'][0].tolist() == [0, 0, 0] and t['hi'][1].tolist() == [16, 16, 16]
    bounds = np.cumsum([0] + list(S.SCENE_FACES.values()))
    for c, leader in enumerate(sorted(S.SCENE_FACES)):
        assert (t['label'][bounds[c]:bounds[c + 1]] == leader).all()
    assert 0.25 * 768 == 192 and (1 / 64) * 768 == 12
    for rules, leaders in S.SCENE_GRID:
        out_v, out_f, info, kept = S.remove_spec(verts, faces, *rules)
        assert kept == leaders, rules
        assert info['faces_out'] == sum(S.SCENE_FACES[l] for l in leaders) == out_f.shape[0]
        assert info['components'] == 6 and info['components_kept'] == len(leaders) and info['largest_faces'] == 768
        assert (info['min_faces'], info['min_diag_frac'], info['keep_largest']) == rules and info['box_diag2'] == 768.0
        assert info['faces_in'] == info['faces_valid'] == 1260 and info['vertices_in'] == 642 and info['vertices_out'] == out_v.shape[0]
        assert out_f.shape[0] == 0 or (np.array_equal(np.unique(out_f), np.arange(out_v.shape[0])))
        # the kept faces in their order, on the kept rows byte for byte
        mask = np.isin(t['label'], leaders)
        assert out_v[out_f].tobytes() == verts[faces[mask]].tobytes()
    assert S.remove_spec(verts, faces, 48)[2]['faces_out'] == 1248 and S.remove_spec(verts, faces, 49)[2]['faces_out'] == 1152
    assert S.remove_spec(verts, faces, None, 0.125)[2]['faces_out'] == 1248 and S.remove_spec(verts, faces, None, None, 3)[2]['faces_out'] == 1152


def test_the_scene_in_other_face_orders():
    verts, built = S.scene()
    sizes = sorted(S.SCENE_FACES.values())
    robin = S.table_spec(*S.scene('robin'))
    assert robin['leader'].tolist() == [0, 1, 2, 3, 4, 5] and robin['faces'].tolist() == [768, 192, 48, 48, 12, 192]
    assert len(set(robin['label'][:64].tolist())) == 6                                      # every wave mixes components
    perm = S.table_spec(*S.scene('permuted'))
    assert sorted(perm['faces'].tolist()) == sizes and perm['box_diag2'] == 768.0
    for order in ('robin', 'permuted'):
        v, f = S.scene(order)
        assert sorted(map(tuple, f.tolist())) == sorted(map(tuple, built.tolist()))
        for rules, leaders in S.SCENE_GRID:
            # which of the two components of 192 faces wins the tie depends on the order; the number of faces kept does not
            assert S.remove_spec(v, f, *rules)[2]['faces_out'] == sum(S.SCENE_FACES[l] for l in leaders), (order, rules)
    # keep_largest = 2 as built keeps the cube of 4 at (12, 12, 12): leader 768 comes before 1068
    out_v, _, _, kept = S.remove_spec(verts, built, None, None, 2)
    assert kept == [0, 768] and out_v.max() == 16.0
    v, f = S.scene('invalid')
    t = S.table_spec(v, f)
    assert f.shape == (1263, 3) and t['label'][301:304].tolist() == [-1, -1, -1] and t['leader'].tolist() == [0, 771, 963, 1011, 1059, 1071]
    assert t['faces'].tolist() == [768, 192, 48, 48, 12, 192]
    out_v, out_f, info, _ = S.remove_spec(v, f, None, 0.0)
    assert info['faces_in'] == 1263 and info['faces_valid'] == 1260 and info['faces_out'] == 1260 and out_f.tobytes() == built.tobytes()


def test_prefixes_strips_debris_and_small_topologies():
    for prefix, want in ((255, [128, 127]), (257, [128, 128, 1]), (766, [766])):
        assert S.table_spec(*S.cube8(prefix))['faces'].tolist() == want
    for order in ('ascending', 'reversed', 'permuted'):
        t = S.table_spec(*S.strip(1000, order))
        assert t['leader'].tolist() == [0] and t['faces'].tolist() == [1000] and (t['label'] == 0).all()
    verts, faces = S.debris()
    t = S.table_spec(verts, faces)
    assert faces.shape == (672, 3) and t['leader'].shape == (158,) and int((t['faces'] == 1).sum()) == 81
    assert int((t['faces'] == 33).sum()) == 2 and int(t['faces'].max()) == 66 and int(t['faces'].sum()) == 672
    for name in S.SMALL:
        verts, faces, want = S.small(name)
        assert S.table_spec(verts, faces)['faces'].tolist() == want, name
    assert S.small('welded vertex')[0].shape == (15, 3) and S.small('welded edge')[0].shape == (14, 3)
    assert S.pairs(S.fins()[1], 5) == set()
    assert S.pairs(np.array([[0, 1, 2], [2, 1, 3], [7, 7, 1]]), 4) == {(0, 1)}


@pytest.mark.parametrize('name', ['scene', 'scene robin', 'scene permuted', 'cube8:255', 'cube8:257', 'cube8:766', 'strip', 'strip reversed',
                                  'strip permuted', 'debris'] + list(S.SMALL))
def test_the_labels_are_those_of_the_oracle(name):
    if name.startswith('scene'):
        verts, faces = S.scene(name[6:] or 'built')
    elif name.startswith('cube8'):
        verts, faces = S.cube8(int(name[6:]))
    elif name.startswith('strip'):
        verts, faces = S.strip(1000, name[6:] or 'ascending')
    elif name == 'debris':
        verts, faces = S.debris()
    else:
        verts, faces, _ = S.small(name)
    assert S.valid_faces(faces, verts.shape[0]).all()
    assert np.array_equal(S.labels_spec(faces, verts.shape[0]), mesh_oracle.components_union_find(faces))


def test_signed_zero_and_the_box():
    verts = np.array([[-0.0, 0, 0], [1, -0.0, 0], [0, 1, -0.0], [-2, 0, 0], [-3, -0.0, 0], [-2, -1, -0.0]], dtype=np.float32)
    t = S.table_spec(verts, np.array([[0, 1, 2], [3, 4, 5]]))
    assert t['lo'].tobytes() == np.array([[0, 0, 0], [-3, -1, 0]], dtype=np.float32).tobytes()          # +0.0 throughout
    assert t['hi'].tobytes() == np.array([[1, 1, 0], [-2, 0, 0]], dtype=np.float32).tobytes()
    assert t['diag2'].tolist() == [2.0, 2.0] and t['box_diag2'] == 16.0 + 4.0


def test_empty_and_all_invalid_meshes_come_back_as_given():
    verts = S.fins()[0]
    bad = np.array([[0, 0, 1], [-1, 2, 3], [1, 2, 5], [0, 1, 1 << 40]], dtype=np.int64)
    for v, f in ((verts, np.zeros((0, 3), np.int64)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), (verts, bad),
                 (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int64))):
        t = S.table_spec(v, f)
        assert t['leader'].shape == (0,) and t['box_diag2'] == 0.0 and (t['label'] == -1).all() and t['lo'].shape == (0, 3)
        out_v, out_f, info, kept = S.remove_spec(v, f, 1, 0.5, 1)
        assert out_v.tobytes() == v.tobytes() and out_f.tobytes() == f.tobytes() and kept == []
        assert info == {'faces_in': f.shape[0], 'faces_valid': 0, 'faces_out': f.shape[0], 'vertices_in': v.shape[0], 'vertices_out': v.shape[0],
                        'components': 0, 'components_kept': 0, 'largest_faces': 0, 'box_diag2': 0.0, 'min_faces': 1, 'min_diag_frac': 0.5,
                        'keep_largest': 1}
    # invalid faces among valid ones are dropped, whatever the rules
    out_v, out_f, info, _ = S.remove_spec(verts, np.concatenate([bad[:2], S.fins()[1], bad[2:]]), 1)
    assert out_f.tobytes() == S.fins()[1].tobytes() and info['faces_in'] == 7 and info['faces_valid'] == info['faces_out'] == 3


def test_remove_pieces_argument_rules():
    import torch
    from ppsurf_amd import pieces
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for name in ('min_faces', 'keep_largest'):
        for bad in (0, -1, 2 ** 31, 2.0, 2.5, float('nan'), '3', True, False):
            with pytest.raises(ValueError, match=name):
                pieces.remove_pieces(v, f, **{name: bad})
    for bad in (-0.1, 1.5, float('nan'), float('inf'), -float('inf'), '0.5', True, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(ValueError, match='min_diag_frac'):
            pieces.remove_pieces(v, f, min_diag_frac=bad)
    with pytest.raises(ValueError, match='no rule'):
        pieces.remove_pieces(v, f)
    with pytest.raises(ValueError, match='keep_largest'):                      # every rule is checked, not the first alone
        pieces.remove_pieces(v, f, 5, 0.5, 0)
    assert pieces._checked_rules(np.int64(2 ** 31 - 1), np.float32(0.5), 1) == (2 ** 31 - 1, 0.5, 1)
    assert pieces._checked_rules(None, 0, None) == (None, 0.0, None) and pieces._checked_rules(None, 1, None) == (None, 1.0, None)
    assert pieces._checked_rules(1, None, None) == (1, None, None)
    # good rules, CPU tensors: the device guard of the other mesh stages, after the parameters
    for fn in (lambda: pieces.remove_pieces(v, f, 1), lambda: pieces.remove_pieces(v, f, None, 0.5, 2), lambda: pieces.component_table(v, f),
               lambda: pieces.face_components(f, 3)):
        with pytest.raises(pieces.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(pieces.CpuTensorError, PpsError) and issubclass(pieces.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='remove_pieces: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        pieces.remove_pieces(v, f, keep_largest=1)


@pytest.mark.parametrize('argv', [['m.ply'], ['m.ply', 'o.ply'], ['m.ply', 'o.obj', '--min_faces', '5'], ['m.ply', 'o.ply', '--min_faces', '0'],
                                  ['m.ply', 'o.ply', '--min_faces', '-3'], ['m.ply', 'o.ply', '--min_faces', '2.5'],
                                  ['m.ply', 'o.ply', '--min_faces', '2147483648'], ['m.ply', 'o.ply', '--min_faces', 'True'],
                                  ['m.ply', 'o.ply', '--min_diag_frac', '1.5'], ['m.ply', 'o.ply', '--min_diag_frac', '-0.1'],
                                  ['m.ply', 'o.ply', '--min_diag_frac', 'nan'], ['m.ply', 'o.ply', '--min_diag_frac', 'tenth'],
                                  ['m.ply', 'o.ply', '--keep_largest', '0'], ['m.ply', 'o.ply', '--keep_largest', '1.0'],
                                  ['m.ply', 'o.ply', '--min_faces', '5', '--keep_largest', '0']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import pieces
    with pytest.raises(SystemExit) as e:
        pieces.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_pieces_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P, D = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_pieces_edge_keys'] == (I, [P, I64, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_pieces_hook'] == (I, [P, P, I64, P, I64, P, P])
    assert len([n for n in _lib.EXT_SIGNATURES if n.startswith('ppsx_pieces_')]) == 4                   # no compress of its own: labels.py's
    assert _lib.EXT_SIGNATURES['ppsx_pieces_stats'] == (I, [P, I64, P, I64, P, P, I64, P, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_pieces_select'] == (I, [P, P, P, P, I64, I, I64, I, D, I, I64, D, P, P])
    assert _lib.EXT_PARAMS['ppsx_pieces_edge_keys'] == ['faces', 'nf', 'nv', 'keys', 'stream']
    assert _lib.EXT_PARAMS['ppsx_pieces_hook'] == ['fa', 'fb', 'np', 'label', 'nf', 'changed', 'stream']
    assert _lib.EXT_PARAMS['ppsx_pieces_stats'] == ['verts', 'nv', 'faces', 'nf', 'label', 'cid', 'nc', 'count', 'lo', 'hi', 'stream']
    assert _lib.EXT_PARAMS['ppsx_pieces_select'] == ['count', 'lo', 'hi', 'rank', 'nc', 'has_min_faces', 'min_faces', 'has_min_diag_frac',
                                                     'min_diag_frac', 'has_keep_largest', 'keep_largest', 'box_diag2', 'keep', 'stream']
    assert not any(n.startswith('pps_pieces') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_pieces')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == ('topology.py' if name == 'ppsx_pieces_edge_keys' else 'pieces.py'), '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {'ppsx_pieces_edge_keys': 1, 'ppsx_pieces_hook': 1, 'ppsx_pieces_stats': 1,
                                                                   'ppsx_pieces_select': 1}
    assert 'pps_pieces.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)
