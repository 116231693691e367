"""CPU tier of the orientation stage: the numpy specification tests/orient_spec.py against meshes written out by hand,
seeded scrambles of outward meshes, non-orientable and open meshes, the order of the volume sum, the argument rules of `orient_mesh` and of
the command, and the extension entries of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import call_sites
import orient_spec as S
import pieces_spec

_cache = {}


def spec(name, mode):
    """(verts, faces as given, faces out, info, table) of a named case, computed once."""
    if (name, mode) not in _cache:
        verts, faces = S.case(name)
        _, out, info, table = S.orient_spec(verts, faces, mode)
        _cache[(name, mode)] = (verts, faces, out, info, table)
    return _cache[(name, mode)]


def test_a_tetrahedron_by_hand():
    verts, faces = S.tetra()
    assert S.signed_volumes(verts, faces) == {0: 1.0}
    _, out, info, table = S.orient_spec(verts, faces, 'outward')
    assert out.tobytes() == faces.tobytes() and out is not faces
    assert info == {'faces_in': 4, 'faces_valid': 4, 'faces_flipped': 0, 'components': 1, 'components_closed': 1, 'components_open': 0,
                    'components_non_orientable': 0, 'faces_non_orientable': 0, 'components_flipped': 0, 'zero_volume': 0, 'mode': 'outward'}
    assert table[0]['vol'] == 1.0 and table[0]['pairs'] == 6 and table[0]['turn'] == 1
    _, out, info, _ = S.orient_spec(verts, faces, 'inward')
    assert out.tolist() == [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]] and info['faces_flipped'] == 4 and info['components_flipped'] == 1
    # one face turned: exactly that face turns back; inward turns the other three
    one = S.turned(faces, [2])
    _, out, info, table = S.orient_spec(verts, one, 'outward')
    assert out.tobytes() == faces.tobytes() and info['faces_flipped'] == 1 and info['components_flipped'] == 0 and table[0]['ones'] == 1
    _, out, info, _ = S.orient_spec(verts, one, 'inward')
    assert out.tobytes() == S.turned(faces).tobytes() and info['faces_flipped'] == 3 and info['components_flipped'] == 1
    assert S.orient_spec(verts, one, 'majority')[1].tobytes() == faces.tobytes()
    # the leader turned: outward still finds the outside, majority follows the three
    lead = S.turned(faces, [0])
    assert S.orient_spec(verts, lead, 'outward')[1].tobytes() == faces.tobytes()
    assert S.orient_spec(verts, lead, 'majority')[1].tobytes() == faces.tobytes()
    assert S.orient_spec(verts, S.turned(faces, [1, 2, 3]), 'majority')[1].tobytes() == S.turned(faces).tobytes()


def test_two_copies_of_one_triangle():
    verts, same = S.case('twins same')
    fa, fb, ea, eb, s = S.pair_list(same, 4)
    assert sorted(zip(fa.tolist(), fb.tolist(), ea.tolist(), eb.tolist())) == [(0, 1, 0, 0), (0, 1, 1, 1), (0, 1, 2, 2)] and s.tolist() == [1, 1, 1]
    for mode in S.MODES:
        _, out, info, table = S.orient_spec(verts, same, mode)
        assert out.tolist() == [[0, 1, 2], [0, 2, 1]], mode                 # the second turns: a tie, so the leader keeps its winding
        assert info['components'] == 1 and info['components_closed'] == 1 and info['faces_flipped'] == 1 and info['components_flipped'] == 0
        assert info['zero_volume'] == (0 if mode == 'majority' else 1) and table[0]['vol'] in (None, 0.0)
    verts, opposite = S.case('twins opposite')
    fa, fb, ea, eb, s = S.pair_list(opposite, 4)
    assert sorted(zip(ea.tolist(), eb.tolist())) == [(0, 2), (1, 1), (2, 0)] and s.tolist() == [0, 0, 0]
    for mode in S.MODES:
        _, out, info, _ = S.orient_spec(verts, opposite, mode)
        assert out.tobytes() == opposite.tobytes() and info['faces_flipped'] == 0 and info['components_closed'] == 1
        assert info['zero_volume'] == (0 if mode == 'majority' else 1)


@pytest.mark.parametrize('name', S.CLOSED)
def test_seeded_scrambles_come_back_outward(name):
    verts, good = S.closed_mesh(name)
    scrambled, mask = S.scramble(good, S.SEEDS[name])
    assert 0.4 < mask.mean() < 0.6 and S.valid_faces(good, verts.shape[0]).all()
    comps = {'sphere': 1, 'cube': 1, 'torus': 1, 'scene': 6}[name]
    assert all(vol > 0 for vol in S.signed_volumes(verts, good).values()) and len(S.signed_volumes(verts, good)) == comps
    _, faces, out, info, table = spec(name, 'outward')
    assert faces.tobytes() == scrambled.tobytes() and out.tobytes() == good.tobytes()
    assert S.pair_list(out, verts.shape[0])[4].sum() == 0 and S.pair_list(faces, verts.shape[0])[4].sum() > 0
    assert all(vol > 0 for vol in S.signed_volumes(verts, out).values())
    assert info['components'] == info['components_closed'] == comps and info['components_open'] == info['components_non_orientable'] == 0
    assert info['faces_flipped'] == int(mask.sum()) and info['zero_volume'] == 0 and info['faces_valid'] == good.shape[0]
    assert info['components_flipped'] == int(mask[[row['leader'] for row in table]].sum())
    assert spec(name, 'inward')[2].tobytes() == S.turned(good).tobytes()
    assert all(vol < 0 for vol in S.signed_volumes(verts, spec(name, 'inward')[2]).values())
    # the flips do not depend on the mode, and the labels are those of the pieces
    label, flip, bad = S.flips_spec(faces, verts.shape[0])
    assert np.array_equal(label, pieces_spec.labels_spec(faces, verts.shape[0])) and not bad.any()
    assert np.array_equal(flip.astype(bool), mask ^ mask[label])


def test_non_orientable_components_come_back_as_given():
    for name, closed in (('moebius', False), ('klein', True)):
        verts, faces = S.case(name)
        assert S.valid_faces(faces, verts.shape[0]).all()
        for mode in S.MODES:
            _, out, info, table = S.orient_spec(verts, faces, mode)
            assert out.tobytes() == faces.tobytes() and info['faces_flipped'] == 0 and info['components'] == 1
            assert info['components_non_orientable'] == 1 and info['faces_non_orientable'] == faces.shape[0] and info['zero_volume'] == 0
            assert info['components_closed'] == int(closed) and info['components_open'] == int(not closed) and table[0]['turn'] == 0
    assert S.case('klein')[1].shape == (256, 3) and S.case('moebius')[1].shape == (96, 3)
    # the torus on the same vertices is orientable: the seam alone makes the difference
    assert not S.flips_spec(S.torus()[1], 128)[2].any()
    sphere_v, sphere_good = S.sphere()
    for name in ('klein and sphere', 'moebius and sphere'):
        verts, faces = S.case(name)
        other = S.case(name.split(' ')[0])[1]
        _, out, info, _ = S.orient_spec(verts, faces, 'outward')
        k = other.shape[0]
        assert out[:k].tobytes() == other.tobytes() and (out[k:] - out[k:].min()).tobytes() == sphere_good.tobytes()
        assert info['components'] == 2 and info['components_non_orientable'] == 1 and info['faces_non_orientable'] == k
        assert info['faces_flipped'] == int(S.scramble(sphere_good, S.SEEDS['sphere'])[1].sum())


def test_open_meshes_take_the_majority():
    verts, good = S.flat()
    faces, mask = S.scramble(good, 25, 0.3)
    assert good.shape == (288, 3) and 0.2 < mask.mean() < 0.4 and S.case('flat 30')[1].tobytes() == faces.tobytes()
    for mode in S.MODES:
        _, out, info, _ = S.orient_spec(verts, faces, mode)
        assert out.tobytes() == good.tobytes() and info['components_open'] == 1 and info['components_closed'] == 0
        assert info['faces_flipped'] == int(mask.sum()) and info['zero_volume'] == 0 and info['components_flipped'] == int(mask[0])
    # an exact tie: the leader keeps its winding, whichever it is
    for leader_turned in (False, True):
        verts, faces = S.flat_tie(leader_turned)
        assert int((faces != good).any(axis=1).sum()) == 144 and bool((faces[0] != good[0]).any()) == leader_turned
        for mode in S.MODES:
            _, out, info, _ = S.orient_spec(verts, faces, mode)
            assert out.tobytes() == (S.turned(good) if leader_turned else good).tobytes()
            assert info['faces_flipped'] == 144 and info['components_flipped'] == 0
    # a strip (i, i + 1, i + 2): every pair runs its edge the same way, every other face turns
    verts, faces = pieces_spec.strip(1025)
    _, out, info, _ = S.orient_spec(verts, faces, 'outward')
    assert out.tobytes() == S.turned(faces, np.arange(1, 1025, 2)).tobytes() and info['faces_flipped'] == 512
    for order in ('reversed', 'permuted'):
        verts, faces = S.case('strip ' + order)
        label, flip, bad = S.flips_spec(faces, verts.shape[0])
        assert (label == 0).all() and not bad.any() and np.array_equal(flip, (faces[:, 0] - faces[0, 0]) % 2)
    # an edge with three owners joins nothing: three components of one face
    assert S.orient_spec(*S.case('fins'))[2]['components'] == 3 and S.orient_spec(*S.case('fins'))[2]['faces_flipped'] == 0


def test_rows_are_kept_as_given():
    verts, faces = S.case('sphere invalid')
    plain = S.case('sphere')[1]
    assert faces.shape == (1283, 3) and [faces[k].tolist() for k in (3, 300, 301)] == S.INVALID.tolist()
    keep = np.ones(1283, dtype=bool)
    keep[[3, 300, 301]] = False
    assert faces[keep].tobytes() == plain.tobytes()
    for mode in S.MODES:
        _, out, info, _ = S.orient_spec(verts, faces, mode)
        assert out[~keep].tobytes() == S.INVALID.tobytes() and out[keep].tobytes() == S.orient_spec(verts, plain, mode)[1].tobytes()
        assert info['faces_in'] == 1283 and info['faces_valid'] == 1280
        again = S.orient_spec(verts, faces, mode)
        assert again[1].tobytes() == out.tobytes() and again[2] == info
    # nothing to turn, nothing valid, nothing at all
    verts, good = S.case('sphere coherent')
    assert S.orient_spec(verts, good, 'outward')[1].tobytes() == good.tobytes() and S.orient_spec(verts, good, 'outward')[2]['faces_flipped'] == 0
    assert S.orient_spec(*S.case('sphere inside out'))[1].tobytes() == good.tobytes()
    assert S.orient_spec(*S.case('sphere inside out'))[2]['components_flipped'] == 1
    for name in ('empty', 'all invalid'):
        verts, faces = S.case(name)
        _, out, info, table = S.orient_spec(verts, faces, 'outward')
        assert out.tobytes() == faces.tobytes() and table == [] and info['faces_valid'] == 0 and info['components'] == 0 and info['faces_flipped'] == 0
    assert len(S.CASES) == len(set(S.CASES))
    for name in S.CASES:
        verts, faces = S.case(name)
        assert verts.dtype == np.float32 and faces.dtype == np.int64 and faces.ndim == 2 and faces.shape[1] == 3, name


def test_the_order_of_the_sum_is_what_is_stated_and_matters():
    rng = np.random.default_rng(41)
    t = rng.standard_normal(257) * np.exp(rng.uniform(-8, 8, 257))
    # the stated order, once more from the definition: lanes of four, the strides, the blocks
    lanes = np.zeros(64)
    for l in range(64):
        acc = 0.0
        for j in range(4):
            acc = acc + t[4 * l + j]
        lanes[l] = acc
    for stride in (1, 2, 4, 8, 16, 32):
        for l in range(0, 64, 2 * stride):
            lanes[l] = lanes[l] + lanes[l + stride]
    second = ((0.0 + t[256]) + 0.0) + 0.0 + 0.0
    want = (0.0 + lanes[0]) + second
    assert S.ordered_sum(t) == want and S.block_sums(t).tolist() == [lanes[0], t[256]]
    assert S.ordered_sum(t) != np.sum(t) and abs(S.ordered_sum(t) - np.sum(t)) <= 1e-12 * np.abs(t).sum()
    assert S.ordered_sum(t[:256]) == lanes[0] and S.ordered_sum([]) == 0.0 and S.ordered_sum([-0.0]).tobytes() == np.float64(0.0).tobytes()
    # on a component of 257 faces: a fan around one vertex, closed by a second hub below it
    verts = np.random.default_rng(42).standard_normal((700, 3)).astype(np.float32)
    i = np.arange(257)
    faces = np.stack([i * 0, 1 + i, 1 + (i + 1) % 257], axis=1).astype(np.int64)
    none = np.zeros(257, dtype=np.uint8)
    terms = S.volume_terms(verts, faces, i, none, 0)
    assert terms.dtype == np.float64 and (terms == 0).all()                 # R is the hub: every face holds it
    faces = faces[:, [1, 2, 0]]                                           # R = vertex 1 now
    terms = S.volume_terms(verts, faces, i, none, 0)
    assert S.ordered_sum(terms) == S.ordered_sum(terms[:256]) + terms[256] and S.ordered_sum(terms) != np.sum(terms)
    flip = (i % 3 == 0).astype(np.uint8)
    assert np.array_equal(S.volume_terms(verts, faces, i, flip, 0), np.where(flip == 1, -terms, terms))


def test_orient_mesh_argument_rules():
    import torch
    from ppsurf_amd import orient
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in ('Outward', 'out', '', None, 1, True, b'outward', ['outward']):
        with pytest.raises(ValueError, match='mode'):
            orient.orient_mesh(v, f, bad)
    assert orient.MODES == S.MODES and orient.SUM_BLOCK == S.BLOCK
    # a good mode, CPU tensors: the device guard of the other mesh stages, after the parameters
    for fn in (lambda: orient.orient_mesh(v, f), lambda: orient.orient_mesh(v, f, 'majority'), lambda: orient.face_flips(f, 3)):
        with pytest.raises(orient.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(orient.CpuTensorError, PpsError) and issubclass(orient.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='orient_mesh: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        orient.orient_mesh(v, f, mode='inward')


@pytest.mark.parametrize('argv', [['m.ply'], [], ['m.ply', 'o.obj'], ['m.ply', 'o.ply', '--mode', 'up'], ['m.ply', 'o.ply', '--mode'],
                                  ['m.ply', 'o.ply', '--mode', 'Outward'], ['m.ply', 'o.ply', '--min_faces', '5']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import orient
    with pytest.raises(SystemExit) as e:
        orient.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_orient_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.EXT_SIGNATURES['ppsx_orient_pair_sign'] == (I, [P, I64, P, P, P, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_orient_hook'] == (I, [P, P, P, I64, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_orient_compress'] == (I, [P, I64, P])
    assert _lib.EXT_SIGNATURES['ppsx_orient_check'] == (I, [P, P, P, I64, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_orient_block_sums'] == (I, [P, I64, P, I64, P, P, I64, P, P, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_orient_comp_sums'] == (I, [P, I64, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_orient_apply'] == (I, [P, I64, P, P, P, I64, P, P])
    assert _lib.EXT_PARAMS['ppsx_orient_pair_sign'] == ['faces', 'nf', 'fa', 'fb', 'ea', 'eb', 'np', 'sign', 'stream']
    assert _lib.EXT_PARAMS['ppsx_orient_hook'] == ['fa', 'fb', 'sign', 'np', 'word', 'nf', 'changed', 'stream']
    assert _lib.EXT_PARAMS['ppsx_orient_compress'] == ['word', 'nf', 'stream']
    assert _lib.EXT_PARAMS['ppsx_orient_check'] == ['fa', 'fb', 'sign', 'np', 'word', 'nf', 'bad', 'stream']
    assert _lib.EXT_PARAMS['ppsx_orient_block_sums'] == ['verts', 'nv', 'faces', 'nf', 'flip', 'list', 'nl', 'first', 'count', 'lead', 'nb', 'sums',
                                                         'stream']
    assert _lib.EXT_PARAMS['ppsx_orient_comp_sums'] == ['sums', 'nb', 'start', 'nc', 'vol', 'stream']
    assert _lib.EXT_PARAMS['ppsx_orient_apply'] == ['faces', 'nf', 'cid', 'flip', 'turn', 'nc', 'out', 'stream']
    sites = call_sites.ext_call_sites('ppsx_orient')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'orient.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {n: 1 for n in _lib.EXT_PARAMS if n.startswith('ppsx_orient_')} and len(sites) == 7
    # orient.py calls no other stage's entries; the pairs come through the topology layer, which holds the one call of the key entry
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'orient.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(sites) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert [path for path, _, _ in call_sites.ext_call_sites('ppsx_pieces_edge_keys')['ppsx_pieces_edge_keys']] == ['topology.py']
    assert 'pps_orient.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)
