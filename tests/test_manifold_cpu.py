"""CPU tier of the manifold split: the numpy specification tests/manifold_spec.py against cases written out by hand,
its postconditions on every case, the argument rules of `split_nonmanifold`, `corner_fans` and of the command, the extension entries of
the C ABI with their call sites, and the shared label walk csrc/pps_labels.h."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import call_sites
import manifold_spec as S
import orient_spec
import pieces_spec

_cache = {}


def spec(name):
    """(verts, faces, verts out, faces out, info, parts) of a named case, computed once."""
    if name not in _cache:
        verts, faces = S.case(name)
        _cache[name] = (verts, faces) + S.split_spec(verts, faces)
    return _cache[name]


def test_a_bow_tie_by_hand():
    verts, faces, out_v, out_f, info, parts = spec('bow-tie')
    assert faces.tolist() == [[0, 1, 2], [0, 3, 4]] and S.pair_list(faces, 5)[0].shape[0] == 0          # no shared edge: every corner is a fan
    assert parts['label'].tolist() == [0, 1, 2, 3, 4, 5] and parts['fans'].tolist() == [2, 1, 1, 1, 1]
    assert parts['source'].tolist() == [0, 1, 2, 3, 4, 0] and out_f.tolist() == [[0, 1, 2], [5, 3, 4]] and not parts['same']
    assert out_v.tobytes() == verts[[0, 1, 2, 3, 4, 0]].tobytes()
    assert info == {'vertices_in': 5, 'vertices_out': 6, 'vertices_split': 1, 'max_fans': 2, 'faces_in': 2, 'faces_valid': 2,
                    'edges_border_in': 6, 'edges_border_out': 6, 'edges_manifold_in': 0, 'edges_manifold_out': 0, 'edges_nonmanifold_in': 0,
                    'closed_out': False}
    # the face order decides which copy keeps row 0
    assert S.split_spec(verts, faces[::-1])[1].tolist() == [[0, 3, 4], [5, 1, 2]]
    # an invalid row in front moves the corners, not the result
    _, faces_i, _, out_i, info_i, parts_i = spec('bow-tie invalid')
    assert faces_i.shape == (5, 3) and (parts_i['label'].reshape(-1, 3)[[0, 2, 4]] == -1).all() and info_i['faces_valid'] == 2
    assert parts_i['label'].reshape(-1, 3)[[1, 3]].tolist() == [[3, 4, 5], [9, 10, 11]]
    assert out_i[[1, 3]].tolist() == [[0, 1, 2], [5, 3, 4]] and np.array_equal(out_i[[0, 2, 4]], S.INVALID) and info_i['faces_in'] == 5


def test_a_book_of_three_pages_by_hand():
    verts, faces, out_v, out_f, info, parts = spec('book')
    assert faces.tolist() == [[0, 1, 2], [0, 1, 3], [0, 1, 4]] and S.owner_counts(faces, 5).tolist() == [3, 1, 1, 1, 1, 1, 1]
    # the leaders in ascending order: 0 and 1 keep the rows 0 and 1, 3 and 4 get the rows 5 and 6, 6 and 7 the rows 7 and 8
    assert parts['label'].tolist() == list(range(9)) and parts['fans'].tolist() == [3, 3, 1, 1, 1]
    assert parts['source'].tolist() == [0, 1, 2, 3, 4, 0, 1, 0, 1] and out_f.tolist() == [[0, 1, 2], [5, 6, 3], [7, 8, 4]]
    assert out_v.tobytes() == verts[parts['source']].tobytes()
    assert info == {'vertices_in': 5, 'vertices_out': 9, 'vertices_split': 2, 'max_fans': 3, 'faces_in': 3, 'faces_valid': 3,
                    'edges_border_in': 6, 'edges_border_out': 9, 'edges_manifold_in': 0, 'edges_manifold_out': 0, 'edges_nonmanifold_in': 1,
                    'closed_out': False}
    # two pages are a manifold edge: linked slot to slot when both run the spine the same way, crossed when one is turned
    assert S.fans_spec(faces[:2], 5).tolist() == [0, 1, 2, 0, 1, 5] and S.split_spec(verts, faces[:2])[3]['same']
    assert S.fans_spec(np.array([[0, 1, 2], [1, 0, 3]]), 5).tolist() == [0, 1, 2, 1, 0, 5]
    assert S.fans_spec(np.array([[0, 1, 2], [3, 1, 0]]), 5).tolist() == [0, 1, 2, 3, 1, 0]
    # two copies of one triangle are three pairs, linked corner by corner; three copies share no pair and fall apart
    assert S.fans_spec(np.array([[0, 1, 2], [1, 2, 0]]), 5).tolist() == [0, 1, 2, 1, 2, 0]
    assert S.split_spec(verts, np.array([[0, 1, 2]] * 3))[1].tolist() == [[0, 1, 2], [5, 6, 7], [8, 9, 10]]


def test_two_cubes_welded_along_an_edge_by_hand():
    verts, faces, out_v, out_f, info, parts = spec('welded edge')
    assert sorted(S.owner_counts(faces, 14).tolist()) == [2] * 34 + [4]
    shared = [i for i in range(14) if verts[i].tolist() in ([1.0, 1.0, 0.0], [1.0, 1.0, 1.0])]
    assert len(shared) == 2 and parts['fans'][shared].tolist() == [2, 2] and int(parts['fans'].sum()) == 16
    # the first cube's faces come first, so it keeps the rows; the second cube gets the two new ones
    assert parts['source'][:14].tolist() == list(range(14)) and sorted(parts['source'][14:].tolist()) == shared
    assert np.array_equal(out_f[:12], faces[:12]) and sorted(set(out_f[12:].reshape(-1).tolist()) - set(range(14))) == [14, 15]
    assert not set(out_f[:12].reshape(-1).tolist()) & set(out_f[12:].reshape(-1).tolist())                # the two solids share no row now
    assert info == {'vertices_in': 14, 'vertices_out': 16, 'vertices_split': 2, 'max_fans': 2, 'faces_in': 24, 'faces_valid': 24,
                    'edges_border_in': 0, 'edges_border_out': 0, 'edges_manifold_in': 34, 'edges_manifold_out': 36, 'edges_nonmanifold_in': 1,
                    'closed_out': True}
    # the stages downstream: two closed components, and every vertex is regular
    assert pieces_spec.labels_spec(out_f, 16).tolist() == [0] * 12 + [12] * 12
    assert orient_spec.orient_spec(verts, faces, 'outward')[2]['components_closed'] == 0
    assert orient_spec.orient_spec(out_v, out_f, 'outward')[2]['components_closed'] == 2


def test_what_the_issue_counted():
    assert spec('simplified sphere 6')[4]['edges_nonmanifold_in'] == 1
    assert sorted(S.owner_counts(S.case('simplified torus 8')[1], 134).tolist())[-8:] == [4] * 8 and spec('simplified torus 8')[4]['edges_nonmanifold_in'] == 8
    assert spec('simplified torus 8')[4]['edges_border_in'] == 0 and spec('simplified torus 8')[4]['edges_border_out'] == 32          # the cut closes nothing
    assert spec('simplified torus 4')[4]['edges_nonmanifold_in'] == 20 and set(S.owner_counts(S.case('simplified torus 4')[1], 30).tolist()) == {1, 2, 3, 4}
    assert spec('three tetrahedra')[4]['max_fans'] == 3 and spec('three tetrahedra')[4]['closed_out'] and spec('three tetrahedra')[4]['vertices_out'] == 12
    assert spec('welded vertex')[4]['vertices_split'] == 1 and spec('welded vertex')[4]['edges_nonmanifold_in'] == 0


@pytest.mark.parametrize('name', S.CASES)
def test_the_postconditions_hold_on_every_case(name):
    verts, faces, out_v, out_f, info, parts = spec(name)
    assert verts.dtype == np.float32 and faces.dtype == np.int64 and faces.ndim == 2 and faces.shape[1] == 3
    S.check(verts, faces, (out_v, out_f, parts['source']))
    assert parts['same'] == (info['vertices_split'] == 0) == (info['vertices_out'] == info['vertices_in'])
    if parts['same']:
        assert out_v is verts and out_f.tobytes() == faces.tobytes() and info['edges_nonmanifold_in'] == 0
    assert info['vertices_out'] - info['vertices_in'] == int((parts['fans'] - 1).clip(min=0).sum())
    # every fan names one vertex, and its leader is its smallest corner
    label, corner = parts['label'], faces.reshape(-1)
    live = label >= 0
    assert (label[live] <= np.arange(label.shape[0])[live]).all() and (label[label[live]] == label[live]).all()
    assert np.array_equal(corner[label[live]], corner[live])
    base, kind = name, ''
    for tail in (' invalid', ' shuffled'):
        if name.endswith(tail) and name[:-len(tail)] in S.BASES:
            base, kind = name[:-len(tail)], tail
    if base in S.CLOSED or base in ('moebius', 'fan300', 'empty', 'all invalid') or base.startswith('strip'):
        assert parts['same'], name
    if kind == ' invalid':                                             # the invalid rows change no count but faces_in
        want = dict(spec(base)[4], faces_in=info['faces_in'])
        assert info == want and faces.shape[0] == S.case(base)[1].shape[0] + 3
    if kind == ' shuffled':                                            # the order changes which copy keeps the row, no count
        assert info == spec(base)[4] and sorted(faces.tolist()) == sorted(S.case(base)[1].tolist())


def test_the_face_table_alone():
    f = np.array([[0, 1, 2], [0, 0, 1], [2, 1, 3], [-1, 2, 3], [1, 3, 0]], dtype=np.int64)
    label = np.array([0, 1, 2, 3, 4, 5, 2, 1, 8, 9, 10, 11, 1, 8, 0], dtype=np.int32)
    newrow = np.arange(15, dtype=np.int64)
    newrow[[0, 1, 2, 8]] = [0, 4, 2, 5]
    assert S.faces_spec(f, 4, label, newrow, 6).tolist() == [[0, 4, 2], [0, 0, 1], [2, 4, 5], [-1, 2, 3], [4, 5, 0]]
    assert S.faces_spec(f, 4, label, newrow, 5).tolist() == [[0, 4, 2], [0, 0, 1], [2, 1, 3], [-1, 2, 3], [1, 3, 0]]          # row 5 is out of range
    label[6] = -1                                                      # a negative label: the entry stays
    label[12] = 15                                                     # no corner: the face is copied
    assert S.faces_spec(f, 4, label, newrow, 6).tolist() == [[0, 4, 2], [0, 0, 1], [2, 4, 5], [-1, 2, 3], [1, 3, 0]]


def test_argument_rules():
    import torch
    from ppsurf_amd import manifold
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for fn in (lambda: manifold.split_nonmanifold(v, f), lambda: manifold.split_nonmanifold(v, f, return_source=True), lambda: manifold.corner_fans(f, 3)):
        with pytest.raises(manifold.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(manifold.CpuTensorError, PpsError) and issubclass(manifold.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='split_nonmanifold: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        manifold.split_nonmanifold(v, f)
    # one int32 label per corner
    manifold._checked_corners('x', (2 ** 31 - 1) // 3)
    for nf in ((2 ** 31 - 1) // 3 + 1, 2 ** 31 - 1):
        with pytest.raises(ValueError, match='x: at most'):
            manifold._checked_corners('x', nf)
    assert manifold.MAX_COUNT == 2 ** 31 - 1


@pytest.mark.parametrize('argv', [['m.ply'], [], ['m.ply', 'o.obj'], ['m.ply', 'o.ply', 'p.ply'], ['m.ply', 'o.ply', '--eps', '0.5'],
                                  ['m.ply', 'o.ply', '--mode', 'outward'], ['m.ply', 'o.stl']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import manifold
    with pytest.raises(SystemExit) as e:
        manifold.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.EXT_SIGNATURES['ppsx_manifold_hook'] == (I, [P, I64, I64, P, P, P, P, I64, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_manifold_faces'] == (I, [P, I64, I64, P, P, I64, P, P])
    assert _lib.EXT_PARAMS['ppsx_manifold_hook'] == ['faces', 'nf', 'nv', 'fa', 'fb', 'ea', 'eb', 'np', 'label', 'changed', 'stream']
    assert _lib.EXT_PARAMS['ppsx_manifold_faces'] == ['faces', 'nf', 'nv', 'label', 'newrow', 'nv_out', 'out', 'stream']
    assert not any(n.startswith('pps_manifold') for n in _lib.SIGNATURES)                                # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_manifold')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'manifold.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {'ppsx_manifold_hook': 1, 'ppsx_manifold_faces': 1}
    # manifold.py names no other entry: the keys come through topology.py, the loop and the compress launch through labels.py, which
    # holds the one call of the one compress entry
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'manifold.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(sites) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert [path for path, _, _ in call_sites.ext_call_sites('ppsx_labels_compress')['ppsx_labels_compress']] == ['labels.py']
    # no stage holds a loop of its own: the flag is zeroed in labels.fixed_point and nowhere else in the package
    package = os.path.join(call_sites.REPO, 'ppsurf_amd')
    assert [os.path.basename(p) for p in sorted(glob.glob(os.path.join(package, '**', '*.py'), recursive=True))
            if 'changed.zero_()' in open(p).read()] == ['labels.py']
    assert 'pps_manifold.hip' in build.SOURCES and 'pps_labels.h' in build.HEADERS
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)


def test_the_label_walk_lives_in_one_header():
    csrc = os.path.join(call_sites.REPO, 'ppsurf_amd', 'csrc')
    defines = re.compile(r'\b(?:int|void)\s+(load_label|walk_end|join_ends)\s*\(')
    users = []
    for path in sorted(glob.glob(os.path.join(csrc, '*.h')) + glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.cpp'))):
        text = open(path).read()
        name = os.path.basename(path)
        if name == 'pps_labels.h':
            assert sorted(defines.findall(text)) == ['join_ends', 'load_label', 'walk_end']
            assert '__hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)' in text
        else:
            assert not defines.findall(text), name
            if '#include "pps_labels.h"' in text:
                users.append(name)
                # every user walks through the header: directly, or through the shared join (weld, manifold)
                assert ('walk_end(label' in text or 'join_ends(label' in text) and 'load_label(label' in text, name
    assert users == ['pps_labels.hip', 'pps_manifold.hip', 'pps_pieces.hip', 'pps_weld.hip']
