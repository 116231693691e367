"""CPU tier of the weld stage: the numpy specification tests/weld_spec.py against cases written out by hand and against
seeded soups of indexed meshes, `weld.read_input` on the two STL flavours, the argument rules of `weld_mesh`, `vertex_clusters` and of the
command, and the extension entries of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import call_sites
import orient_spec
import weld_spec as S

_cache = {}


def spec(name):
    """(verts, faces, eps as given, verts out, faces out, info, parts) of a named case, computed once."""
    if name not in _cache:
        verts, faces, eps = S.case(name)
        _cache[name] = (verts, faces, eps) + S.weld_spec(verts, faces, eps, name in S.DROP)
    return _cache[name]


def test_a_tetrahedron_soup_by_hand():
    verts, faces, eps, out_v, out_f, info, parts = spec('tetra soup')
    tv, tf = orient_spec.tetra()                                       # faces (0 2 1) (0 1 3) (0 3 2) (1 2 3): first seen in the order 0 2 1 3
    assert verts.shape == (12, 3) and faces.tolist() == np.arange(12).reshape(4, 3).tolist() and eps == 0.0
    assert parts['leader'].tolist() == [0, 1, 2, 0, 2, 5, 0, 5, 1, 2, 1, 5] and parts['rows'].tolist() == [0, 1, 2, 5]
    assert out_v.tobytes() == tv[[0, 2, 1, 3]].tobytes() and out_f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 1], [2, 1, 3]]
    assert out_v[out_f].tobytes() == tv[tf].tobytes() and parts['code'].tolist() == [0, 0, 0, 0] and not parts['same']
    assert info == {'vertices_in': 12, 'vertices_out': 4, 'clusters_merged': 4, 'largest_cluster': 3, 'faces_in': 4, 'faces_invalid': 0,
                    'faces_collapsed': 0, 'faces_duplicate': 0, 'faces_out': 4, 'eps': 0.0, 'drop_duplicates': False}
    # invalid rows interleaved: they leave, the rest is the same mesh
    _, faces7, _, out_v7, out_f7, info7, parts7 = spec('tetra soup invalid')
    assert faces7.shape == (7, 3) and parts7['code'].tolist() == [1, 0, 0, 1, 0, 0, 1] and info7['faces_invalid'] == 3 and info7['faces_out'] == 4
    assert out_v7.tobytes() == out_v.tobytes() and out_f7.tobytes() == out_f.tobytes()


def test_the_link_is_exact():
    assert spec('signed zeros')[6]['leader'].tolist() == [0, 0, 0, 3]                       # -0.0 equals +0.0
    assert spec('signed zeros')[3].tobytes() == spec('signed zeros')[0][[0, 3]].tobytes()      # the leader's bytes, not a canonical zero
    # p = (0, 0, 0), q = (3, 4, 0): d2 == eps2 == 25 exactly
    assert spec('3-4-5 linked')[2] == 5.0 and spec('3-4-5 linked')[6]['leader'].tolist() == [0, 0]
    assert spec('3-4-5 apart')[2] == np.nextafter(5.0, 0.0) < 5.0 and spec('3-4-5 apart')[6]['leader'].tolist() == [0, 1]
    assert spec('3-4-5 apart')[6]['same']
    i, j = S.linked_pairs(np.array([[0, 0, 0], [3, 4, 0], [3, 4, 0]], dtype=np.float32), 0.0)
    assert (i.tolist(), j.tolist()) == ([2], [1])
    # symmetric: the rows swapped give the same clusters
    pts = S.case('cloud')[0]
    assert np.array_equal(S.clusters_spec(pts[::-1], 1.0), np.zeros(700, dtype=np.int32)) and spec('cloud eps')[5]['largest_cluster'] == 700


def test_single_linkage_chains():
    verts, faces, eps, out_v, out_f, info, parts = spec('chain 5')
    gaps = np.diff(verts[:, 0].astype(np.float64))
    assert eps == S.CHAIN_EPS and (gaps < eps).all() and (gaps > 0.89 * eps).all() and verts[4, 0] - verts[0, 0] > 3.59 * eps
    assert S.linked_pairs(verts, eps)[0].shape[0] == 4                                       # only the neighbours are linked
    assert parts['leader'].tolist() == [0] * 5 and info['largest_cluster'] == 5 and out_v.tobytes() == verts[:1].tobytes()
    assert parts['code'].tolist() == [2] and info['faces_collapsed'] == 1 and out_f.shape == (0, 3)
    for name in ('chain 1025', 'chain 1025 reversed', 'chain 1025 shuffled'):
        verts, _, eps = S.case(name)
        assert S.linked_pairs(verts, eps)[0].shape[0] == 1024 and (spec(name)[6]['leader'] == 0).all(), name
    assert sorted(S.case('chain 1025 shuffled')[0][:, 0].tolist()) == S.case('chain 1025')[0][:, 0].tolist()


def test_face_codes_duplicates_and_unreferenced_leaders():
    verts, faces, eps, out_v, out_f, info, parts = spec('collapsed')
    assert parts['leader'].tolist() == [0, 1, 2, 3, 1] and parts['code'].tolist() == [0, 2, 0] and out_f.tolist() == [[0, 1, 2], [0, 1, 3]]
    assert info['faces_collapsed'] == 1 and info['clusters_merged'] == 1 and info['vertices_out'] == 4
    # the faces kernel's table on its own: a newrow entry out of range is code 1, and only the kept rows are renumbered
    f = np.array([[0, 1, 2], [0, 1, 3], [2, 2, 1], [0, 4, 1], [1, 2, 3]], dtype=np.int64)
    out, code = S.faces_spec(f, 4, np.array([0, 0, 1, 4], dtype=np.int64))
    assert code.tolist() == [2, 1, 1, 1, 1] and out.tobytes() == f.tobytes()
    out, code = S.faces_spec(f, 4, np.array([3, 0, 1, 2], dtype=np.int64))
    assert code.tolist() == [0, 0, 1, 1, 0] and out.tolist() == [[3, 0, 1], [3, 0, 2], [2, 2, 1], [0, 4, 1], [0, 1, 2]]
    assert S.faces_spec(f, 0, np.zeros(0, dtype=np.int64))[1].tolist() == [1] * 5
    # three copies of a triangle: rotated, then mirrored
    verts, faces, _, out_v, out_f, info, _ = spec('twins')
    assert out_f.tolist() == [[0, 1, 2], [1, 2, 0], [0, 2, 1]] and info['faces_duplicate'] == 0 and info['faces_out'] == 3
    _, _, _, drop_v, drop_f, drop_info, _ = spec('twins dropped')
    assert drop_f.tolist() == [[0, 1, 2]] and drop_info['faces_duplicate'] == 2 and drop_info['drop_duplicates'] is True and drop_v.tobytes() == out_v.tobytes()
    assert S.weld_spec(verts[:6], faces[:2], 0.0, True)[1].tolist() == [[0, 1, 2]]          # the same winding alone
    assert S.weld_spec(verts[[0, 1, 2, 6, 7, 8]], faces[:2], 0.0, True)[1].tolist() == [[0, 1, 2]]          # the opposite winding alone
    # a leader that no kept face references stays: the weld deletes duplicates and nothing else
    verts, faces, _, out_v, out_f, info, parts = spec('unreferenced')
    assert parts['rows'].tolist() == [0, 1, 2, 3, 4] and out_v.tobytes() == verts[:5].tobytes() and out_f.tolist() == [[0, 1, 2], [0, 2, 1]]
    assert info['clusters_merged'] == 2 and info['vertices_out'] == 5
    # a bare cloud loses its duplicates
    pts, _, _, out_v, _, info, parts = spec('cloud')
    assert out_v.shape[0] == np.unique(pts, axis=0).shape[0] == info['vertices_out'] == 209 and info['faces_out'] == 0
    assert np.array_equal(np.unique(out_v, axis=0), np.unique(pts, axis=0)) and (np.diff(parts['rows']) > 0).all()


def test_the_same_arrays_come_back_when_there_is_nothing_to_do():
    for name in ('empty', 'all invalid', 'welded sphere', 'single', '3-4-5 apart'):
        verts, faces, eps, out_v, out_f, info, parts = spec(name)
        assert parts['same'] and out_v.tobytes() == verts.tobytes() and out_f.tobytes() == faces.tobytes(), name
        assert info['vertices_out'] == verts.shape[0] and info['faces_out'] == faces.shape[0] and info['clusters_merged'] == 0, name
    assert spec('all invalid')[5]['faces_invalid'] == 3 and spec('empty')[5]['largest_cluster'] == 0 and spec('single')[5]['largest_cluster'] == 1
    # one invalid face beside valid ones, a merge beside invalid ones only, a dropped duplicate: not the same
    assert not spec('welded sphere invalid')[6]['same'] and spec('welded sphere invalid')[4].tobytes() == spec('welded sphere')[1].tobytes()
    assert not spec('all invalid merged')[6]['same'] and spec('all invalid merged')[4].shape == (0, 3) and spec('all invalid merged')[3].shape == (1, 3)
    verts, faces = orient_spec.tetra()
    twice = np.concatenate([faces, faces[:1, [1, 2, 0]]])
    assert S.weld_spec(verts, twice, 0.0, False)[3]['same'] and not S.weld_spec(verts, twice, 0.0, True)[3]['same']
    assert S.weld_spec(verts, twice, 0.0, True)[1].tobytes() == faces.tobytes()
    assert len(S.CASES) == len(set(S.CASES)) and set(S.DROP) <= set(S.CASES)
    for name in S.CASES:
        verts, faces, eps = S.case(name)
        assert verts.dtype == np.float32 and faces.dtype == np.int64 and faces.ndim == 2 and faces.shape[1] == 3 and eps >= 0, name


@pytest.mark.parametrize('name', ['sphere', 'cube', 'torus'])
def test_seeded_soups_weld_back_to_the_indexed_mesh(name):
    verts, faces = orient_spec.case(name)                              # the scrambled winding: the weld leaves it alone
    nv = verts.shape[0]
    assert np.unique(verts, axis=0).shape[0] == nv and np.unique(faces).shape[0] == nv
    sv, sf, first = S.soup(verts, faces, S.SEEDS[name + ' soup'])
    assert sv.shape == (3 * faces.shape[0], 3) and sorted(sf.reshape(-1).tolist()) == list(range(sv.shape[0])) and sv[sf].tobytes() == verts[faces].tobytes()
    assert not (np.diff(sf.reshape(-1)) == 1).all()                    # shuffled
    _, _, eps, out_v, out_f, info, parts = spec(name + ' soup')
    want_v, want_f = S.welded_soup(verts, faces, first)
    assert eps == 0.0 and out_v.tobytes() == want_v.tobytes() and out_f.tobytes() == want_f.tobytes()
    assert out_v[out_f].tobytes() == verts[faces].tobytes() and parts['rows'].tolist() == sorted(first.tolist())
    assert info['vertices_in'] == 3 * faces.shape[0] and info['vertices_out'] == info['clusters_merged'] == nv and info['faces_out'] == faces.shape[0]
    assert info['faces_invalid'] == info['faces_collapsed'] == 0
    # the soup has no pair at all; welded, every edge has its two owners, and the outward orientation leaves every pair coherent
    assert orient_spec.pair_list(sf, sv.shape[0])[0].shape[0] == 0 and 2 * orient_spec.pair_list(out_f, nv)[0].shape[0] == 3 * faces.shape[0]
    _, oriented, oinfo, _ = orient_spec.orient_spec(out_v, out_f, 'outward')
    assert orient_spec.pair_list(out_f, nv)[4].sum() > 0 and orient_spec.pair_list(oriented, nv)[4].sum() == 0
    assert oinfo['components'] == oinfo['components_closed'] == 1 and all(vol > 0 for vol in orient_spec.signed_volumes(out_v, oriented).values())
    if name == 'sphere':                                               # copies moved by a tenth of eps: the same clusters, the leaders' bytes
        jv, jf, jeps, jout_v, jout_f, jinfo, jparts = spec('sphere soup jitter')
        assert jeps == 1.0e-3 and not np.array_equal(jv, sv) and jf.tobytes() == sf.tobytes() and jout_f.tobytes() == out_f.tobytes()
        assert np.array_equal(jparts['leader'], parts['leader']) and jout_v.tobytes() == jv[parts['rows']].tobytes()


@pytest.mark.parametrize('ascii_', [False, True])
def test_read_input_reads_an_stl_as_a_soup(tmp_path, ascii_):
    from ppsurf_amd import meshio, weld
    path = str(tmp_path / 'tetra.STL')
    corners = S.tetra_stl(path, ascii_)
    verts, faces, colors, double = weld.read_input(path)
    assert verts.dtype == np.float64 and verts.shape == (12, 3) and np.array_equal(verts, corners.astype(np.float64))
    assert faces.dtype == np.int64 and faces.tolist() == np.arange(12).reshape(4, 3).tolist() and colors is None and double is False
    assert S.weld_spec(verts, faces)[1].tobytes() == spec('tetra soup')[4].tobytes()
    with pytest.raises(ValueError, match='unsupported mesh file'):     # the readers of the other stages still refuse it
        meshio.read_mesh_file(path)
    # a PLY goes through meshio.read_mesh_file
    ply = str(tmp_path / 'tetra.ply')
    tv, tf = orient_spec.tetra()
    rgb = np.arange(12, dtype=np.uint8).reshape(4, 3)
    meshio.write_ply_mesh_colored(ply, tv.astype(np.float64), tf, rgb, double=True)
    verts, faces, colors, double = weld.read_input(ply)
    assert np.array_equal(verts, tv) and np.array_equal(faces, tf) and np.array_equal(colors, rgb) and double is True


def test_weld_mesh_argument_rules():
    import torch
    from ppsurf_amd import weld
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in (True, False, None, '0', [0.0], float('nan'), float('inf'), -1e-30, -1, np.float32('nan'), 1j):
        with pytest.raises(ValueError, match='eps'):
            weld.weld_mesh(v, f, bad)
        with pytest.raises(ValueError, match='eps'):
            weld.vertex_clusters(v, bad)
    # a good eps, CPU tensors: the device guard of the other mesh stages, after the parameter
    for fn in (lambda: weld.weld_mesh(v, f), lambda: weld.weld_mesh(v, f, 0.5, True), lambda: weld.weld_mesh(v, f, np.float32(1)),
               lambda: weld.weld_mesh(v, f, 2), lambda: weld.vertex_clusters(v), lambda: weld.vertex_clusters(v, eps=0.25)):
        with pytest.raises(weld.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(weld.CpuTensorError, PpsError) and issubclass(weld.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='weld_mesh: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        weld.weld_mesh(v, f, eps=0.0, drop_duplicates=True)
    assert weld.H_FLOOR > 0 and 1.0 / np.float32(weld.H_FLOOR) < 3.0e38 and np.float32(weld.H_FLOOR) == weld.H_FLOOR


@pytest.mark.parametrize('argv', [['m.ply'], [], ['m.ply', 'o.obj'], ['m.stl', 'o.stl'], ['m.ply', 'o.ply', '--eps', '-0.5'], ['m.ply', 'o.ply', '--eps'],
                                  ['m.ply', 'o.ply', '--eps', 'nan'], ['m.ply', 'o.ply', '--eps', 'inf'], ['m.ply', 'o.ply', '--eps', 'small'],
                                  ['m.ply', 'o.ply', '--drop_duplicates', '1'], ['m.ply', 'o.ply', '--min_faces', '5']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import weld
    with pytest.raises(SystemExit) as e:
        weld.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_weld_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P, F, Dbl = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_weld_hook'] == (I, [P, I64, P, P, F, F, P, I64, P, P, Dbl, P, P, P])
    assert len([n for n in _lib.EXT_SIGNATURES if n.startswith('ppsx_weld_')]) == 2                      # no compress of its own: labels.py's
    assert _lib.EXT_SIGNATURES['ppsx_weld_faces'] == (I, [P, I64, I64, P, P, P, P])
    assert _lib.EXT_PARAMS['ppsx_weld_hook'] == ['pts', 'n', 'lo', 'hi', 'h', 'inv_h', 'table', 'capacity', 'order', 'offsets', 'eps', 'label', 'changed',
                                                 'stream']
    assert _lib.EXT_PARAMS['ppsx_weld_faces'] == ['faces', 'nf', 'nv', 'newrow', 'out', 'code', 'stream']
    sites = call_sites.ext_call_sites('ppsx_weld')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'weld.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {n: 1 for n in _lib.EXT_PARAMS if n.startswith('ppsx_weld_')} and len(sites) == 2
    # weld.py calls no other stage's entries: the cell lists come through trim.SupportGrid, which holds the one call of the slot entry, the
    # loop and the compress launch through labels.py
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'weld.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(sites) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert [path for path, _, _ in call_sites.ext_call_sites('ppsx_trim_cell_slots')['ppsx_trim_cell_slots']] == ['trim.py']
    assert 'pps_weld.hip' in build.SOURCES and 'pps_cells.h' in build.HEADERS
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)
