"""CPU tier of the edge-collapse decimation: the numpy specification tests/decimate_spec.py against chains written out
by hand, the invariants of a closed manifold, the quality that a clustering cannot give, the border rule, its edge cases, the argument
rules of `decimate_mesh` and of the command, and the extension entries of the C ABI."""
import ctypes

import numpy as np
import pytest

import call_sites
import decimate_spec as S
import denoise_spec

_cache = {}


def result(name):
    """The specification's result on a named mesh, computed once."""
    if name not in _cache:
        verts, faces, max_faces = S.named(name)
        _cache[name] = S.decimate_spec(verts, faces, max_faces)
    return _cache[name]


def test_the_octahedron_and_the_tetrahedron_by_hand():
    verts, faces = S.octahedron()
    for rounds, want in ((1, 6), (2, 4), (1000, 4)):
        out_v, out_f, info = S.decimate_spec(verts, faces, 4, rounds)
        assert info['faces_out'] == want == out_f.shape[0] and info['rounds'] == min(rounds, 2) == info['collapses']
        assert info['reached'] == (want == 4) and info['vertices_out'] == out_v.shape[0] == 6 - info['collapses']
        assert S.closed_manifold(out_v, out_f) and S.euler(out_v, out_f) == 2
    # every cost of the first round is the same by symmetry: the hash picks the edge; what is left of 4 faces has no candidate
    out_v, out_f, info = S.decimate_spec(verts, faces, 4)
    r = S.round_spec(out_v.astype(np.float64), out_f, 4)
    assert r['regular'].all() and (r['prio'] == S.NONE).all() and not r['flag'].any()
    # the tetrahedron is the floor: within the budget it comes back as given, and it has no candidate either
    verts, faces = S.tetrahedron()
    out_v, out_f, info = S.decimate_spec(verts, faces, 4)
    assert out_v is not None and out_v.tobytes() == verts.tobytes() and out_f.tobytes() == faces.tobytes()
    assert info == {'faces_in': 4, 'faces_valid': 4, 'faces_out': 4, 'vertices_in': 4, 'vertices_out': 4, 'rounds': 0, 'collapses': 0, 'fallbacks': 0,
                    'locked_vertices': 0, 'reached': True, 'max_faces': 4, 'max_rounds': 1000}
    r = S.round_spec(verts.astype(np.float64), faces, 4)
    assert r['regular'].all() and (r['prio'] == S.NONE).all()
    # the bipyramid between them: only the six edges from an apex can collapse
    out_v, out_f, _ = S.decimate_spec(*S.octahedron(), 4, 1)
    r = S.round_spec(out_v.astype(np.float64), out_f, 5)
    assert int((r['prio'][:, 0] != S.NONE).sum()) == 6 and int(r['flag'].sum()) == 1


def test_the_hash_and_the_priority_order():
    assert int(S.mix(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF          # splitmix64 of seed 0, first output
    key = (np.uint64(3) << np.uint64(32)) | np.uint64(7)
    z = (int(key) + 0x9E3779B97F4A7C15) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert int(S.mix(np.array([key]))[0]) == z ^ (z >> 31)
    prio = np.array([[5, 9, 1], [5, 2, 9], [4, 2 ** 64 - 2, 3], [5, 2, 8], [2 ** 64 - 1] * 3], dtype=np.uint64)
    assert S.ascending(prio).tolist() == [2, 3, 1, 0, 4]
    assert S.group_min(np.array([0, 0, 2, 2, 2]), prio, 4).tolist() == [[5, 2, 9], [2 ** 64 - 1] * 3, [4, 2 ** 64 - 2, 3], [2 ** 64 - 1] * 3]
    assert S.taken(prio, np.array([1, 1, 1, 1, 0], dtype=bool), 2).tolist() == [2, 3]


@pytest.mark.parametrize('name', sorted(S.CLOSED))
def test_a_closed_manifold_stays_closed_and_manifold(name):
    verts, faces, max_faces = S.named(name)
    assert S.closed_manifold(verts, faces) and S.euler(verts, faces) == S.CLOSED[name]
    out_v, out_f, info = result(name)
    assert (S.edge_owners(out_f) == 2).all()                                        # every edge has exactly two owners
    assert np.unique(np.sort(out_f, axis=1), axis=0).shape[0] == out_f.shape[0]     # no duplicated face
    assert S.valid_faces(out_f, out_v.shape[0]).all()                               # no invalid face
    assert S.euler(out_v, out_f) == S.CLOSED[name]
    assert max_faces - 1 <= info['faces_out'] <= max_faces and info['reached'] and info['faces_out'] == out_f.shape[0]
    assert info['locked_vertices'] == 0 and info['vertices_out'] == out_v.shape[0] == np.unique(out_f).shape[0]
    assert info['faces_valid'] - info['faces_out'] == 2 * info['collapses'] and info['vertices_in'] - info['vertices_out'] == info['collapses']
    if name == 'fan':
        assert np.bincount(faces.reshape(-1)).max() == 300                          # the crowded rows


def test_a_cube_keeps_its_faces_flat_and_its_volume():
    verts, faces, _ = S.named('cube8')
    assert faces.shape == (768, 3) and S.signed_volume(verts, faces) == 512.0
    out_v, out_f, info = result('cube8')
    assert info['faces_out'] == 192 and info['fallbacks'] == 0
    assert (denoise_spec.cube_surface_distance(out_v, 8) == 0.0).all()
    assert S.signed_volume(out_v, out_f) == 512.0
    # down to the 12 faces of a cube: 8 vertices, still a closed manifold
    out_v, out_f, info = result('cube8:12')
    assert info['faces_out'] == 12 and out_v.shape == (8, 3) and S.closed_manifold(out_v, out_f) and S.euler(out_v, out_f) == 2


def test_the_border_and_what_touches_nothing_stay_byte_for_byte():
    verts, faces, max_faces = S.named('patch')
    loose = np.array([[50.0, 50.0, -0.0]], dtype=np.float32)                        # a vertex of no face: not regular, dropped at the end
    verts = np.concatenate([verts, loose])
    border = S.border_vertices(faces, verts.shape[0])
    assert int(border.sum()) == 48
    out_v, out_f, info = S.decimate_spec(verts, faces, max_faces)
    assert info['locked_vertices'] == 49 and info['faces_out'] == 144 and info['vertices_out'] == 169 - info['collapses']
    assert S.decimate_spec(*S.named('patch'))[2]['locked_vertices'] == 48
    # the border vertices survive, in their order, with their bytes, and the border is the same loop of edges
    got = {p.tobytes() for p in out_v}
    assert all(p.tobytes() in got for p in verts[:169][border[:169]])
    out_border = S.border_vertices(out_f, out_v.shape[0])
    assert out_v[out_border].tobytes() == verts[border].tobytes()
    assert int((S.edge_owners(out_f) == 1).sum()) == 48 and (S.edge_owners(out_f) <= 2).all()
    assert S.euler(out_v, out_f) == S.euler(verts, faces) == 1


def test_the_ends_of_a_non_manifold_edge_never_move():
    verts, faces, _ = S.named('welded')
    assert verts.shape == (14, 3) and int((S.edge_owners(faces) == 4).sum()) == 1
    out_v, out_f, info = result('welded')
    assert info['locked_vertices'] == 2 and not info['reached'] and info['faces_out'] == 8 and info['rounds'] >= 1
    offsets, _, mult = S.adjacency(faces, 14)
    ends = np.unique(S.sources(offsets)[mult == 4])
    got = {p.tobytes() for p in out_v}
    assert ends.shape == (2,) and all(verts[e].tobytes() in got for e in ends)
    assert int((S.edge_owners(out_f) == 4).sum()) == 1 and int((S.edge_owners(out_f) == 2).sum()) == S.edge_owners(out_f).shape[0] - 1


def test_other_rules_of_the_output():
    verts, faces, max_faces = S.named('sphere')
    # the same ordered mesh gives the same bytes twice
    one, two = S.decimate_spec(verts, faces, max_faces), result('sphere')
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() and one[2] == two[2]
    # three invalid rows are dropped and change nothing else
    bad = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 642]], dtype=np.int64)
    out_v, out_f, info = S.decimate_spec(verts, np.concatenate([faces[:301], bad, faces[301:]]), max_faces)
    assert info['faces_in'] == 1283 and info['faces_valid'] == 1280 and out_v.tobytes() == two[0].tobytes() and out_f.tobytes() == two[1].tobytes()
    # -0.0 survives on a vertex that never moved
    signed = verts.copy()
    untouched = np.nonzero((two[0][:, None, :] == verts[None, :, :]).all(axis=2).any(axis=0))[0]
    assert untouched.shape[0] > 50
    signed[untouched[0], 1] = -0.0
    out_v = S.decimate_spec(signed, faces, max_faces, 1)[0]
    assert any(p.tobytes() == signed[untouched[0]].tobytes() for p in out_v) and np.signbit(signed[untouched[0], 1])
    # within the budget: as given, the invalid rows too
    mixed = np.concatenate([bad, faces])
    for budget in (1280, 5000):
        out_v, out_f, info = S.decimate_spec(verts, mixed, budget)
        assert out_v.tobytes() == verts.tobytes() and out_f.tobytes() == mixed.tobytes()
        assert info['reached'] and info['rounds'] == 0 and info['faces_out'] == 1283 and info['faces_valid'] == 1280 and info['vertices_out'] == 642
    # an empty mesh and a mesh without a valid face
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), (verts, np.zeros((0, 3), np.int64)), (verts, bad)):
        out_v, out_f, info = S.decimate_spec(v, f, 4)
        assert out_v.tobytes() == v.tobytes() and out_f.tobytes() == f.tobytes() and info['faces_valid'] == 0 and info['reached']
        assert info['locked_vertices'] == 0 and info['faces_out'] == f.shape[0]
    # max_rounds = 1 stops after one round
    out_v, out_f, info = S.decimate_spec(verts, faces, max_faces, 1)
    assert info['rounds'] == 1 and not info['reached'] and info['collapses'] >= 1 and info['faces_out'] == 1280 - 2 * info['collapses']
    assert S.closed_manifold(out_v, out_f)


def test_winners_share_no_end_and_no_neighbour():
    verts, faces, _ = S.named('sphere')
    r = S.round_spec(verts.astype(np.float64), faces, verts.shape[0])
    win = np.nonzero(r['flag'])[0]
    assert win.shape[0] >= 10
    ends = np.concatenate([r['src'][win], r['nbr'][win]])
    assert np.unique(ends).shape[0] == 2 * win.shape[0]
    is_end = np.zeros(verts.shape[0], dtype=bool)
    is_end[ends] = True
    partner = np.full(verts.shape[0], -1)
    partner[r['src'][win]], partner[r['nbr'][win]] = r['nbr'][win], r['src'][win]
    # a neighbour of an end is no end of another winner
    assert not (is_end[r['src']] & is_end[r['nbr']] & (partner[r['src']] != r['nbr'])).any()
    # the global minimum wins
    live = np.nonzero((r['prio'] != S.NONE).any(axis=1))[0]
    assert r['flag'][live[S.ascending(r['prio'][live])[0]]]


def test_decimate_mesh_argument_rules():
    import torch
    from ppsurf_amd import decimate
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in (3, 0, -1, 2 ** 31, 4.0, 4.5, float('nan'), '4', True, False, None):
        with pytest.raises(ValueError, match='max_faces'):
            decimate.decimate_mesh(v, f, bad)
    for bad in (0, -1, 2 ** 31, 2.0, float('inf'), '3', True, False, None):
        with pytest.raises(ValueError, match='max_rounds'):
            decimate.decimate_mesh(v, f, 4, bad)
    with pytest.raises(ValueError, match='max_faces'):                         # the parameters come first, in their order
        decimate.decimate_mesh(v, f, 3, 0)
    assert decimate._checked_params(np.int64(2 ** 31 - 1), np.int32(1)) == (2 ** 31 - 1, 1) and decimate._checked_params(4, 1000) == (4, 1000)
    with pytest.raises(decimate.CpuTensorError, match='no CPU'):
        decimate.decimate_mesh(v, f, 4)
    assert issubclass(decimate.CpuTensorError, PpsError) and issubclass(decimate.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='decimate_mesh: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        decimate.decimate_mesh(v, f, max_faces=100, max_rounds=5)


@pytest.mark.parametrize('argv', [['m.ply'], ['m.ply', 'o.ply'], ['m.ply', 'o.obj', '--max_faces', '100'], ['m.ply', 'o.ply', '--max_faces', '3'],
                                  ['m.ply', 'o.ply', '--max_faces', '-3'], ['m.ply', 'o.ply', '--max_faces', '2.5'],
                                  ['m.ply', 'o.ply', '--max_faces', '2147483648'], ['m.ply', 'o.ply', '--max_faces', 'True'],
                                  ['m.ply', 'o.ply', '--max_faces', '100', '--max_rounds', '0'],
                                  ['m.ply', 'o.ply', '--max_faces', '100', '--max_rounds', '1.5'], ['m.ply', 'o.ply', '--max_rounds', '5']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import decimate
    with pytest.raises(SystemExit) as e:
        decimate.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_decimate_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    want = {'ppsx_decimate_regular': ['offsets', 'mult', 'ne', 'inc_offsets', 'ni', 'nv', 'regular', 'stream'],
            'ppsx_decimate_edges': ['pos', 'nv', 'faces', 'nf', 'offsets', 'nbr', 'src', 'ne', 'inc_offsets', 'inc', 'ni', 'regular', 'prio', 'x',
                                    'fell', 'stream'],
            'ppsx_decimate_vertex_min': ['offsets', 'nbr', 'ne', 'nv', 'prio', 'm1', 'stream'],
            'ppsx_decimate_ring_min': ['offsets', 'nbr', 'ne', 'nv', 'm1', 'best', 'stream'],
            'ppsx_decimate_winners': ['src', 'nbr', 'ne', 'nv', 'prio', 'best', 'flag', 'stream'],
            'ppsx_decimate_move': ['win', 'nw', 'src', 'nbr', 'ne', 'x', 'pos', 'nv', 'rename', 'stream'],
            'ppsx_decimate_rename': ['faces', 'nf', 'nv', 'rename', 'out', 'keep', 'stream']}
    counts = ('ne', 'ni', 'nv', 'nf', 'nw')
    for name, params in want.items():
        assert _lib.EXT_PARAMS[name] == params, name
        assert _lib.EXT_SIGNATURES[name] == (I, [I64 if p in counts else P for p in params]), name
    assert sorted(n for n in _lib.EXT_PARAMS if n.startswith('ppsx_decimate')) == sorted(want)
    assert not any(n.startswith('pps_decimate') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_decimate')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'decimate.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {name: 1 for name in want}
    # the stage adds no call site of another stage's entries: it takes its rows from topology.adjacency_rows / incidence_rows
    stages = sorted({n.split('_')[1] for n in _lib.EXT_PARAMS} - {'decimate'})
    assert len(stages) >= 7
    for stage in stages:
        for name, where in call_sites.ext_call_sites('ppsx_' + stage + '_').items():
            assert all(path != 'decimate.py' for path, _, _ in where), name
    assert 'pps_decimate.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)
