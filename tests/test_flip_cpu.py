"""CPU tier of the Delaunay edge flips: the numpy specification tests/flip_spec.py against quads written out by hand,
the Delaunay property of flat jittered lattices checked by brute force, the invariants on curved and repaired meshes, the independence of
the winners of every round, the argument rules of `flip_edges` and of the command, and the extension entries of the C ABI.

Recorded, not asserted (this generator, seeds = n): lattice 4: 20 Delaunay violations before, 10 flips in 5 rounds; lattice 12: 173, 85
flips in 7 rounds; lattice 24: 561, 279 flips in 7 rounds; 0 violations after in all three."""
import ctypes
import os
import re

import numpy as np
import pytest

import call_sites
import decimate_spec
import flip_spec as S

_cache = {}


def spec(name, max_angle=10.0):
    """(verts, faces as given, faces out, info, the evaluations of the rounds) of a named case, computed once."""
    if (name, max_angle) not in _cache:
        verts, faces = S.case(name)
        trace = []
        _, out, info = S.flip_spec(verts, faces, max_angle, trace=trace)
        _cache[(name, max_angle)] = (verts, faces, out, info, trace)
    return _cache[(name, max_angle)]


def quad_mesh(a, b, c, d, second=(1, 0, 3)):
    """The two faces (0, 1, 2) and `second` over the four points."""
    return np.array([a, b, c, d], dtype=np.float32), np.array([[0, 1, 2], list(second)], dtype=np.int64)


def test_a_flat_quad_with_the_long_diagonal_flips_once():
    verts, faces = quad_mesh((-2, 0, 0), (2, 0, 0), (0, 0.5, 0), (0, -0.5, 0))
    trace = []
    out_v, out, info = S.flip_spec(verts, faces, trace=trace)
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]] and out_v.tobytes() == verts.tobytes()
    assert info == {'faces_in': 2, 'faces_valid': 2, 'edges_manifold': 1, 'candidates_in': 1, 'candidates_out': 0, 'flips': 1, 'rounds': 1,
                    'converged': True, 'max_angle': 10.0, 'min_gain': 1e-6, 'max_rounds': 100}
    ev = trace[0]
    assert ev['s'].tolist() == [-3.75] and ev['quad'].tolist() == [[0, 1, 2, 3]] and ev['win'].tolist() == [True]
    assert int(ev['prio'][0]) == ((S.INF_BITS - int(np.float32(3.75).view(np.uint32))) << 32) | int(S.fmix32(0))
    assert ev['vmin'].tolist() == [int(ev['prio'][0])] * 4
    # whichever face comes first, and whichever slot holds the edge
    for second in ((0, 3, 1), (3, 1, 0)):
        assert S.flip_spec(verts, np.array([[2, 0, 1], list(second)]))[1].tolist() == [[0, 3, 2], [1, 2, 3]]
    assert S.flip_spec(verts, faces[::-1])[1].tolist() == [[1, 2, 3], [0, 3, 2]]          # f = (1, 0, 3): a = 1, b = 0, c = 3, d = 2
    # the flipped quad is at rest
    again = S.flip_spec(verts, out)
    assert again[1].tobytes() == out.tobytes() and again[2]['candidates_in'] == 0 and again[2]['rounds'] == 0


def test_a_square_a_non_convex_quad_and_a_crease_do_not_flip_and_a_cap_does():
    verts, faces = quad_mesh((0, 0, 0), (1, 1, 0), (0, 1, 0), (1, 0, 0))
    ev = S.evaluate(verts.astype(np.float64), faces, 4, S.cos2_of(10.0), 0.0)
    assert ev['s'].tolist() == [0.0] and not ev['cand'].any()                           # p = q = 0 exactly, and 0 < -0 is false
    assert S.flip_spec(verts, faces, min_gain=0.0)[1].tobytes() == faces.tobytes()
    # b lies inside the triangle a, c, d: the new faces would fold over
    verts, faces = quad_mesh((0, 0, 0), (2, 0, 0), (3, 1, 0), (3, -1, 0))
    assert S.flip_spec(verts, faces, 90.0, 0.0)[2]['candidates_in'] == 0
    P = verts.astype(np.float64)
    n = np.cross(P[1] - P[0], P[2] - P[0]) + np.cross(P[0] - P[1], P[3] - P[1])
    assert np.dot(np.cross(P[2] - P[1], P[3] - P[1]), n) < 0                              # m2.N: the fold guard by itself refuses
    # c exactly on ab: a face without area passes the crease guard and is flipped away, first of all
    verts, faces = quad_mesh((-1, 0, 0), (1, 0, 0), (0, 0, 0), (0, -1, 0))
    trace = []
    _, out, info = S.flip_spec(verts, faces, trace=trace)
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]] and info['flips'] == 1 and info['converged']
    assert trace[0]['s'].tolist() == [-np.inf] and int(trace[0]['prio'][0]) >> 32 == 0
    assert S.min_angle(verts, faces) == 0.0 and S.min_angle(verts, out) == 45.0
    # both faces without area: inf - inf is no candidate
    verts, faces = quad_mesh((-1, 0, 0), (1, 0, 0), (0, 0, 0), (0.5, 0, 0))
    assert S.flip_spec(verts, faces)[2]['candidates_in'] == 0
    # 90 degrees between the faces, the angles at c and d obtuse
    verts, faces = quad_mesh((0, 0, 0), (1, 0, 0), (0.5, 0.1, 0), (0.5, 0, 0.1))
    assert S.flip_spec(verts, faces)[2]['candidates_in'] == 0 and S.flip_spec(verts, faces)[1].tobytes() == faces.tobytes()
    flat = verts.copy()
    flat[3] = (0.5, -0.1, 0)
    assert S.flip_spec(flat, faces)[2]['flips'] == 1
    bent = verts.copy()
    bent[3] = (0.5, -0.1, 0.03)                                                           # 16.7 degrees: between 10 and 30
    assert S.flip_spec(bent, faces, 10.0)[2]['flips'] == 0 and S.flip_spec(bent, faces, 30.0)[2]['flips'] == 1


def test_closed_and_doubled_faces_have_no_candidate():
    verts, faces = decimate_spec.tetrahedron()
    ev = S.evaluate(verts.astype(np.float64), faces, 4, S.cos2_of(90.0), 0.0)
    assert ev['f'].shape[0] == 6 and not ev['cand'].any() and np.isnan(ev['s']).all()   # every {c, d} is an edge already
    assert S.flip_spec(verts, faces, 90.0, 0.0)[2]['edges_manifold'] == 6
    verts = np.array([[-2, 0, 0], [2, 0, 0], [0, 0.5, 0], [0, -0.5, 0]], dtype=np.float32)
    for second in ((0, 1, 2), (1, 2, 0)):                                                 # two copies: every pair runs its edge the same way
        faces = np.array([[0, 1, 2], list(second)], dtype=np.int64)
        _, out, info = S.flip_spec(verts, faces, 90.0, 0.0)
        assert out.tobytes() == faces.tobytes() and info['edges_manifold'] == 3 and info['candidates_in'] == 0 and S.incoherent_pairs(faces, 4) == 3
    faces = np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64)                              # a triangle and its mirror: c == d
    _, out, info = S.flip_spec(verts, faces, 90.0, 0.0)
    assert out.tobytes() == faces.tobytes() and info['edges_manifold'] == 3 and info['candidates_in'] == 0 and S.incoherent_pairs(faces, 4) == 0
    faces = np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int64)                              # the long diagonal, run the same way twice
    _, out, info = S.flip_spec(verts, faces, 90.0, 0.0)
    assert out.tobytes() == faces.tobytes() and info['edges_manifold'] == 1 and info['candidates_in'] == 0


@pytest.mark.parametrize('n', S.LATTICES)
def test_a_flat_jittered_lattice_comes_out_delaunay(n):
    verts, faces, out, info, trace = spec('lattice {}'.format(n))
    assert faces.shape == (2 * n * n, 3) and (verts[:, 2] == 0).all() and verts[:, :2].min() == 0.0 and verts[:, :2].max() == float(n)
    before, after = S.delaunay_violations(verts, faces), S.delaunay_violations(verts, out)
    print('lattice', n, 'violations', before, '->', after, 'flips', info['flips'], 'rounds', info['rounds'])
    assert before > 0 and after == 0 and info['converged'] and 0 < info['rounds'] <= 15 and info['candidates_out'] == 0
    assert (S.areas2(verts, faces) > 0).all() and (S.areas2(verts, out) > 0).all()
    assert abs(S.areas2(verts, out).sum() - 2.0 * n * n) <= 1e-9 * n * n and abs(S.areas2(verts, faces).sum() - 2.0 * n * n) <= 1e-9 * n * n
    assert info['edges_manifold'] == 3 * n * n - 2 * n and S.min_angle(verts, out) > S.min_angle(verts, faces)
    # the crease guard plays no part on a flat mesh
    assert S.flip_spec(verts, faces, 90.0)[1].tobytes() == out.tobytes()


def test_a_co_circular_lattice_needs_the_margin():
    verts, faces = S.jittered_lattice(8)
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing='ij')
    c, s = np.cos(0.3), np.sin(0.3)
    verts = np.stack([c * i.reshape(-1) - s * j.reshape(-1), s * i.reshape(-1) + c * j.reshape(-1), 0.0 * i.reshape(-1)], axis=1).astype(np.float32)
    with_margin, without = S.flip_spec(verts, faces)[2], S.flip_spec(verts, faces, min_gain=0.0)[2]
    print('rotated lattice: rounds', with_margin['rounds'], 'with the margin,', without['rounds'], 'without')
    assert with_margin['converged'] and with_margin['rounds'] <= without['rounds'] and with_margin['flips'] <= without['flips']


@pytest.mark.parametrize('max_angle', S.ANGLES)
@pytest.mark.parametrize('name', [b + v for b in S.BASES for v in S.VARIANTS])
def test_invariants_on_curved_and_repaired_meshes(name, max_angle):
    verts, faces, out, info, trace = spec(name, max_angle)
    nv = verts.shape[0]
    ok = S.valid_faces(faces, nv)
    assert out.shape == faces.shape and out.dtype == np.int64 and out[~ok].tobytes() == faces[~ok].tobytes()
    assert np.array_equal(S.valid_faces(out, nv), ok) and info['faces_valid'] == int(ok.sum()) and info['faces_in'] == faces.shape[0]
    border0, many0, keys0, count0 = S.edge_sets(faces, nv)
    border1, many1, keys1, count1 = S.edge_sets(out, nv)
    assert np.array_equal(border0, border1) and np.array_equal(many0, many1) and np.array_equal(keys0[count0 > 2], keys1[count1 > 2])
    assert np.array_equal(count0[count0 > 2], count1[np.isin(keys1, many0)])
    stay = np.isin(keys1, keys0)
    assert np.array_equal(count1[stay], count0[np.isin(keys0, keys1)])                   # no edge gains (or loses) an owner ...
    assert (count1[~stay] == 2).all() and int((~stay).sum()) == int((~np.isin(keys0, keys1)).sum()) <= info['flips']          # ... but the turned ones
    live = out[ok]
    assert np.unique(np.sort(live, axis=1), axis=0).shape[0] == np.unique(np.sort(faces[ok], axis=1), axis=0).shape[0]
    assert decimate_spec.closed_manifold(verts, live) == decimate_spec.closed_manifold(verts, faces[ok])
    assert decimate_spec.euler(verts, live) == decimate_spec.euler(verts, faces[ok])
    assert S.incoherent_pairs(out, nv) == S.incoherent_pairs(faces, nv) == 0
    assert info['converged'] and info['candidates_out'] == 0 and info['rounds'] == len(trace) <= 100
    assert info['flips'] == sum(int(ev['win'].sum()) for ev in trace) and info['edges_manifold'] == int((count0 == 2).sum())
    again = S.flip_spec(verts, out, max_angle)
    assert again[1].tobytes() == out.tobytes() and again[2]['flips'] == 0 and again[2]['candidates_in'] == 0
    for ev in trace:
        win = np.nonzero(ev['win'])[0]
        corners = ev['quad'][win].reshape(-1)
        assert win.shape[0] >= 1 and np.unique(corners).shape[0] == corners.shape[0]      # the winners share no quad vertex
        assert ev['win'][int(np.argmin(ev['prio']))] and np.unique(ev['prio'][ev['cand']]).shape[0] == int(ev['cand'].sum())
        faces_of = np.concatenate([ev['f'][win], ev['g'][win]])
        assert np.unique(faces_of).shape[0] == faces_of.shape[0]
    if name.startswith('cubes welded'):
        assert many0.shape[0] == 1 and info['flips'] == 0                               # right angles and squares: nothing to do
    if name.endswith(' shuffled') or name.endswith(' invalid'):
        plain = spec(name.rsplit(' ', 1)[0], max_angle)
        assert info['flips'] > 0 or plain[3]['flips'] == 0
    if name == 'cube decimated':
        assert faces.shape[0] == 192 and decimate_spec.signed_volume(verts, faces) == 512.0 and decimate_spec.signed_volume(verts, out) == 512.0
        print('decimated cube: smallest angle', S.min_angle(verts, faces), '->', S.min_angle(verts, out), 'at', max_angle)
        assert S.min_angle(verts, out) > S.min_angle(verts, faces) and info['flips'] > 0
    if name in ('torus scrambled', 'sphere scrambled'):
        assert decimate_spec.closed_manifold(verts, faces) and info['flips'] > 0


def test_the_fixtures_are_what_they_say():
    assert len(S.CASES) == len(set(S.CASES)) == 23
    for name in S.CASES:
        verts, faces = S.case(name)
        assert verts.dtype == np.float32 and faces.dtype == np.int64 and faces.ndim == 2 and faces.shape[1] == 3 and faces.flags['C_CONTIGUOUS'], name
    for b in S.BASES:
        verts, faces = S.base(b)
        assert S.valid_faces(faces, verts.shape[0]).all() and faces.shape[0] >= 20
        bad = S.case(b + ' invalid')[1]
        assert bad.shape[0] == faces.shape[0] + 3 and [bad[k].tolist() for k in (3, 10, 11)] == S.INVALID.tolist()
        mixed = S.case(b + ' shuffled')[1]
        assert mixed.tobytes() != faces.tobytes() and np.array_equal(np.unique(mixed, axis=0), np.unique(faces, axis=0))
    assert S.base('sphere decimated')[1].shape[0] == 600 and S.base('cube decimated')[1].shape[0] == 192
    plain = decimate_spec.torus(32, 16)[1]
    assert 50 < int((S.base('torus scrambled')[1] != plain).any(axis=1).sum()) and decimate_spec.euler(*S.base('torus scrambled')) == 0
    assert S.case('lattice 12')[1].shape[0] == 288 and S.flip_spec(*S.case('lattice 12'))[2]['edges_manifold'] == 408
    for name in ('empty', 'all invalid'):
        verts, faces = S.case(name)
        _, out, info = S.flip_spec(verts, faces)
        assert out.tobytes() == faces.tobytes() and info['faces_valid'] == 0 and info['edges_manifold'] == 0 and info['converged'] and info['rounds'] == 0


def test_max_rounds_is_a_bound_and_candidates_out_reports_what_is_left():
    verts, faces, out, info, _ = spec('lattice 12')
    _, one, first = S.flip_spec(verts, faces, max_rounds=1)
    assert first['rounds'] == 1 and not first['converged'] and first['candidates_out'] > 0 and 0 < first['flips'] < info['flips']
    assert first['candidates_in'] == info['candidates_in'] and first['max_rounds'] == 1
    assert S.flip_spec(verts, one)[1].tobytes() == out.tobytes() and S.flip_spec(verts, one)[2]['candidates_in'] == first['candidates_out']
    whole = S.flip_spec(verts, faces, max_rounds=info['rounds'])                          # the last allowed round empties the list
    assert whole[2]['converged'] and whole[2]['candidates_out'] == 0 and whole[1].tobytes() == out.tobytes()
    short = S.flip_spec(verts, faces, max_rounds=info['rounds'] - 1)
    assert not short[2]['converged'] and short[2]['rounds'] == info['rounds'] - 1


def test_fmix32_and_the_priority_word():
    assert int(S.fmix32(0)) == 0 and int(S.fmix32(1)) == 0x514E28B7 and int(S.fmix32(0xFFFFFFFF)) == 0x81F16F39
    r = np.arange(1 << 16)
    assert np.unique(S.fmix32(r)).shape[0] == r.shape[0] and S.fmix32(r).dtype == np.uint32
    # worst first: the more negative s, the smaller the high word; -inf has the smallest of all
    s = np.array([-np.inf, -1e30, -3.75, -1.0, -1e-6, -1e-30], dtype=np.float64)
    high = S.INF_BITS - (-s).astype(np.float32).view(np.uint32).astype(np.int64)
    assert high[0] == 0 and (np.diff(high) > 0).all() and high.max() < 2 ** 31
    assert int(S.NONE) == 2 ** 64 - 1 and 0.0 < S.cos2_of(90.0) < 1e-30 and abs(S.cos2_of(10.0) - 0.9698463103929542) < 1e-15


def test_flip_edges_argument_rules():
    import torch
    from ppsurf_amd import flip
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in (0, 0.0, -1, 90.5, 180, float('nan'), float('inf'), True, '10', None, [10.0]):
        with pytest.raises(ValueError, match='max_angle'):
            flip.flip_edges(v, f, max_angle=bad)
    for bad in (-1e-9, -1, float('nan'), float('inf'), False, '0', None):
        with pytest.raises(ValueError, match='min_gain'):
            flip.flip_edges(v, f, min_gain=bad)
    for bad in (0, -1, 2 ** 31, 1.0, 10.5, True, '3', None):
        with pytest.raises(ValueError, match='max_rounds'):
            flip.flip_edges(v, f, max_rounds=bad)
    assert flip._checked_params(90, 0, np.int64(7)) == (90.0, 0.0, 7) and flip._checked_params(np.float32(0.5), np.float64(2.0), 2 ** 31 - 1)[2] == 2 ** 31 - 1
    # good parameters, CPU tensors: the device guard of the other mesh stages, after the parameters
    for fn in (lambda: flip.flip_edges(v, f), lambda: flip.flip_edges(v, f, 90, 0, 1)):
        with pytest.raises(flip.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(flip.CpuTensorError, PpsError) and issubclass(flip.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='flip_edges: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        flip.flip_edges(v, f, max_angle=30.0)
    assert flip.MAX_COUNT == 2 ** 31 - 1


@pytest.mark.parametrize('argv', [['m.ply'], [], ['m.ply', 'o.obj'], ['m.ply', 'o.ply', '--max_angle', '0'], ['m.ply', 'o.ply', '--max_angle', '91'],
                                  ['m.ply', 'o.ply', '--max_angle'], ['m.ply', 'o.ply', '--min_gain', '-1'], ['m.ply', 'o.ply', '--min_gain', 'nan'],
                                  ['m.ply', 'o.ply', '--max_rounds', '0'], ['m.ply', 'o.ply', '--max_rounds', '1.5'], ['m.ply', 'o.ply', '--gen_flip', '1']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import flip
    with pytest.raises(SystemExit) as e:
        flip.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_flip_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P, F64 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_flip_candidates'] == (I, [P, I64, P, I64, P, P, P, P, I64, P, I64, F64, F64, P, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_flip_winners'] == (I, [P, P, I64, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_flip_apply'] == (I, [P, P, P, P, I64, I64, P, I64, P])
    assert _lib.EXT_PARAMS['ppsx_flip_candidates'] == ['verts', 'nv', 'faces', 'nf', 'fa', 'fb', 'ea', 'eb', 'np', 'keys', 'ne', 'cos2', 'min_gain', 'prio',
                                                       'quad', 'vmin', 'stream']
    assert _lib.EXT_PARAMS['ppsx_flip_winners'] == ['prio', 'quad', 'np', 'vmin', 'nv', 'flag', 'stream']
    assert _lib.EXT_PARAMS['ppsx_flip_apply'] == ['fa', 'fb', 'quad', 'flag', 'np', 'nv', 'faces', 'nf', 'stream']
    sites = call_sites.ext_call_sites('ppsx_flip')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'flip.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {n: 1 for n in _lib.EXT_PARAMS if n.startswith('ppsx_flip_')} and len(sites) == 3
    # flip.py calls no other stage's entries; the edges come through the topology layer, which holds the one call of the key entry
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'flip.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(sites) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert [path for path, _, _ in call_sites.ext_call_sites('ppsx_pieces_edge_keys')['ppsx_pieces_edge_keys']] == ['topology.py']
    assert 'pps_flip.hip' in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, 'pps_flip.hip'))
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)
    # the specification shares no code with the module
    spec_source = open(os.path.join(call_sites.REPO, 'tests', 'flip_spec.py')).read()
    assert 'ppsurf_amd' not in re.sub(r'""".*?"""', '', spec_source, flags=re.S)


def test_the_hand_made_quads_that_both_tiers_run():
    flips = {name: S.flip_spec(verts, faces, max_angle, min_gain)[2]['flips'] for name, verts, faces, max_angle, min_gain in S.hand_cases()}
    assert flips == {'long diagonal': 1, 'long diagonal, other slots': 1, 'long diagonal, other order': 1, 'square': 0, 'non-convex': 0, 'cap': 1,
                     'two caps': 0, 'crease 90': 0, 'crease 16.7 at 10': 0, 'crease 16.7 at 30': 1, 'twins': 0, 'mirror': 0, 'incoherent': 0}
