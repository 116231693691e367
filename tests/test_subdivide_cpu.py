"""CPU tier of the longest-edge bisection: the numpy specification tests/subdivide_spec.py against meshes written out
by hand, the invariants on closed, open, repaired and non-manifold meshes measured without the rule, the half-angle bound of Rosenberg and
Stenger, the bounds on rounds and faces, the argument rules of `split_long_edges` and of the command, and the extension entries of the C ABI.

Recorded, not asserted (these generators): every case converges in at most 15 rounds; smallest angle after / before at factors 1.0, 0.5, 0.26:
tetrahedron 0.500 (60 -> 30.000 degrees), sphere 0.632, torus 0.983, 1.000 for the rest; the sphere at 0.26 ends with about 42 000 faces."""
import ctypes
import os
import re

import numpy as np
import pytest

import call_sites
import decimate_spec
import subdivide_spec as S

_cache = {}


def spec(name, factor):
    """(verts, faces as given, verts out, faces out, ends, info, trace) of a named case at a factor, computed once."""
    if (name, factor) not in _cache:
        verts, faces = S.case(name)
        trace = []
        out_v, out_f, ends, info = S.subdivide_spec(verts, faces, factor=factor, trace=trace)
        _cache[(name, factor)] = (verts, faces, out_v, out_f, ends, info, trace)
    return _cache[(name, factor)]


def hand(name):
    return [c for c in S.hand_cases() if c[0] == name][0][1:]


def rows_sorted(faces):
    return faces[np.lexsort(faces.T[::-1])]


@pytest.mark.parametrize('name, row, new', [('slot 0', (0, 3, 2), (3, 1, 2)), ('slot 1', (2, 0, 3), (2, 3, 1)), ('slot 2', (3, 2, 0), (1, 2, 3))])
def test_one_triangle_with_one_long_edge_gets_the_two_rows(name, row, new):
    verts, faces, max_edge, max_rounds = hand(name)
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge, max_rounds=max_rounds)
    assert out_f.tolist() == [list(row), list(new)] and out_v[:3].tobytes() == verts.tobytes() and out_v[3].tolist() == [2.0, 0.0, 0.0]
    assert ends.tolist() == [[0, 1]] and out_v.dtype == np.float32 and out_f.dtype == np.int64 and ends.dtype == np.int64
    assert info == {'vertices_in': 3, 'vertices_out': 4, 'faces_in': 1, 'faces_valid': 1, 'faces_out': 2, 'edges_in': 3, 'max_edge': 3.5,
                    'candidates_in': 1, 'candidates_out': 0, 'splits': 1, 'rounds': 1, 'converged': True, 'limited': False, 'max_rounds': 100,
                    'max_faces': (2 ** 32 - 1) // 3, 'added': [1]}
    for f in out_f:                                                                       # both wound like the parent: +z
        assert np.cross(out_v[f[1]] - out_v[f[0]], out_v[f[2]] - out_v[f[0]])[2] > 0


def test_shared_edges_split_all_their_owners_through_one_vertex():
    verts, faces, max_edge, _ = hand('two faces')
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge)
    assert out_f.tolist() == [[0, 4, 2], [1, 4, 3], [4, 1, 2], [4, 0, 3]] and out_v[4].tolist() == [2.0, 0.0, 0.0] and info['added'] == [1]
    assert S.incoherent_pairs(out_f) == 0 and (S.edge_lengths2(out_v, out_f)[1] <= 2).all()
    verts, faces, max_edge, _ = hand('three on an edge')
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge)
    assert out_f.tolist() == [[0, 5, 2], [1, 5, 3], [0, 5, 4], [5, 1, 2], [5, 0, 3], [5, 1, 4]] and info['splits'] == 1 and ends.tolist() == [[0, 1]]
    keys, owners, _ = S.edge_lengths2(out_v, out_f)
    assert sorted(owners[owners > 2].tolist()) == [3, 3] and set(keys[owners > 2].tolist()) == {(0 << 32) | 5, (1 << 32) | 5}
    verts, faces, max_edge, _ = hand('two copies')
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge)
    assert out_f.tolist() == [[0, 3, 2], [0, 3, 2], [3, 1, 2], [3, 1, 2]] and info['vertices_out'] == 4 and info['splits'] == 1


def test_a_face_whose_longest_edge_loses_waits_exactly_one_round():
    verts, faces, max_edge, _ = hand('waits')
    trace = []
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge, trace=trace)
    first, second = trace[0][2], trace[1][2]
    shared = int(np.nonzero(first['keys'] == ((0 << 32) | 1))[0][0])
    assert first['cand'][shared] and first['votes'][shared] == 1 and first['owners'][shared] == 2 and not first['win'][shared]
    assert first['hit'].tolist() == [True, False] and ends[0].tolist() == [1, 2] and info['added'][0] == 1
    shared = int(np.nonzero(second['keys'] == ((0 << 32) | 1))[0][0])
    assert second['win'][shared] and second['hit'][:2].tolist() == [True, True] and [0, 1] in ends[1:1 + info['added'][1]].tolist()
    assert info['converged'] and (S.edge_lengths2(out_v, out_f)[2] <= max_edge * max_edge).all()


def test_three_equal_lengths_split_one_edge():
    verts, faces, max_edge, _ = hand('equilateral')
    ev = S.evaluate(verts, faces, max_edge * max_edge)
    assert ev['len2'].tolist() == [8.0, 8.0, 8.0] and ev['cand'].all() and np.unique(ev['prio'] >> np.uint64(32)).shape[0] == 1
    assert int(ev['win'].sum()) == 1 and ev['win'][int(np.argmin(ev['prio']))] and ev['votes'].sum() == 1
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge, max_rounds=1)
    assert info['added'] == [1] and info['faces_out'] == 2 and not info['converged'] and info['candidates_out'] > 0
    whole = S.subdivide_spec(verts, faces, max_edge=max_edge)
    assert whole[3]['converged'] and whole[3]['added'][0] == 1


def test_an_edge_between_neighbouring_floats_is_no_candidate():
    verts, faces, max_edge, max_rounds = hand('neighbouring floats')
    key = np.array([(0 << 32) | 1], dtype=np.int64)
    for max2 in (0.0, 1e-300, 1e-60, 1e-16):
        len2, prio = S.edge_priorities(key, verts, max2)
        assert 0.0 < len2[0] < 1e-13 and prio[0] == S.NONE
    assert S.midpoints(verts, [0], [1]).tobytes() in (verts[0:1].tobytes(), verts[1:2].tobytes())
    trace = []
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge, max_rounds=max_rounds, trace=trace)
    assert info['rounds'] == max_rounds and [0, 1] not in ends.tolist()
    for V, F, ev in trace:
        assert not ev['cand'][ev['keys'] == key[0]].any()
    new = out_v[verts.shape[0]:]                                                          # no new vertex lies on an end of its own edge
    assert (new != out_v[ends[:, 0]]).any(axis=1).all() and (new != out_v[ends[:, 1]]).any(axis=1).all()


def test_rows_that_are_invalid_as_given_stay_out_of_play():
    verts, faces, max_edge, _ = hand('rows out of play')
    trace = []
    out_v, out_f, ends, info = S.subdivide_spec(verts, faces, max_edge=max_edge, trace=trace)
    assert info['splits'] > 0 and info['vertices_out'] > 8 and info['faces_valid'] == 1 and info['edges_in'] == 3
    assert out_f[0].tolist() == [7, 1, 2] and out_f[2].tolist() == [5, 6, 5] and out_v[:7].tobytes() == verts.tobytes()
    for V, F, ev in trace:
        assert F[0].tolist() == [-1, -1, -1] and F[2].tolist() == [-1, -1, -1] and not ev['hit'][[0, 2]].any()
    alone = S.subdivide_spec(verts, faces[1:2], max_edge=max_edge)
    assert alone[0].tobytes() == out_v.tobytes() and alone[2].tobytes() == ends.tobytes()
    assert np.array_equal(np.delete(out_f, [0, 2], axis=0), alone[1])
    for name in ('empty', 'all invalid'):
        verts, faces = S.case(name)
        for kw in (dict(max_edge=0.5), dict(factor=0.5)):
            out_v, out_f, ends, info = S.subdivide_spec(verts, faces, **kw)
            assert out_f.tobytes() == faces.tobytes() and out_v.tobytes() == verts.tobytes() and ends.shape == (0, 2) and info['converged']
            assert info['faces_valid'] == 0 and info['rounds'] == 0 and info['added'] == [] and info['max_edge'] == kw.get('max_edge', 0.0)


@pytest.mark.parametrize('factor', S.FACTORS)
@pytest.mark.parametrize('name', [b + v for b in S.BASES for v in S.VARIANTS])
def test_invariants(name, factor):
    verts, faces, out_v, out_f, ends, info, trace = spec(name, factor)
    nv, nf = verts.shape[0], faces.shape[0]
    ok = S.valid_faces(faces, nv)
    before, after = faces[ok], S.live(out_f, out_v.shape[0])
    max2 = info['max_edge'] * info['max_edge']
    assert info['converged'] and not info['limited'] and info['candidates_out'] == 0 and info['rounds'] == len(trace) == len(info['added']) <= 100
    assert info['splits'] == sum(info['added']) == ends.shape[0] == out_v.shape[0] - nv and info['faces_out'] == out_f.shape[0]
    assert info['faces_valid'] == int(ok.sum()) and info['faces_in'] == nf and info['vertices_in'] == nv and info['vertices_out'] == out_v.shape[0]
    assert out_v.dtype == np.float32 and out_v[:nv].tobytes() == verts.tobytes() and out_f[:nf][~ok].tobytes() == faces[~ok].tobytes()
    assert after.shape[0] == out_f.shape[0] - int((~ok).sum()) and (ends[:, 0] < ends[:, 1]).all() and (ends[:, 1] < nv + np.arange(ends.shape[0])).all()
    keys0, owners0, len0 = S.edge_lengths2(verts, before)
    keys1, owners1, len1 = S.edge_lengths2(out_v, after)
    assert info['edges_in'] == keys0.shape[0] and info['candidates_in'] == int((len0 > max2).sum())
    assert info['max_edge'] == factor * float(np.sqrt(np.sort(len0)[(len0.shape[0] - 1) // 2]))           # (this measure sums in another order)
    assert len1.max() <= max2 and len1.min() > 0.0
    stay = np.isin(keys1, keys0)
    assert np.array_equal(owners1[stay], owners0[np.isin(keys0, keys1)])                 # a surviving edge keeps its owners
    won = np.concatenate([ev['owners'][ev['win']] for _, _, ev in trace]) if trace else np.zeros(0, dtype=np.int64)
    hits = sum(int(ev['hit'].sum()) for _, _, ev in trace)
    assert hits == int(won.sum()) == out_f.shape[0] - nf
    assert int((owners1 == 1).sum()) == int((owners0 == 1).sum()) + int((won == 1).sum())
    assert int((owners1 > 2).sum()) == int((owners0 > 2).sum()) + int((won > 2).sum())
    assert int((owners1 == 2).sum()) == int((owners0 == 2).sum()) + int((won == 2).sum()) + hits
    assert decimate_spec.closed_manifold(out_v, after) == decimate_spec.closed_manifold(verts, before)
    assert decimate_spec.euler(out_v, after) == decimate_spec.euler(verts, before)
    assert np.unique(np.sort(after, axis=1), axis=0).shape[0] == after.shape[0]
    assert S.incoherent_pairs(after) == S.incoherent_pairs(before) == 0
    again = S.subdivide_spec(out_v, out_f, max_edge=info['max_edge'])
    assert again[0].tobytes() == out_v.tobytes() and again[1].tobytes() == out_f.tobytes() and again[3]['splits'] == 0 and again[3]['candidates_in'] == 0
    for V, F, ev in trace:
        win_keys = ev['keys'][ev['win']]
        live = F[S.valid_faces(F, V.shape[0])]
        face_keys = np.stack([(np.minimum(live[:, i], live[:, (i + 1) % 3]) << 32) | np.maximum(live[:, i], live[:, (i + 1) % 3]) for i in range(3)], axis=1)
        assert win_keys.shape[0] >= 1 and (np.isin(face_keys, win_keys).sum(axis=1) <= 1).all()      # the winners share no face
        top = int(np.argmin(ev['prio']))
        assert ev['win'][top] and ev['len2'][top] >= ev['len2'][ev['cand']].max() * (1.0 - 2.0 ** -20)
        assert np.unique(ev['prio'][ev['cand']]).shape[0] == int(ev['cand'].sum())
    ratio = S.min_angle(out_v, after) / S.min_angle(verts, before)
    print('{} at {}: {} rounds, {} -> {} faces, smallest angle x {:.3f}'.format(name, factor, info['rounds'], nf, out_f.shape[0], ratio))
    assert ratio >= 0.5 * (1.0 - 1e-3)
    if name.endswith(' shuffled') or name.endswith(' invalid'):
        plain = spec(name.rsplit(' ', 1)[0], factor)
        assert plain[2].tobytes() == out_v.tobytes() and plain[4].tobytes() == ends.tobytes() and plain[5]['added'] == info['added']
        assert np.array_equal(rows_sorted(S.live(plain[3], out_v.shape[0])), rows_sorted(after))
    if name.startswith('cube') and not name.startswith('cubes'):
        assert decimate_spec.signed_volume(verts, before) == 512.0 and decimate_spec.signed_volume(out_v, after) == 512.0
    if name.startswith('cubes welded'):
        assert int((owners0 > 2).sum()) == 1


def test_the_fixtures_are_what_they_say():
    assert len(S.CASES) == len(set(S.CASES)) == 35 and len(S.hand_cases()) == 10
    for name in S.CASES:
        verts, faces = S.case(name)
        assert verts.dtype == np.float32 and faces.dtype == np.int64 and faces.ndim == 2 and faces.shape[1] == 3 and faces.flags['C_CONTIGUOUS'], name
    for b in S.BASES:
        verts, faces = S.base(b)
        assert S.valid_faces(faces, verts.shape[0]).all()
        bad = S.case(b + ' invalid')[1]
        assert bad.shape[0] == faces.shape[0] + 3 and not S.valid_faces(bad, verts.shape[0])[[3, min(10, faces.shape[0] + 1), min(11, faces.shape[0] + 2)]].any()
        mixed = S.case(b + ' shuffled')[1]
        assert mixed.tobytes() != faces.tobytes() and np.array_equal(rows_sorted(mixed), rows_sorted(faces))
    assert S.base('cube')[1].shape[0] == 768 and S.base('sphere')[1].shape[0] == 1280 and S.base('torus')[1].shape[0] == 1024
    assert 30000 < spec('sphere', 0.26)[5]['faces_out'] < 60000
    verts, faces = S.hostile()
    big = S.hostile(1e38)[0]
    assert np.isfinite(big).all() and 0.99e38 < float(np.abs(big).max()) <= 1.0e38 and faces.shape[0] == 288 and verts.shape[0] == 169


def test_max_rounds_and_max_faces_are_bounds_that_apply_nothing_by_halves():
    verts, faces, out_v, out_f, ends, info, trace = spec('sphere decimated', 0.5)
    assert info['rounds'] >= 3
    one = S.subdivide_spec(verts, faces, max_edge=info['max_edge'], max_rounds=1)
    assert one[3]['rounds'] == 1 and not one[3]['converged'] and not one[3]['limited'] and one[3]['candidates_out'] > 0 and one[3]['added'] == info['added'][:1]
    assert S.subdivide_spec(one[0], one[1], max_edge=info['max_edge'])[3]['candidates_in'] == one[3]['candidates_out']
    whole = S.subdivide_spec(verts, faces, max_edge=info['max_edge'], max_rounds=info['rounds'])      # the last allowed round empties the list
    assert whole[3]['converged'] and whole[1].tobytes() == out_f.tobytes()
    # a budget one face below what the third round needs: two rounds are applied in full and nothing of the third
    two = S.subdivide_spec(verts, faces, max_edge=info['max_edge'], max_rounds=2)
    need = two[3]['faces_out'] + int(trace[2][2]['hit'].sum())
    short = S.subdivide_spec(verts, faces, max_edge=info['max_edge'], max_faces=need - 1)
    assert short[3]['limited'] and not short[3]['converged'] and short[3]['rounds'] == 2 and short[3]['max_faces'] == need - 1
    assert short[0].tobytes() == two[0].tobytes() and short[1].tobytes() == two[1].tobytes() and short[2].tobytes() == two[2].tobytes()
    assert short[3]['candidates_out'] == two[3]['candidates_out'] > 0 and short[3]['faces_out'] <= need - 1
    enough = S.subdivide_spec(verts, faces, max_edge=info['max_edge'], max_faces=need, max_rounds=3)
    assert not enough[3]['limited'] and enough[3]['rounds'] == 3 and enough[3]['faces_out'] == need
    none = S.subdivide_spec(verts, faces, max_edge=info['max_edge'], max_faces=faces.shape[0])
    assert none[3]['limited'] and none[3]['rounds'] == 0 and none[1].tobytes() == faces.tobytes() and none[0].tobytes() == verts.tobytes()
    # the same bound through factor and through the max_edge it reports
    assert S.subdivide_spec(verts, faces, max_edge=info['max_edge'])[1].tobytes() == out_f.tobytes()


def test_fmix32_and_the_priority_word():
    assert int(S.fmix32(0)) == 0 and int(S.fmix32(1)) == 0x514E28B7 and int(S.fmix32(0xFFFFFFFF)) == 0x81F16F39
    r = np.arange(1 << 16)
    assert np.unique(S.fmix32(r)).shape[0] == r.shape[0] and S.fmix32(r).dtype == np.uint32
    # longest first: the larger len2, the smaller the high word, from the smallest subnormal to the largest double
    len2 = np.array([np.finfo(np.float64).max, 4.6e77, 16.0, 8.0, 8.0 * (1 + 2.0 ** -19), 1e-60, 5e-324], dtype=np.float64)
    high = S.INF_HIGH - (len2.view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert high[0] == 1 and high[-1] == S.INF_HIGH and (np.diff(high[[0, 1, 2, 4, 3, 5, 6]]) > 0).all()
    assert int(S.NONE) == 2 ** 64 - 1 and S.MAX_FACES == 1431655765
    verts = np.array([[0, 0, 0], [4, 0, 0]], dtype=np.float32)
    len2, prio = S.edge_priorities(np.array([1, 1], dtype=np.int64), verts, 1.0)
    assert len2.tolist() == [16.0, 16.0] and [int(p) for p in prio] == [((0x7FF00000 - 0x40300000) << 32) | 0, ((0x7FF00000 - 0x40300000) << 32) | 0x514E28B7]
    keys = np.array([1, -1, (1 << 32) | 1, (1 << 32) | 0, 2, S.SENTINEL], dtype=np.int64)
    len2, prio = S.edge_priorities(keys, verts, 1.0)
    assert len2.tolist() == [16.0, 0, 0, 0, 0, 0] and (prio[1:] == S.NONE).all() and prio[0] != S.NONE


def test_midpoint_colours_are_rounded_means_round_by_round():
    from ppsurf_amd import subdivide
    verts, faces, out_v, out_f, ends, info, _ = spec('sphere decimated', 0.5)
    rgb = np.random.default_rng(3).integers(0, 256, size=(verts.shape[0], 4)).astype(np.uint8)
    got = subdivide.midpoint_colors(rgb, ends, info['added'])
    assert got.dtype == np.uint8 and got.shape == (out_v.shape[0], 4) and got.tobytes() == S.interpolate_colors(rgb, ends, info['added']).tobytes()
    assert (ends >= verts.shape[0]).any()                                                 # an end that is itself new: the rounds matter
    assert subdivide.midpoint_colors(np.array([[0, 255], [1, 255]], dtype=np.uint8), [[0, 1]], [1]).tolist() == [[0, 255], [1, 255], [1, 255]]
    assert subdivide.midpoint_colors(rgb, np.zeros((0, 2)), []).tobytes() == rgb.tobytes()


def test_split_long_edges_argument_rules():
    import torch
    from ppsurf_amd import subdivide
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for kw in (dict(), dict(max_edge=1.0, factor=1.0), dict(max_edge=None, factor=None)):
        with pytest.raises(ValueError, match='exactly one'):
            subdivide.split_long_edges(v, f, **kw)
    for bad in (0, 0.0, -1, float('nan'), float('inf'), True, '1', [1.0]):
        with pytest.raises(ValueError, match='max_edge'):
            subdivide.split_long_edges(v, f, max_edge=bad)
        with pytest.raises(ValueError, match='factor'):
            subdivide.split_long_edges(v, f, factor=bad)
    for bad in (0, -1, 2 ** 31, 1.0, 10.5, True, '3', None):
        with pytest.raises(ValueError, match='max_rounds'):
            subdivide.split_long_edges(v, f, max_edge=1.0, max_rounds=bad)
    for bad in (-1, (2 ** 32 - 1) // 3 + 1, 1.0, True, '3'):
        with pytest.raises(ValueError, match='max_faces'):
            subdivide.split_long_edges(v, f, factor=1.0, max_faces=bad)
    assert subdivide._checked_params(2, None, np.int64(7), None) == (2.0, None, 7, (2 ** 32 - 1) // 3)
    assert subdivide._checked_params(None, np.float32(0.5), 2 ** 31 - 1, np.int64(0)) == (None, 0.5, 2 ** 31 - 1, 0)
    # good parameters, CPU tensors: the device guard of the other mesh stages, after the parameters
    for fn in (lambda: subdivide.split_long_edges(v, f, 1.0), lambda: subdivide.split_long_edges(v, f, factor=0.5, return_ends=True)):
        with pytest.raises(subdivide.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(subdivide.CpuTensorError, PpsError) and issubclass(subdivide.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='split_long_edges: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        subdivide.split_long_edges(v, f, max_edge=0.5)
    assert subdivide.MAX_FACES == S.MAX_FACES and subdivide.MAX_COUNT == S.MAX_VERTS


@pytest.mark.parametrize('argv', [['m.ply'], [], ['m.ply', 'o.ply'], ['m.ply', 'o.obj', '--factor', '1'], ['m.ply', 'o.ply', '--max_edge', '0'],
                                  ['m.ply', 'o.ply', '--max_edge', '1', '--factor', '1'], ['m.ply', 'o.ply', '--factor', 'nan'],
                                  ['m.ply', 'o.ply', '--factor', '-1'], ['m.ply', 'o.ply', '--factor'], ['m.ply', 'o.ply', '--max_edge', 'inf'],
                                  ['m.ply', 'o.ply', '--factor', '1', '--max_rounds', '0'], ['m.ply', 'o.ply', '--factor', '1', '--max_rounds', '1.5'],
                                  ['m.ply', 'o.ply', '--factor', '1', '--max_faces', '-1'], ['m.ply', 'o.ply', '--factor', '1', '--max_faces', '1431655766'],
                                  ['m.ply', 'o.ply', '--factor', '1', '--gen_subdivide', '1']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import subdivide
    with pytest.raises(SystemExit) as e:
        subdivide.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_help_text_names_the_guard(capsys):
    from ppsurf_amd import subdivide
    with pytest.raises(SystemExit) as e:
        subdivide.main(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert e.value.code == 0 and '--max_faces' in text and 'guard against a typo' in text and 'grows like' in text


def test_the_subdivide_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P, F64 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_subdivide_edges'] == (I, [P, I64, P, I64, F64, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_subdivide_votes'] == (I, [P, I64, P, I64, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_subdivide_winners'] == (I, [P, P, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_subdivide_hits'] == (I, [P, P, I64, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_subdivide_emit'] == (I, [P, I64, P, P, P, I64, I64, P, I64, P, P, P, P, I64, P, P, P, P])
    assert _lib.EXT_PARAMS['ppsx_subdivide_edges'] == ['keys', 'ne', 'verts', 'nv', 'max2', 'len2', 'prio', 'stream']
    assert _lib.EXT_PARAMS['ppsx_subdivide_votes'] == ['run_of', 'nf', 'prio', 'ne', 'choice', 'votes', 'stream']
    assert _lib.EXT_PARAMS['ppsx_subdivide_winners'] == ['prio', 'votes', 'owners', 'ne', 'win', 'stream']
    assert _lib.EXT_PARAMS['ppsx_subdivide_hits'] == ['run_of', 'choice', 'nf', 'win', 'ne', 'hit', 'stream']
    assert _lib.EXT_PARAMS['ppsx_subdivide_emit'] == ['verts', 'nv', 'keys', 'win', 'vslot', 'ne', 'nw', 'faces', 'nf', 'run_of', 'choice', 'hit', 'fslot',
                                                      'nh', 'new_verts', 'ends', 'out', 'stream']
    sites = call_sites.ext_call_sites('ppsx_subdivide')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'subdivide.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {n: 1 for n in _lib.EXT_PARAMS if n.startswith('ppsx_subdivide_')} and len(sites) == 5
    # subdivide.py calls no other stage's entries; the edges come through the topology layer, which holds the one call of the key entry
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'subdivide.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(sites) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert [path for path, _, _ in call_sites.ext_call_sites('ppsx_pieces_edge_keys')['ppsx_pieces_edge_keys']] == ['topology.py']
    assert 'pps_subdivide.hip' in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, 'pps_subdivide.hip'))
    kernel_source = open(os.path.join(build.CSRC, 'pps_subdivide.hip')).read()
    assert 'pps_labels.h' not in kernel_source and 'atomicAdd(votes' in kernel_source and '__shared__' not in kernel_source
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(sites) <= set(_lib._ext_entries)
    # the specification shares no code with the module
    spec_source = open(os.path.join(call_sites.REPO, 'tests', 'subdivide_spec.py')).read()
    assert 'ppsurf_amd' not in re.sub(r'""".*?"""', '', spec_source, flags=re.S)
