"""Host tier of the self-intersection stage: the numpy specification tests/intersect_spec.py against things that do not
know its rule -- an exact oracle in rational arithmetic on random integer triangles, the counts of the issue recomputed, and invariants
(order of the faces, power-of-two scalings, flags against pairs, convex meshes) -- and the parts of ppsurf_amd/intersect.py that need no
GPU: the parameter checks and the argument errors of the command."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import call_sites
import intersect_spec as S


# ---- the exact oracle ----------------------------------------------------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _span(tri, s, line):
    """The closed interval of the parameters dot(line, x) of the points x of the triangle that lie in the other plane; s the signed
    distances of its corners to that plane (integers, not normalised)."""
    at = [Fraction(_dot(line, tri[i])) for i in range(3) if s[i] == 0]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        if s[i] * s[j] < 0:
            at.append(_dot(line, tri[i]) + Fraction(s[i], s[i] - s[j]) * _dot(line, _sub(tri[j], tri[i])))
    return min(at), max(at)


def oracle(t1, t2, k1=None, k2=None):
    """'crossing', 'apart' or 'contact' of two triangles with integer corners, exactly.  k1, k2: the corners of a shared vertex.
    crossing: the planes differ, no corner other than the shared one lies in the other plane, and the two closed triangles have a segment of
    positive length in common.  apart: the corners of one (other than the shared one) lie strictly on one side of the other's plane, or the
    two triangles meet the common line of the planes in disjoint intervals.  Everything else is contact."""
    n1, n2 = _cross(_sub(t1[1], t1[0]), _sub(t1[2], t1[0])), _cross(_sub(t2[1], t2[0]), _sub(t2[2], t2[0]))
    if n1 == (0, 0, 0) or n2 == (0, 0, 0):
        return 'contact'                                              # a zero-area face
    s2, s1 = [_dot(n1, _sub(p, t1[0])) for p in t2], [_dot(n2, _sub(p, t2[0])) for p in t1]
    o2, o1 = [s for j, s in enumerate(s2) if j != k2], [s for i, s in enumerate(s1) if i != k1]
    for other in (o1, o2):
        if all(s > 0 for s in other) or all(s < 0 for s in other):
            return 'apart'
    line = _cross(n1, n2)
    if line == (0, 0, 0):
        return 'contact'                                              # one plane (distinct parallel planes are apart above)
    lo1, hi1 = _span(t1, s1, line)
    lo2, hi2 = _span(t2, s2, line)
    if hi1 < lo2 or hi2 < lo1:
        return 'apart'
    if all(s != 0 for s in o1 + o2) and min(hi1, hi2) > max(lo1, lo2):
        return 'crossing'
    return 'contact'


def test_the_oracle_knows_the_hand_made_pairs():
    flat = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    assert oracle(flat, [(1, 1, -1), (1, 1, 1), (5, 5, 0)]) == 'contact'                  # (5, 5, 0) lies in the plane: the rule may say either
    assert oracle(flat, [(1, 2, -1), (1, 2, 1), (5, 3, 1)]) == 'crossing'
    assert oracle(flat, [(1, 1, 1), (1, 1, 2), (5, 5, 1)]) == 'apart'
    assert oracle(flat, [(9, 9, -1), (9, 9, 1), (9, 8, 1)]) == 'apart'                    # through the plane, beside the triangle
    assert oracle(flat, [(0, 0, 0), (1, 1, -1), (1, 1, 1)], 0, 0) == 'crossing'
    assert oracle(flat, [(0, 0, 0), (1, 1, 1), (2, 1, 2)], 0, 0) == 'apart'
    assert oracle(flat, [(0, 0, 0), (-1, -1, -1), (-1, -2, 1)], 0, 0) == 'contact'        # through the plane, but the triangles meet at the vertex alone
    assert oracle(flat, [(1, 1, 0), (2, 1, 0), (1, 2, 0)]) == 'contact' and oracle(flat, [(1, 1, 0), (2, 2, 0), (3, 3, 0)]) == 'contact'
    assert oracle(flat, [(1, 1, 3), (2, 1, 3), (1, 2, 3)]) == 'apart'


@pytest.mark.parametrize('share', [False, True])
def test_the_rule_agrees_with_the_exact_oracle_on_integer_triangles(share):
    rng = np.random.default_rng(290 + share)
    m = 4000
    verts, faces, verdicts = [], [], []
    for i in range(m):
        p = rng.integers(-8, 9, size=(6, 3))
        base = 6 * i
        if share:                                                    # one shared index, at a random corner of each face
            k1, k2 = int(rng.integers(3)), int(rng.integers(3))
            f, g = [1, 2], [3, 4]
            f.insert(k1, 0)
            g.insert(k2, 0)
        else:
            k1 = k2 = None
            f, g = [0, 1, 2], [3, 4, 5]
        verdicts.append(oracle([tuple(p[j].tolist()) for j in f], [tuple(p[j].tolist()) for j in g], k1, k2))
        verts.append(p)
        faces += [[base + j for j in f], [base + j for j in g]]
    verts, faces = np.concatenate(verts).astype(np.float32), np.array(faces, dtype=np.int64)
    boxed, crosses = S.judge(verts, faces, np.arange(0, 2 * m, 2), np.arange(1, 2 * m, 2))
    verdicts = np.array(verdicts)
    counts = {k: int((verdicts == k).sum()) for k in ('crossing', 'apart', 'contact')}
    print('shared vertex' if share else 'no shared vertex', counts, 'flagged', int(crosses.sum()), 'boxed', int(boxed.sum()))
    assert crosses[verdicts == 'crossing'].all()                     # every crossing pair is flagged (and so boxed)
    assert not crosses[verdicts == 'apart'].any()                    # no pair that is apart is flagged
    assert (crosses <= boxed).all() and counts['crossing'] > 200 and counts['apart'] > 2000
    assert counts['contact'] <= 0.05 * m, counts                     # the excluded share: a condition of this test
    # and the same verdicts from the other face of every pair
    boxed_back, crosses_back = S.judge(verts, faces, np.arange(1, 2 * m, 2), np.arange(0, 2 * m, 2))
    assert np.array_equal(boxed, boxed_back) and np.array_equal(crosses, crosses_back)


# ---- the counts of the issue, recomputed ---------------------------------------------------------------------------------------------------------
def test_the_counts_on_the_clean_cases():
    want = {'icosphere': (320, 0, 0), 'icosphere noisy': (320, 0, 0), 'cube': (192, 0, 0), 'two icospheres': (640, 88, 88),
            'two cubes 1.5': (384, 90, 60), 'two cubes 2': (384, 0, 0)}
    for name, (nf, pairs, flagged) in want.items():
        verts, faces = S.clean(name)
        flags, got, info = S.intersect_spec(verts, faces)
        assert (info['faces_in'], info['faces_live'], info['pairs'], info['faces_intersecting']) == (nf, nf, pairs, flagged), (name, info)
        # the rows that are not live change no verdict: the same pairs between the same faces with them mixed in
        bad_v, bad_f = S.case(name)
        bad_flags, bad_pairs, bad_info = S.intersect_spec(bad_v, bad_f)
        assert (bad_info['faces_in'], bad_info['faces_live'], bad_info['pairs']) == (nf + 7, nf, pairs), name
        live = np.nonzero(S.live_faces(bad_v, bad_f))[0]
        assert np.array_equal(bad_f[live], faces) and np.array_equal(live[got], bad_pairs) and not bad_flags[~S.live_faces(bad_v, bad_f)].any()
    verts, faces = S.clean('two icospheres')
    pairs = S.intersect_spec(verts, faces)[1]
    assert ((pairs[:, 0] < 320) & (pairs[:, 1] >= 320)).all()         # every pair has one face of each sphere
    verts, faces = S.clean('large triangle')
    pairs, ext = S.intersect_spec(verts, faces)[1], S.boxes(verts, faces)[2]
    assert pairs.shape[0] > 20 and (pairs[:, 1] == 320).all() and ext[320] > 4 * ext[:320].max()
    info = S.intersect_spec(*S.case('soup'))[2]
    assert info['faces_live'] == 300 and info['pairs'] > 50
    assert S.intersect_spec(*S.case('empty'))[2]['faces_in'] == 0 and S.intersect_spec(*S.case('nothing live'))[2] == dict(
        faces_in=7, faces_live=0, faces_intersecting=0, pairs=0, boxed_pairs=0, pairs_listed=True, max_pairs=S.MAX_PAIRS)


def test_the_hand_made_pairs():
    for name, verts, faces, want in S.hand_cases():
        flags, pairs, info = S.intersect_spec(verts, faces)
        assert pairs.tolist() == want and flags.tolist() == [bool(want)] * 2, name
    names = [c[0] for c in S.hand_cases()]
    assert {'piercing', 'shared vertex crossing', 'shared vertex touching', 'folded flat', 'two copies', 'through a vertex'} <= set(names)
    boxed = {c[0]: S.intersect_spec(c[1], c[2])[2]['boxed_pairs'] for c in S.hand_cases()}
    assert boxed['folded flat'] == boxed['two copies'] == 0 and boxed['shared vertex touching'] == boxed['through a vertex'] == 1


# ---- invariants ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', S.CASES)
def test_invariants_of_the_rule(name):
    verts, faces = S.case(name)
    nf = faces.shape[0]
    flags, pairs, info = S.intersect_spec(verts, faces)
    assert flags.dtype == bool and pairs.dtype == np.int64 and pairs.shape == (info['pairs'], 2)
    marked = np.zeros(nf, dtype=bool)
    marked[pairs.reshape(-1)] = True
    assert np.array_equal(flags, marked) and info['faces_intersecting'] == int(flags.sum())      # flagged exactly when in a pair
    keys = (pairs[:, 0] << 32) | pairs[:, 1]
    assert (pairs[:, 0] < pairs[:, 1]).all() and (np.diff(keys) > 0).all()                       # strictly ascending
    assert info['boxed_pairs'] >= info['pairs'] and not flags[~S.live_faces(verts, faces)].any()
    # the order of the faces: a random permutation, the rows mapped back
    perm = np.random.default_rng(5).permutation(nf)
    p_flags, p_pairs, p_info = S.intersect_spec(verts, faces[perm])
    back = perm[p_pairs] if p_pairs.shape[0] else p_pairs
    back = np.stack([back.min(axis=1), back.max(axis=1)], axis=1) if back.shape[0] else back
    assert p_info == info and np.array_equal(p_flags, flags[perm])
    assert np.array_equal(back[np.lexsort((back[:, 1], back[:, 0]))], pairs)
    # exact scalings
    for scale in (2.0 ** 40, 2.0 ** -40):
        scaled = (verts.astype(np.float64) * scale).astype(np.float32)
        assert np.array_equal(scaled.astype(np.float64) / scale, verts.astype(np.float64), equal_nan=True)
        s_flags, s_pairs, s_info = S.intersect_spec(scaled, faces)
        assert s_info == info and np.array_equal(s_flags, flags) and np.array_equal(s_pairs, pairs)
    # max_pairs: nothing listed one below the count, everything at it
    if info['pairs']:
        short = S.intersect_spec(verts, faces, info['pairs'] - 1)
        assert short[1].shape == (0, 2) and not short[2]['pairs_listed'] and np.array_equal(short[0], flags) and short[2]['pairs'] == info['pairs']
        assert S.intersect_spec(verts, faces, info['pairs'])[2]['pairs_listed']


def test_closed_convex_meshes_have_no_pair_and_the_cut_mesh_has_none_left():
    import decimate_spec
    import eval_spec
    for verts, faces in (eval_spec.icosphere(0), eval_spec.icosphere(3), S.cube(), decimate_spec.tetrahedron()):
        info = S.intersect_spec(np.asarray(verts, dtype=np.float32), faces)[2]
        assert info['pairs'] == 0 and info['faces_live'] == info['faces_in'] and (info['boxed_pairs'] > 0) == (info['faces_in'] > 4)      # a tetrahedron's faces all share an edge
    # what remove_self_intersections leaves of the two spheres: nothing crosses among the kept faces (the downstream test of the GPU tier)
    verts, faces = S.clean('two icospheres')
    kept, rows = S.removed(faces, S.intersect_spec(verts, faces)[0])
    assert kept.shape[0] == 640 - 88 and np.array_equal(faces[rows], kept) and S.intersect_spec(verts, kept)[2]['pairs'] == 0


def test_boxes_and_the_rounded_up_extent():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1e-30, 3e38, -3e38], [0.1, 0.2, 0.3], [np.nan, 0, 0], [0, -3e38, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 4], [0, 1, 5], [0, 1, 1], [0, 1, 7], [3, 6, 1]], dtype=np.int64)
    lo, hi, ext, live = S.boxes(verts, faces)
    assert live.tolist() == [1, 1, 0, 0, 0, 1] and ext[0] == 1.0 and (lo[2:5] == 0).all() and (hi[2:5] == 0).all() and (ext[2:5] == 0).all()
    assert np.array_equal(lo[1], [0, 0, np.float32(-3e38)]) and np.array_equal(hi[1], [np.float32(0.1), np.float32(3e38), np.float32(0.3)])
    assert ext[1] == np.float32(3e38) and ext[5] == np.inf                                     # 6e38 is above the largest float
    # rounded UP: the fp64 difference of two floats need not be a float
    x = S.ru32(np.array([1.0 + 2.0 ** -30, 1.0, 0.0, 1e300]))
    assert x.tolist() == [float(np.nextafter(np.float32(1), np.float32(2))), 1.0, 0.0, np.inf]


# ---- the host parts of the module ------------------------------------------------------------------------------------------------------------------
def test_parameter_checks_come_first_and_cpu_tensors_are_refused():
    from ppsurf_amd import intersect, topology
    verts, faces = (torch.from_numpy(a) for a in S.clean('cube'))
    for bad in (-1, 2 ** 31, 1.5, '3', None, True, np.float32(2)):
        with pytest.raises(ValueError, match='max_pairs must be an integer in 0'):
            intersect.self_intersections(verts, faces, max_pairs=bad)
    assert intersect._checked_params(0) == 0 and intersect._checked_params(np.int64(7)) == 7 and intersect._checked_params(2 ** 31 - 1) == 2 ** 31 - 1
    with pytest.raises(intersect.CpuTensorError, match='no CPU'):
        intersect.self_intersections(verts, faces)
    with pytest.raises(intersect.CpuTensorError, match='no CPU'):
        intersect.remove_self_intersections(verts, faces)
    assert intersect.CpuTensorError is topology.CpuTensorError and intersect.MAX_PAIRS == S.MAX_PAIRS == 2 ** 24
    # the finite check of the other stages is as it was; this stage alone switches it off
    nan = torch.tensor([[0.0, 0.0, float('nan')]] * 3)
    with pytest.raises(ValueError, match='non-finite'):
        topology.checked_mesh('x', nan, faces[:1])
    assert topology.checked_mesh('x', nan.double(), faces[:1], limit=True, finite=False)[0].dtype == torch.float32


@pytest.mark.parametrize('argv', [[], ['m.ply', 'o.obj'], ['m.ply', '--action', 'select'], ['m.ply', 'o.ply', '--action', 'cut'],
                                  ['m.ply', '--max_pairs', '-1'], ['m.ply', '--max_pairs', '2147483648'], ['m.ply', '--max_pairs', '1.5'],
                                  ['m.ply', '--pairs_out', 'pairs.txt'], ['m.ply', 'o.ply', 'p.ply'], ['m.ply', 'o.ply', '--gen_intersect', '1']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import intersect
    with pytest.raises(SystemExit) as e:
        intersect.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_help_text_says_what_is_not_detected(capsys):
    from ppsurf_amd import intersect
    with pytest.raises(SystemExit) as e:
        intersect.main(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert e.value.code == 0 and 'weld first' in text and 'not detected' in text and '--pairs_out' in text and 'remove,select' in text
    assert 'weld' in intersect.__doc__ and 'NOT detected' in intersect.__doc__ and 'coplanar' in intersect.self_intersections.__doc__


def test_the_intersect_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P, F32 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    walk = [P, I64, P, I64, P, P, P, P, I64, P, P, F32, F32, P, I64, P, P, P, I64]
    names = ['verts', 'nv', 'faces', 'nf', 'lo', 'hi', 'live', 'small', 'ns', 'glo', 'ghi', 'h', 'inv_h', 'table', 'capacity', 'order', 'offsets', 'large', 'nl']
    assert _lib.EXT_SIGNATURES['ppsx_intersect_boxes'] == (I, [P, I64, P, I64, P, P, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_intersect_count'] == (I, walk + [P, P, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_intersect_emit'] == (I, walk + [P, P, I64, P, P])
    assert _lib.EXT_PARAMS['ppsx_intersect_boxes'] == ['verts', 'nv', 'faces', 'nf', 'lo', 'hi', 'ext', 'live', 'stream']
    assert _lib.EXT_PARAMS['ppsx_intersect_count'] == names + ['flag', 'count', 'boxed', 'stream']
    assert _lib.EXT_PARAMS['ppsx_intersect_emit'] == names + ['count', 'pair_offsets', 'np', 'pairs', 'stream']
    sites = call_sites.ext_call_sites('ppsx_intersect')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'intersect.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {n: 1 for n in _lib.EXT_PARAMS if n.startswith('ppsx_intersect_')} and len(sites) == 3
    # intersect.py calls no other stage's entries: the cell lists come through trim.SupportGrid, which holds the one call of the slot entry
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'intersect.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(sites) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert 'pps_intersect.hip' in build.SOURCES and len(call_sites.ext_call_sites('ppsx_trim_cell_slots')['ppsx_trim_cell_slots']) == 1
