"""CPU tier of the isotropic remeshing: the numpy specification tests/remesh_spec.py against invariants -- topology kept,
borders byte for byte, the fixed point of the collapse, the length guard, planted needles removed, the tangential step on a plane, the
volume against plain Laplacian smoothing, the states against a scalar restatement -- the loop against the chain written by hand and against
the quality of its input, and the parameter rules and the declarations of ppsurf_amd/remesh.py.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import call_sites
import decimate_spec as DS
import flip_spec
import intersect_spec
import remesh_spec as R
import smooth_spec
import subdivide_spec

D = np.float64
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64).tobytes()


def mesh(name):
    if name not in _cache:
        if name == 'needles':
            _cache[name] = R.needles()[:2]
        elif name == 'spindle':
            _cache[name] = R.spindle()
        elif name == 'open fan':
            _cache[name] = smooth_spec.fan(300)
        elif name == 'torus16x8':
            _cache[name] = DS.torus(16, 8)
        else:
            _cache[name] = DS.named(name)[:2]
    return _cache[name]


def median(name):
    v, f = mesh(name)
    return subdivide_spec.median_edge(v, f)


def collapsed(name, low, high):
    """collapse_rows_spec of a named mesh with the bounds as multiples of its median edge, computed once."""
    key = ('collapse', name, low, high)
    if key not in _cache:
        v, f = mesh(name)
        L = median(name)
        _cache[key] = R.collapse_rows_spec(v, f, low * L, None if high is None else high * L)
    return _cache[key]


def remeshed(name):
    key = ('remesh', name)
    if key not in _cache:
        _cache[key] = R.remesh_spec(*mesh(name), factor=1.0)
    return _cache[key]


# ---- collapse ----------------------------------------------------------------------------------------------------------------------------------
CLOSED = {'sphere': 2, 'torus': 0, 'cube8': 2, 'spindle': 2, 'needles': 2}


@pytest.mark.parametrize('name', sorted(CLOSED))
@pytest.mark.parametrize('high', [None, 4.0 / 3.0])
def test_a_closed_manifold_stays_closed_and_manifold_with_its_euler_characteristic(name, high):
    v, f = mesh(name)
    assert DS.closed_manifold(v, f) and DS.euler(v, f) == CLOSED[name]
    kept, out_v, out_f, info = collapsed(name, 1.1, high)
    assert DS.closed_manifold(out_v, out_f) and DS.euler(out_v, out_f) == CLOSED[name]
    assert info['vertices_out'] == out_v.shape[0] == info['vertices_in'] - info['collapses'] and info['faces_out'] == info['faces_in'] - 2 * info['collapses']
    if high is None or name in ('sphere', 'torus', 'needles'):         # on the regular cube and the spindle the length guard refuses all
        assert info['collapses'] > 0, info
    # the sign of the volume is kept: no collapse turned the surface inside out
    assert DS.signed_volume(out_v, out_f) * DS.signed_volume(v, f) > 0


@pytest.mark.parametrize('name', ['patch', 'open fan', 'welded'])
def test_border_and_non_regular_vertices_come_back_byte_for_byte(name):
    v, f = mesh(name)
    kept, out_v, out_f, info = collapsed(name, 1.5, None)
    r = R.mesh_rows(f, v.shape[0])
    locked = np.nonzero(~r['regular'] & (np.bincount(f.reshape(-1), minlength=v.shape[0]) > 0))[0]
    assert locked.shape[0] > 0 and info['locked_vertices'] == int((~r['regular']).sum())
    assert np.isin(locked, kept).all()
    at = np.searchsorted(kept, locked)
    assert bits(out_v[at]) == bits(v[locked])
    if name == 'patch':
        assert info['collapses'] > 0                                   # the interior did collapse
        assert sorted(map(tuple, np.sort(out_v[DS.border_vertices(out_f, out_v.shape[0])], axis=0).tolist())) == \
            sorted(map(tuple, np.sort(v[DS.border_vertices(f, v.shape[0])], axis=0).tolist()))
    if name == 'welded':
        assert info['locked_vertices'] == 2                            # the two vertices of the welded edge; the regular ones may collapse


@pytest.mark.parametrize('name,low,high', [('sphere', 1.1, None), ('sphere', 1.1, 4.0 / 3.0), ('torus', 1.1, None), ('needles', 0.5, None),
                                           ('patch', 1.5, None)])
def test_at_converged_a_fresh_evaluation_has_no_candidate(name, low, high):
    kept, out_v, out_f, info = collapsed(name, low, high)
    assert info['converged'] and info['rounds'] >= 1
    min2, max2 = R.bounds2(low * median(name), None if high is None else high * median(name))
    again = R.round_spec(out_v.astype(D), out_f, out_v.shape[0], min2, max2)
    # the output is rounded to float32 once: an edge may land on the other side of the bound only by that rounding, and none does here
    assert int((again['prio'][:, 0] != R.NONE).sum()) == 0
    v, f = mesh(name)
    limited = R.collapse_spec(v, f, low * median(name), None if high is None else high * median(name), max_rounds=1)[2]
    assert limited['rounds'] == 1 and limited['converged'] == (info['rounds'] == 1)


@pytest.mark.parametrize('name', ['sphere', 'torus', 'needles'])
def test_with_max_edge_no_edge_grows_beyond_the_longer_of_the_bound_and_the_longest_input_edge(name):
    v, f = mesh(name)
    L = median(name)
    kept, out_v, out_f, info = collapsed(name, 1.1, 4.0 / 3.0)
    free = collapsed(name, 1.1, None)
    assert info['collapses'] > 0 and free[3]['collapses'] > info['collapses']          # the guard refused collapses that +inf admits
    longest_in, longest_out = R.edge_lengths(v, f).max(), R.edge_lengths(out_v, out_f).max()
    print('longest edge in {!r} out {!r} bound {!r}'.format(longest_in, longest_out, 4.0 / 3.0 * L))
    assert longest_out <= max(longest_in, 4.0 / 3.0 * L)
    assert R.edge_lengths(free[1], free[2]).max() > max(longest_in, 4.0 / 3.0 * L) or name == 'needles'


def test_every_planted_needle_is_removed():
    v, f, planted = R.needles()
    assert planted.shape[0] == R.PLANTED == 12
    L = subdivide_spec.median_edge(v, f)
    lengths = R.edge_lengths(v, f)
    assert int((lengths < 0.01 * L * 1.2).sum()) == R.PLANTED and int((lengths < 0.5 * L).sum()) == R.PLANTED
    kept, out_v, out_f, info = collapsed('needles', 0.5, None)
    assert info['vertices_out'] == info['vertices_in'] - R.PLANTED == 630 and info['collapses'] == info['candidates'] == R.PLANTED
    assert info['rounds'] == 1 and info['converged']                  # no two planted vertices are within three rings: one round takes all
    assert R.edge_lengths(out_v, out_f).min() > 0.5 * L
    # the smallest angle: the needles were the only corners below a degree
    assert flip_spec.min_angle(v, f) < 1.0 and flip_spec.min_angle(out_v, out_f) > 10.0


def test_meshes_without_a_candidate_come_back_as_given():
    for v, f, bound in (DS.tetrahedron() + (10.0,), DS.octahedron() + (1.0,), mesh('sphere') + (0.01,),
                        (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 1.0), (mesh('sphere')[0], np.array([[0, 0, 1], [-1, 2, 3]]), 1.0)):
        kept, out_v, out_f, info = R.collapse_rows_spec(v, f, bound)
        assert bits(out_v) == bits(v) and bits(out_f) == bits(np.asarray(f, dtype=np.int64)) and kept.tolist() == list(range(v.shape[0]))
        assert info['collapses'] == 0 and info['rounds'] == 0 and info['converged'] and info['vertices_out'] == v.shape[0]
    # every edge of the tetrahedron is short, and the link rule refuses them all
    assert R.collapse_spec(*DS.tetrahedron(), 10.0)[2]['candidates'] == 0


def test_an_edge_of_length_zero_qualifies_and_a_face_without_area_at_an_end_blocks():
    v, f = mesh('sphere')
    r = R.mesh_rows(f, v.shape[0])
    a = 100
    b = int(r['nbr'][r['offsets'][a]])
    twin = v.copy()
    twin[b] = twin[a]                                                  # the edge (a, b) has length 0; its two faces have no area
    kept, out_v, out_f, info = R.collapse_rows_spec(twin, f, 1e-6)
    assert info['candidates'] == 1 and info['collapses'] == 1 and info['vertices_out'] == v.shape[0] - 1
    # a third vertex on the same spot: now a face without area holds one end only of every zero edge
    c = next(int(w) for w in r['nbr'][r['offsets'][a]:r['offsets'][a + 1]] if w != b and w in r['nbr'][r['offsets'][b]:r['offsets'][b + 1]])
    twin[c] = twin[a]
    info = R.collapse_spec(twin, f, 1e-6)[2]
    assert info['candidates'] == 0 and info['collapses'] == 0


# ---- relax -------------------------------------------------------------------------------------------------------------------------------------
def relax_reference(verts, faces, lam):
    """(y float64, state) of one pass, vertex by vertex in plain Python floats: a restatement that shares no code with the specification."""
    x = np.asarray(verts, dtype=np.float32).astype(D)
    nv = x.shape[0]
    ok = R.valid_faces(faces, nv)
    nbrs, fans, owners = [set() for _ in range(nv)], [[] for _ in range(nv)], {}
    for t in np.nonzero(ok)[0].tolist():
        i = faces[t].tolist()
        for k in range(3):
            fans[i[k]].append(t)
            nbrs[i[k]].update((i[(k + 1) % 3], i[(k + 2) % 3]))
            e = (min(i[k], i[(k + 1) % 3]), max(i[k], i[(k + 1) % 3]))
            owners[e] = owners.get(e, 0) + 1

    def cross(p, q, r):
        u, w = [q[k] - p[k] for k in range(3)], [r[k] - p[k] for k in range(3)]
        return [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]

    def dot(p, q):
        return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]

    y, state = x.copy(), np.zeros(nv, dtype=np.uint8)
    for v in range(nv):
        row = sorted(nbrs[v])
        if not fans[v] or len(fans[v]) != len(row) or any(owners[(min(v, w), max(v, w))] != 2 for w in row):
            continue
        s = [0.0, 0.0, 0.0]
        for w in row:
            s = [s[k] + float(x[w, k]) for k in range(3)]
        pv = [float(x[v, k]) for k in range(3)]
        d = [s[k] / float(len(row)) - pv[k] for k in range(3)]
        N = [0.0, 0.0, 0.0]
        for t in sorted(fans[v]):
            n = cross(*[[float(c) for c in x[i]] for i in faces[t]])
            N = [N[k] + n[k] for k in range(3)]
        nn, nd = dot(N, N), dot(N, d)
        if nn == 0.0 or not math.isfinite(nn):
            state[v] = 2
            continue
        ratio = nd / nn
        t_k = [d[k] - N[k] * ratio for k in range(3)]
        if not all(math.isfinite(c) for c in t_k):
            state[v] = 2
            continue
        q = [pv[k] + lam * t_k[k] for k in range(3)]
        keeps = True
        for t in sorted(fans[v]):
            old = [[float(c) for c in x[i]] for i in faces[t]]
            new = [q if i == v else old[k] for k, i in enumerate(faces[t].tolist())]
            keeps = keeps and dot(cross(*old), cross(*new)) > 0
        state[v] = 1 if keeps else 3
        if keeps:
            y[v] = q
    return y, state


@pytest.mark.parametrize('name', ['sphere', 'patch', 'four states', 'welded'])
def test_a_pass_equals_its_scalar_restatement_and_the_states_are_counted_right(name):
    v, f = R.four_states() if name == 'four states' else mesh(name)
    want_y, want_state = relax_reference(v, f, 0.5)
    r = R.mesh_rows(f, v.shape[0])
    y, state = R.relax_pass_spec(v.astype(D), f, r['offsets'], r['nbr'], r['inc_offsets'], r['inc'], r['regular'], 0.5)
    assert state.tolist() == want_state.tolist() and y.tobytes() == want_y.tobytes()
    out_v, out_f, info = R.relax_spec(v, f, 1, 0.5)
    assert info['states'] == np.bincount(want_state, minlength=4).tolist() and info['regular'] == int((want_state != 0).sum()) and out_f is not None
    assert bits(out_v) == bits(want_y.astype(np.float32))
    if name == 'four states':
        # the border of the patch, its interior, the pillow, and the corners 40, 53, 54 of the face without area
        assert info['states'] == [48, 118, 3, 3] and np.nonzero(want_state == 3)[0].tolist() == [40, 53, 54]
        assert np.nonzero(want_state == 2)[0].tolist() == [169, 170, 171]
        assert bits(out_v[want_state != 1]) == bits(v[want_state != 1])


@pytest.mark.parametrize('n', [4, 12])
def test_on_a_plane_the_step_stays_in_the_plane_and_the_border_stays(n):
    v, f = flip_spec.jittered_lattice(n)
    out_v, _, info = R.relax_spec(v, f, 5, 0.5)
    border = DS.border_vertices(f, v.shape[0])
    # N = (0, 0, N_z) and d_z = 0 there, so nd = N_z * 0 = 0, r = 0 and t_z = 0 - N_z * 0 = 0 exactly: z keeps its bytes
    assert bits(out_v[:, 2]) == bits(v[:, 2]) and bits(out_v[border]) == bits(v[border])
    assert info['regular'] == int((~border).sum()) == (n - 1) ** 2 and info['states'][0] == int(border.sum())
    assert info['moved'] == info['states'][1] > 0 and (out_v[~border, :2] != v[~border, :2]).any()
    assert (flip_spec.areas2(out_v, f) > 0).all()                      # no triangle turned over
    assert R.edge_cv(out_v, f) < R.edge_cv(v, f)


def test_the_volume_moves_less_than_under_plain_laplacian_smoothing():
    v, f = mesh('sphere')
    before = DS.signed_volume(v, f)
    relaxed = DS.signed_volume(R.relax_spec(v, f, 10, 0.5)[0], f)
    smoothed = DS.signed_volume(smooth_spec.smooth_spec(v, f, 10, lam=0.5, mu=0.0), f)
    print('volume {!r}: relaxed {!r}, Laplacian {!r}'.format(before, relaxed, smoothed))
    assert abs(relaxed - before) < abs(smoothed - before)


def test_no_pass_and_no_face_give_the_mesh_back():
    v, f = mesh('sphere')
    for hv, hf, iters in ((v, f, 0), (v, np.zeros((0, 3), np.int64), 3), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 3)):
        out_v, out_f, info = R.relax_spec(hv, hf, iters, 0.5)
        assert bits(out_v) == bits(hv) and info['moved'] == 0 and info['states'] == [0, 0, 0, 0]


# ---- loop --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['needles', 'torus16x8', 'patch', 'welded'])
def test_the_loop_equals_the_chain_written_by_hand(name):
    v, f = mesh(name)
    L = subdivide_spec.median_edge(v, f)
    low, high = (4.0 * L) / 5.0, (4.0 * L) / 3.0
    V, F, steps = v, f, []
    for _ in range(3):
        V, F, _, split = subdivide_spec.subdivide_spec(V, F, max_edge=high)
        V, F, collapse = R.collapse_spec(V, F, low, high)
        V, F, flips = flip_spec.flip_spec(V, F, 10.0)
        V, F, relax = R.relax_spec(V, F, 1, 0.5)
        steps.append({'splits': split['splits'], 'collapses': collapse['collapses'], 'flips': flips['flips'], 'moved': relax['moved']})
    out_v, out_f, info = R.remesh_spec(v, f, factor=1.0, iters=3)
    assert bits(out_v) == bits(V) and bits(out_f) == bits(F) and info['iterations'] == steps
    assert info['target_edge'] == L and info['low'] == low and info['high'] == high and not info['limited']
    same = R.remesh_spec(v, f, target_edge=L, iters=3)
    assert bits(same[0]) == bits(V) and bits(same[1]) == bits(F)
    origin, _, _, colors, _ = R.remesh_rows_spec(v, f, factor=1.0, iters=3, colors=np.arange(v.shape[0] * 3, dtype=np.int64).reshape(-1, 3) % 251)
    assert origin.shape[0] == V.shape[0] == colors.shape[0] and origin.max() < v.shape[0]


@pytest.mark.parametrize('name', ['needles', 'torus16x8'])
def test_the_loop_evens_the_edges_and_removes_small_corners_and_crosses_nothing(name):
    v, f = mesh(name)
    out_v, out_f, info = remeshed(name)
    cv_in, cv_out = R.edge_cv(v, f), R.edge_cv(out_v, out_f)
    small_in, small_out = R.small_corner_share(v, f), R.small_corner_share(out_v, out_f)
    print('{}: edge cv {!r} -> {!r}, corners below 30 degrees {!r} -> {!r}, smallest angle {!r} -> {!r}, faces {} -> {}'.format(
        name, cv_in, cv_out, small_in, small_out, flip_spec.min_angle(v, f), flip_spec.min_angle(out_v, out_f), f.shape[0], out_f.shape[0]))
    assert cv_out < cv_in and small_out < small_in
    assert DS.closed_manifold(out_v, out_f) and DS.euler(out_v, out_f) == DS.euler(v, f)
    assert intersect_spec.intersect_spec(out_v, out_f)[2]['pairs'] == 0
    assert len(info['iterations']) == 5 and sum(step['collapses'] for step in info['iterations']) > 0


def test_the_loop_gives_back_what_it_cannot_work_on_and_reports_the_split_guard():
    v, f = mesh('sphere')
    for hv, hf in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), (v, np.array([[0, 0, 1], [-1, 2, 3]], dtype=np.int64))):
        out_v, out_f, info = R.remesh_spec(hv, hf, factor=1.0)
        assert bits(out_v) == bits(hv) and bits(out_f) == bits(hf) and info['iterations'] == [] and info['target_edge'] == 0.0
    info = R.remesh_spec(v, f, factor=0.5, iters=1, max_faces=1300)[2]
    assert info['limited'] and info['max_faces'] == 1300


# ---- parameters and declarations -----------------------------------------------------------------------------------------------------------------
class Untouchable:
    """Stands for a tensor: any look at it fails the test."""

    def __getattr__(self, name):
        raise AssertionError('the parameters must be checked before the tensors: .{} was read'.format(name))


BAD_COLLAPSE = [dict(min_edge=0.0), dict(min_edge=-1.0), dict(min_edge=float('nan')), dict(min_edge=float('inf')), dict(min_edge=True),
                dict(min_edge='1'), dict(min_edge=None), dict(min_edge=1.0, max_edge=0.5), dict(min_edge=1.0, max_edge=float('inf')),
                dict(min_edge=1.0, max_edge=float('nan')), dict(min_edge=1.0, max_edge=True), dict(min_edge=1.0, max_rounds=0),
                dict(min_edge=1.0, max_rounds=1.5), dict(min_edge=1.0, max_rounds=True), dict(min_edge=1.0, max_rounds=2 ** 31)]
BAD_RELAX = [dict(iters=-1), dict(iters=1001), dict(iters=1.0), dict(iters=True), dict(lam=0.0), dict(lam=1.5), dict(lam=float('nan')),
             dict(lam=-0.5), dict(lam=True), dict(lam='0.5')]
BAD_REMESH = [dict(), dict(target_edge=1.0, factor=1.0), dict(target_edge=0.0), dict(target_edge=-1.0), dict(target_edge=float('inf')),
              dict(target_edge=True), dict(factor=0.0), dict(factor=float('nan')), dict(factor=True), dict(factor=1.0, iters=-1),
              dict(factor=1.0, iters=1001), dict(factor=1.0, iters=2.0), dict(factor=1.0, iters=True), dict(factor=1.0, relax_lam=0.0),
              dict(factor=1.0, relax_lam=1.01), dict(factor=1.0, relax_lam=True), dict(factor=1.0, flip_angle=0.0), dict(factor=1.0, flip_angle=91.0),
              dict(factor=1.0, flip_angle=True), dict(factor=1.0, max_faces=-1), dict(factor=1.0, max_faces=2 ** 32), dict(factor=1.0, max_faces=1.5),
              dict(factor=1.0, max_faces=True)]


@pytest.mark.parametrize('function,kw', [('collapse_short_edges', kw) for kw in BAD_COLLAPSE] + [('relax_tangential', kw) for kw in BAD_RELAX]
                         + [('remesh_isotropic', kw) for kw in BAD_REMESH])
def test_every_parameter_rule_raises_before_any_tensor_is_looked_at(function, kw):
    from ppsurf_amd import remesh
    with pytest.raises(ValueError):
        getattr(remesh, function)(Untouchable(), Untouchable(), **kw)


def test_good_parameters_reach_the_device_guard():
    import torch
    from ppsurf_amd import remesh
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for call in (lambda: remesh.collapse_short_edges(v, f, 1.0, 2.0, 5), lambda: remesh.relax_tangential(v, f, 0, 1.0),
                 lambda: remesh.remesh_isotropic(v, f, factor=np.float32(1.0), iters=np.int64(0), max_faces=0)):
        with pytest.raises(remesh.CpuTensorError, match='no CPU'):
            call()


@pytest.mark.parametrize('argv', [['m.ply', 'o.ply'], ['m.ply', 'o.ply', '--factor', '1', '--target_edge', '1'], ['m.ply', 'o.ply', '--factor', '0'],
                                  ['m.ply', 'o.ply', '--factor', '1', '--iters', '-1'], ['m.ply', 'o.ply', '--factor', '1', '--relax_lam', '2'],
                                  ['m.ply', 'o.ply', '--factor', '1', '--flip_angle', '0'], ['m.ply', 'o.ply', '--factor', '1', '--stage', 'split'],
                                  ['m.ply', 'o.obj', '--factor', '1'], ['m.ply', 'o.ply', '--factor', '1', '--gen_remesh', '1']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import remesh
    with pytest.raises(SystemExit) as e:
        remesh.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_remesh_entries_are_declared_and_every_call_site_lies_where_it_should():
    from ppsurf_amd import _lib, build
    I, I64, P, F64 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    want = {'ppsx_remesh_short_edges': ['pos', 'nv', 'faces', 'nf', 'offsets', 'nbr', 'src', 'ne', 'inc_offsets', 'inc', 'ni', 'regular', 'min2',
                                        'max2', 'prio', 'stream'],
            'ppsx_remesh_relax_pass': ['x', 'nv', 'faces', 'nf', 'offsets', 'nbr', 'ne', 'inc_offsets', 'inc', 'ni', 'regular', 'lam', 'y', 'state',
                                       'stream']}
    counts, reals = ('ne', 'ni', 'nv', 'nf'), ('min2', 'max2', 'lam')
    for name, params in want.items():
        assert _lib.EXT_PARAMS[name] == params, name
        assert _lib.EXT_SIGNATURES[name] == (I, [I64 if p in counts else F64 if p in reals else P for p in params]), name
    assert sorted(n for n in _lib.EXT_PARAMS if n.startswith('ppsx_remesh')) == sorted(want)
    assert not any(n.startswith('pps_remesh') for n in _lib.SIGNATURES)                                  # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_remesh')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'remesh.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {name: 1 for name in want}
    # remesh.py names no other entry: the rows and the rest of a round come through decimate.py, the splits and flips through their modules
    source = open(os.path.join(call_sites.REPO, 'ppsurf_amd', 'remesh.py')).read()
    assert set(re.findall(r'\bppsx_\w+', source)) == set(want) and not re.search(r'call\(\s*[\'"]pps_', source)
    assert 'pps_remesh.hip' in build.SOURCES and 'pps_collapse.h' in build.HEADERS
    kernel_source = open(os.path.join(build.CSRC, 'pps_remesh.hip')).read()
    assert '#include "pps_collapse.h"' in kernel_source and '__shared__' not in kernel_source and 'atomic' not in kernel_source.split('#include')[1]
    assert 'sqrt' not in re.sub(r'//.*', '', kernel_source)
    assert '#include "pps_collapse.h"' in open(os.path.join(build.CSRC, 'pps_decimate.hip')).read()
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and set(want) <= set(_lib._ext_entries)
    # the specification shares no code with the module
    spec_source = open(os.path.join(call_sites.REPO, 'tests', 'remesh_spec.py')).read()
    assert 'ppsurf_amd' not in re.sub(r'""".*?"""', '', spec_source, flags=re.S)
