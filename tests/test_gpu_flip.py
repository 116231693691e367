"""GPU tier of the Delaunay edge flips: ppsurf_amd/flip.py and the kernels of csrc/pps_flip.hip against the numpy
specification tests/flip_spec.py, byte for byte and twice; each kernel alone on prefixes of the pairs of the 12 x 12 lattice and on hand-made
tables between canary rows; the argument rules of the C entries; `python -m ppsurf_amd.flip` end to end; and the orientation stage on a
flipped mesh."""
import json

import numpy as np
import pytest
import torch

import decimate_spec
import flip_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
NONE = -1                                                             # 2^64 - 1 as the int64 that holds its bits
_cache = {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def bits(prio):
    """The uint64 priorities as the int64 array a tensor holds."""
    return np.asarray(prio, dtype=np.uint64).view(np.int64)


def guarded(n, dtype, fill, *tail):
    """(buffer [n + 2, ...] filled with `fill`, its rows 1 .. n): an output between two canary rows."""
    buf = torch.full((n + 2,) + tail, fill, dtype=dtype, device=DEV)
    return buf, buf[1:n + 1]


def untouched(buf, fill):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


def hostile():
    """(verts f32, faces, P f64, the evaluation at 30 degrees) of the 12 x 12 lattice stretched, bent and shifted so that no coordinate is a
    short binary fraction and the crease guard has work to do; computed once."""
    if 'hostile' not in _cache:
        verts, faces = S.jittered_lattice(12)
        rng = np.random.default_rng(12)
        verts = (verts.astype(np.float64) * [1.37, 0.73, 1.0] + [0.1, -0.3, 0.0]
                 + np.stack([0 * verts[:, 0], 0 * verts[:, 0], 0.15 * rng.standard_normal(verts.shape[0])], axis=1)).astype(np.float32)
        P = verts.astype(np.float64)
        _cache['hostile'] = (verts, faces, P, S.evaluate(P, faces, verts.shape[0], S.cos2_of(30.0), 1e-6))
    return _cache['hostile']


def check_run(flip, v, f, faces, max_angle, min_gain, max_rounds, what):
    want_f, want_info = S.flip_spec(v.cpu().numpy(), faces, max_angle, min_gain, max_rounds)[1:]
    for _ in range(2):
        out_v, out_f, info = flip.flip_edges(v, f, max_angle, min_gain, max_rounds)
        assert out_v is v and out_f.dtype == I64 and out_f.shape == f.shape and info == want_info, (what, info, want_info)
        assert out_f.cpu().numpy().tobytes() == want_f.tobytes(), what
        assert (out_f is f) == (want_info['flips'] == 0), what
        assert json.loads(json.dumps(info)) == info and type(info['converged']) is bool
    return want_info


@pytest.mark.parametrize('name', S.CASES)
def test_flip_edges_matches_the_spec_bytewise(name):
    from ppsurf_amd import flip
    verts, faces = S.case(name)
    v, f = dev(verts), dev(faces)
    for max_angle in S.ANGLES:
        check_run(flip, v, f, faces, max_angle, 1e-6, 100, (name, max_angle))
    assert f.cpu().numpy().tobytes() == faces.tobytes() and v.cpu().numpy().tobytes() == verts.tobytes()          # the inputs are not written


def test_hand_made_quads_bounds_on_the_rounds_and_hostile_coordinates_match_the_spec():
    from ppsurf_amd import flip
    flips = {}
    for name, verts, faces, max_angle, min_gain in S.hand_cases():
        flips[name] = check_run(flip, dev(verts), dev(faces), faces, max_angle, min_gain, 100, name)['flips']
    assert flips['long diagonal'] == flips['cap'] == flips['crease 16.7 at 30'] == 1 and flips['square'] == flips['two caps'] == flips['crease 90'] == 0
    verts, faces = decimate_spec.tetrahedron()
    assert check_run(flip, dev(verts), dev(faces), faces, 90.0, 0.0, 100, 'tetrahedron')['edges_manifold'] == 6
    verts, faces = S.case('lattice 12')
    v, f = dev(verts), dev(faces)
    whole = check_run(flip, v, f, faces, 10.0, 1e-6, 100, 'lattice 12')
    one = check_run(flip, v, f, faces, 10.0, 1e-6, 1, 'one round')
    assert one['rounds'] == 1 and not one['converged'] and one['candidates_out'] > 0
    assert check_run(flip, v, f, faces, 10.0, 1e-6, whole['rounds'], 'just enough')['converged']
    assert not check_run(flip, v, f, faces, 10.0, 1e-6, whole['rounds'] - 1, 'one short')['converged']
    verts, faces = hostile()[:2]
    for max_angle in S.ANGLES:
        assert check_run(flip, dev(verts), dev(faces), faces, max_angle, 1e-6, 100, ('hostile', max_angle))['flips'] > 0
    # a float64 / non-contiguous mesh is taken like its float32 contiguous copy, and returned as given
    wide = dev(verts.astype(np.float64))
    out_v, out_f, info = flip.flip_edges(wide, dev(faces), 30.0)
    assert out_v is wide and out_f.cpu().numpy().tobytes() == S.flip_spec(verts, faces, 30.0)[1].tobytes()


def pair_tables(n):
    """The first n pairs of the hostile lattice as the device sees them -- fa, fb, ea, eb int32 with the owners of every odd pair swapped --
    and what the specification says of them: prio (int64 bits), quad, vmin (int64 bits) over those n pairs alone."""
    verts, faces, P, ev = hostile()
    keys, _, f, g, k, l = S.edge_table(faces, verts.shape[0])
    assert f.shape[0] == 408 and np.array_equal(f, ev['f']) and (f < g).all()
    n = 408 if n is None else n
    odd = np.arange(n) % 2 == 1
    fa, fb = np.where(odd, g[:n], f[:n]).astype(np.int32), np.where(odd, f[:n], g[:n]).astype(np.int32)
    ea, eb = np.where(odd, l[:n], k[:n]).astype(np.int32), np.where(odd, k[:n], l[:n]).astype(np.int32)
    prio, quad = ev['prio'][:n].copy(), ev['quad'][:n].copy()
    return verts, faces, keys, fa, fb, ea, eb, prio, quad


def vmin_of(prio, quad, nv):
    vmin = np.full(nv, S.NONE, dtype=np.uint64)
    live = prio != S.NONE
    for j in range(4):
        np.minimum.at(vmin, quad[live, j], prio[live])
    return vmin


@pytest.mark.parametrize('n', [255, 256, 257, None])
def test_each_kernel_alone_on_a_prefix_of_the_pairs(n):
    from ppsurf_amd import _lib
    verts, faces, keys, fa, fb, ea, eb, prio, quad = pair_tables(n)
    n, nv, nf = fa.shape[0], verts.shape[0], faces.shape[0]
    live = np.nonzero(prio != S.NONE)[0]
    assert live.shape[0] >= 16 and (live % 2 == 0).any() and (live % 2 == 1).any()
    # seven candidates become pairs that cannot be read through or that name no common edge: each is no candidate, the rest do not notice
    hit = live[:7]
    fa[hit[0]], fb[hit[1]], ea[hit[2]], eb[hit[3]] = -1, nf, 3, -1
    ea[hit[4]] = (ea[hit[4]] + 1) % 3
    fb[hit[5]] = fa[hit[5]]
    fa[hit[6]] = 2 ** 31 - 1
    prio[hit], quad[hit] = S.NONE, 0
    want_vmin = vmin_of(prio, quad, nv)
    pbuf, dprio = guarded(n, I64, -7)
    qbuf, dquad = guarded(n, I32, -7, 4)
    vbuf, dvmin = guarded(nv, I64, NONE)
    vbuf[0], vbuf[-1] = -7, -7
    dfa, dfb, dea, deb, dkeys, dv, df = dev(fa), dev(fb), dev(ea), dev(eb), dev(keys), dev(verts), dev(faces)
    for _ in range(2):
        dvmin.fill_(NONE)
        _lib.call('ppsx_flip_candidates', dv, nv, df, nf, dfa, dfb, dea, deb, n, dkeys, int(keys.shape[0]), S.cos2_of(30.0), 1e-6, dprio, dquad, dvmin)
        assert dprio.cpu().numpy().tobytes() == bits(prio).tobytes() and untouched(pbuf, -7)
        assert dquad.cpu().numpy().tobytes() == quad.astype(np.int32).tobytes() and untouched(qbuf, -7)
        assert dvmin.cpu().numpy().tobytes() == bits(want_vmin).tobytes() and untouched(vbuf, -7)
    # the winners: the flag of every pair from the tables alone
    want_flag = ((prio != S.NONE) & (want_vmin[quad] == prio[:, None]).all(axis=1)).astype(np.uint8)
    assert 0 < want_flag.sum() < (prio != S.NONE).sum()
    fbuf, dflag = guarded(n, U8, 7)
    for _ in range(2):
        _lib.call('ppsx_flip_winners', dprio, dquad, n, dvmin, nv, dflag)
        assert dflag.cpu().numpy().tobytes() == want_flag.tobytes() and untouched(fbuf, 7)
    corners = quad[want_flag == 1].reshape(-1)
    assert np.unique(corners).shape[0] == corners.shape[0] and want_flag[int(np.argmin(prio))] == 1
    # the apply: the flagged pairs rewrite their two rows, in either owner order; every other row stays
    win = np.nonzero(want_flag)[0]
    want_f = faces.copy()
    lo, hi = np.minimum(fa[win], fb[win]), np.maximum(fa[win], fb[win])
    want_f[lo] = quad[win][:, [0, 3, 2]]
    want_f[hi] = quad[win][:, [1, 2, 3]]
    wbuf, work = guarded(nf, I64, -7, 3)
    for _ in range(2):
        work.copy_(df)
        _lib.call('ppsx_flip_apply', dfa, dfb, dquad, dflag, n, nv, work, nf)
        assert work.cpu().numpy().tobytes() == want_f.tobytes() and untouched(wbuf, -7)
    assert int((want_f != faces).any(axis=1).sum()) == 2 * win.shape[0] and df.cpu().numpy().tobytes() == faces.tobytes()


def test_winners_and_apply_alone_on_hand_made_tables():
    from ppsurf_amd import _lib
    nv = 12
    hi = lambda w: w << 32
    # pairs 0 and 1 tie in the high word and share vertex 3: the low word decides; pair 2 is alone; pair 3 loses vertex 9 to a priority that
    # no listed pair holds; pair 4 is no candidate, whatever vmin holds; 5, 6 and 7 have a quad entry out of range; pair 8 wins with high word 0
    prio = np.array([hi(5) | 9, hi(5) | 8, hi(7) | 1, hi(2) | 2, -1, hi(1) | 1, hi(1) | 2, hi(1) | 3, 4], dtype=np.int64)
    quad = np.array([[0, 1, 2, 3], [3, 4, 5, 6], [7, 8, 0, 1], [9, 10, 7, 8], [11, 11, 11, 11], [-1, 10, 11, 9], [10, 12, 11, 9], [10, 11, 9, 2 ** 31 - 1],
                     [10, 11, 4, 5]], dtype=np.int32)
    vmin = np.full(nv, -1, dtype=np.int64)
    vmin[[0, 1, 2]] = hi(5) | 9
    vmin[[3, 4, 5, 6]] = hi(5) | 8
    vmin[[7, 8]] = hi(2) | 2
    vmin[9] = hi(2) | 1
    vmin[10] = 4
    vmin[11] = 4
    vmin[[4, 5]] = 4
    want = [0, 0, 0, 0, 0, 0, 0, 0, 1]
    # with vertices 4 and 5 back at pair 1's priority, pair 1 wins and pair 8 does not; pair 0 loses vertex 3 either way
    fbuf, flag = guarded(9, U8, 7)
    _lib.call('ppsx_flip_winners', dev(prio), dev(quad), 9, dev(vmin), nv, flag)
    assert flag.cpu().numpy().tolist() == want and untouched(fbuf, 7)
    vmin[[4, 5]] = hi(5) | 8
    _lib.call('ppsx_flip_winners', dev(prio), dev(quad), 9, dev(vmin), nv, flag)
    assert flag.cpu().numpy().tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0] and untouched(fbuf, 7)
    vmin[11] = -1                                                     # all ones at every vertex of pair 4, which is no candidate
    _lib.call('ppsx_flip_winners', dev(prio), dev(quad), 9, dev(vmin), nv, flag)
    assert flag.cpu().numpy()[4] == 0
    # the apply: winners at the first and the last face in both orders, and flagged pairs that must write nothing
    nf = 300
    faces = np.arange(3 * nf, dtype=np.int64).reshape(nf, 3) % 50
    fa = np.array([0, nf - 2, 5, 6, -1, 7, nf, 9, 10], dtype=np.int32)
    fb = np.array([nf - 1, 1, 5, 8, 3, nf, 4, 11, 12], dtype=np.int32)
    quads = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [1, 2, 3, 4], [1, 2, 3, 50], [1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4], [-1, 2, 3, 4], [9, 8, 7, 6]],
                     dtype=np.int32)
    flags = np.array([1, 2, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)
    want_f = faces.copy()
    want_f[0], want_f[nf - 1], want_f[1], want_f[nf - 2] = (1, 4, 3), (2, 3, 4), (5, 8, 7), (6, 7, 8)
    wbuf, work = guarded(nf, I64, -7, 3)
    work.copy_(dev(faces))
    _lib.call('ppsx_flip_apply', dev(fa), dev(fb), dev(quads), dev(flags), 9, 50, work, nf)
    assert work.cpu().numpy().tobytes() == want_f.tobytes() and untouched(wbuf, -7)


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, flip
    hv, hf, keys, fa, fb, ea, eb, want_prio, want_quad = pair_tables(None)
    nv, nf, n, ne = hv.shape[0], hf.shape[0], fa.shape[0], keys.shape[0]
    verts, faces, dkeys = dev(hv), dev(hf), dev(keys)
    fa, fb, ea, eb = dev(fa), dev(fb), dev(ea), dev(eb)
    prio, quad = torch.full((n,), -7, dtype=I64, device=DEV), torch.full((n, 4), -7, dtype=I32, device=DEV)
    vmin, flag = torch.full((nv,), NONE, dtype=I64, device=DEV), torch.full((n,), 7, dtype=U8, device=DEV)
    work = faces.clone()
    cos2, big = S.cos2_of(30.0), 2 ** 31

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def candidates(verts=verts, nv=nv, faces=faces, nf=nf, fa=fa, fb=fb, ea=ea, eb=eb, np_=n, keys=dkeys, ne=ne, prio=prio, quad=quad, vmin=vmin):
        return run('ppsx_flip_candidates', verts, nv, faces, nf, fa, fb, ea, eb, np_, keys, ne, cos2, 1e-6, prio, quad, vmin)

    def winners(prio=prio, quad=quad, np_=n, vmin=vmin, nv=nv, flag=flag):
        return run('ppsx_flip_winners', prio, quad, np_, vmin, nv, flag)

    def apply(fa=fa, fb=fb, quad=quad, flag=flag, np_=n, nv=nv, faces=work, nf=nf):
        return run('ppsx_flip_apply', fa, fb, quad, flag, np_, nv, faces, nf)

    def clean():
        return bool((prio == -7).all()) and bool((quad == -7).all()) and bool((vmin == NONE).all()) and bool((flag == 7).all()) and torch.equal(work, faces)

    for kw in (dict(np_=-1), dict(nv=-1), dict(nf=-1), dict(ne=-1), dict(np_=big), dict(nv=big), dict(nf=big), dict(verts=None), dict(faces=None),
               dict(fa=None), dict(fb=None), dict(ea=None), dict(eb=None), dict(keys=None), dict(prio=None), dict(quad=None), dict(vmin=None)):
        assert candidates(**kw) == 1, kw
        assert clean(), kw
    assert candidates(np_=0) == 0 and clean()
    assert candidates(np_=0, verts=None, faces=None, fa=None, fb=None, ea=None, eb=None, keys=None, prio=None, quad=None, vmin=None) == 0
    for kw in (dict(np_=-1), dict(nv=-1), dict(np_=big), dict(nv=big), dict(prio=None), dict(quad=None), dict(vmin=None), dict(flag=None)):
        assert winners(**kw) == 1, kw
        assert clean(), kw
    assert winners(np_=0) == 0 and winners(np_=0, prio=None, quad=None, vmin=None, flag=None) == 0 and clean()
    flag.fill_(1)                                                     # every pair flagged: a refused apply still writes nothing
    for kw in (dict(np_=-1), dict(nv=-1), dict(nf=-1), dict(np_=big), dict(nv=big), dict(nf=big), dict(fa=None), dict(fb=None), dict(quad=None),
               dict(flag=None), dict(faces=None)):
        assert apply(**kw) == 1, kw
        assert torch.equal(work, faces), kw
    assert apply(np_=0) == 0 and apply(nf=0) == 0 and apply(np_=0, fa=None, fb=None, quad=None, flag=None, faces=None) == 0 and torch.equal(work, faces)
    flag.fill_(7)
    with pytest.raises(_lib.PpsError, match='ppsx_flip_winners failed with status 1'):
        _lib.call('ppsx_flip_winners', prio, quad, -1, vmin, nv, flag)
    # the good calls after the refused ones
    assert candidates() == 0 and winners() == 0
    assert prio.cpu().numpy().tobytes() == bits(want_prio).tobytes() and quad.cpu().numpy().tobytes() == want_quad.astype(np.int32).tobytes()
    assert vmin.cpu().numpy().tobytes() == bits(vmin_of(want_prio, want_quad, nv)).tobytes()
    assert flag.cpu().numpy().tobytes() == hostile()[3]['win'].astype(np.uint8).tobytes()
    assert apply() == 0 and work.cpu().numpy().tobytes() == S.apply_spec(hf, hostile()[3]).tobytes()
    # the Python layer
    with pytest.raises(ValueError, match='non-finite'):
        flip.flip_edges(torch.cat([verts[:5], torch.full((1, 3), float('nan'), device=DEV)]), faces[:1])
    with pytest.raises(ValueError, match='max_angle'):
        flip.flip_edges(verts.cpu(), faces, max_angle=0)              # the parameter comes first
    with pytest.raises(flip.CpuTensorError, match='no CPU'):
        flip.flip_edges(verts.cpu(), faces)
    with pytest.raises(flip.CpuTensorError, match='no CPU'):
        flip.flip_edges(verts, faces.cpu(), 30.0)


@pytest.mark.parametrize('double', [False, True])
def test_the_command_flips_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import flip, meshio
    verts, faces = S.base('cube decimated')
    faces = np.concatenate([faces[:30], [[0, 0, 1]], faces[30:]])        # a face with a repeated index (a PLY holds no index out of range)
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) + offset[None]
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    stored, stored_f = meshio.read_ply_mesh(src, dtype=np.float64)
    assert np.array_equal(stored_f, faces)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    for extra in ([], ['--max_angle', '30', '--min_gain', '0', '--max_rounds', '3']):
        report = flip.main([src, dst] + extra)
        assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
        params = (30.0, 0.0, 3) if extra else (10.0, 1e-6, 100)
        _, want_f, want_info = S.flip_spec(local, faces, *params)
        assert report == want_info and report['flips'] > 0 and report['faces_valid'] == 192 and report['faces_in'] == 193
        got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
        assert np.array_equal(got_f, want_f) and np.array_equal(got_f, flip.flip_edges(dev(local), dev(faces), *params)[1].cpu().numpy())
        assert got_v.tobytes() == stored.tobytes() and np.array_equal(meshio.read_ply_vertex_colors(dst), rgb)
        assert (b'property double x' in open(dst, 'rb').read(300)) == double


def test_orient_sees_the_same_closed_components_after_the_flips():
    from ppsurf_amd import flip, orient
    verts, faces = S.base('cube decimated')
    v, f = dev(verts), dev(faces)
    out_v, out_f, info = flip.flip_edges(v, f)
    assert info['flips'] > 0 and info['converged'] and out_v is v
    before, after = orient.orient_mesh(v, f, 'outward'), orient.orient_mesh(out_v, out_f, 'outward')
    assert before[2] == after[2] and after[2]['components'] == after[2]['components_closed'] == 1 and after[2]['faces_flipped'] == 0
    assert after[1] is out_f and before[1] is f
