"""GPU tier of the longest-edge bisection: ppsurf_amd/subdivide.py and the kernels of csrc/pps_subdivide.hip against the
numpy specification tests/subdivide_spec.py, byte for byte and twice; each kernel alone on prefixes of the runs and faces of the stretched
12 x 12 lattice and on hand-made tables between canary rows; the argument rules of the C entries; `python -m ppsurf_amd.subdivide` end to
end; and the flips and the orientation stage on a subdivided mesh."""
import json

import numpy as np
import pytest
import torch

import subdivide_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64, U8, F32, F64 = torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64
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


def same(t, want):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


def hostile(scale=1.0):
    """(verts f32, faces, max2, the evaluation at half the median edge) of the stretched, bent and shifted 12 x 12 lattice; computed once."""
    if scale not in _cache:
        verts, faces = S.hostile(scale)
        max_edge = 0.5 * S.median_edge(verts, faces)
        _cache[scale] = (verts, faces, max_edge * max_edge, S.evaluate(verts, faces, max_edge * max_edge))
    return _cache[scale]


def want_of(verts, faces, kw):
    key = (verts.tobytes(), faces.tobytes(), tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = S.subdivide_spec(verts, faces, **kw)
    return _cache[key]


def check_run(subdivide, verts, faces, what, **kw):
    want_v, want_f, want_ends, want_info = want_of(verts, faces, kw)
    v, f = dev(verts), dev(faces)
    for _ in range(2):
        out_v, out_f, ends, info = subdivide.split_long_edges(v, f, return_ends=True, **kw)
        assert info == want_info, (what, info, want_info)
        assert out_v.dtype == F32 and out_f.dtype == I64 and ends.dtype == I64 and ends.shape == (want_info['splits'], 2), what
        assert same(out_v, want_v) and same(out_f, want_f) and same(ends, want_ends), what
        assert (out_f is f) == (out_v is v) == (want_info['splits'] == 0), what
        assert json.loads(json.dumps(info)) == info and type(info['converged']) is bool and type(info['limited']) is bool
    assert same(v, verts) and same(f, faces), what                                        # the inputs are not written
    three = subdivide.split_long_edges(v, f, **kw)
    assert len(three) == 3 and same(three[1], want_f) and three[2] == want_info
    return want_info


@pytest.mark.parametrize('name', S.CASES)
def test_split_long_edges_matches_the_spec_bytewise(name):
    from ppsurf_amd import subdivide
    verts, faces = S.case(name)
    for factor in S.FACTORS:
        info = check_run(subdivide, verts, faces, (name, factor), factor=factor)
        # the same bytes through the bound that the run reported
        if info['faces_valid']:
            want = want_of(verts, faces, dict(factor=factor))
            out_v, out_f, ends, by_edge = subdivide.split_long_edges(dev(verts), dev(faces), max_edge=info['max_edge'], return_ends=True)
            assert by_edge == info and same(out_v, want[0]) and same(out_f, want[1]) and same(ends, want[2]), (name, factor)


def test_hand_made_meshes_bounds_and_hostile_coordinates_match_the_spec():
    from ppsurf_amd import subdivide
    done = {}
    for name, verts, faces, max_edge, max_rounds in S.hand_cases():
        done[name] = check_run(subdivide, verts, faces, name, max_edge=max_edge, max_rounds=max_rounds)
    assert done['slot 0']['added'] == done['two faces']['added'] == done['three on an edge']['added'] == done['two copies']['added'] == [1]
    assert done['waits']['added'][:2] == [1, 2] and done['neighbouring floats']['rounds'] == 4 and done['rows out of play']['faces_valid'] == 1
    verts, faces = S.case('sphere decimated')
    whole = check_run(subdivide, verts, faces, 'whole', factor=0.5)
    one = check_run(subdivide, verts, faces, 'one round', max_edge=whole['max_edge'], max_rounds=1)
    assert one['rounds'] == 1 and not one['converged'] and one['candidates_out'] > 0
    two = check_run(subdivide, verts, faces, 'two rounds', max_edge=whole['max_edge'], max_rounds=2)
    third = check_run(subdivide, verts, faces, 'three rounds', max_edge=whole['max_edge'], max_rounds=3)
    short = check_run(subdivide, verts, faces, 'one face short', max_edge=whole['max_edge'], max_faces=third['faces_out'] - 1)
    assert short['limited'] and short['rounds'] == 2 and short['faces_out'] == two['faces_out']
    assert not check_run(subdivide, verts, faces, 'enough', max_edge=whole['max_edge'], max_faces=third['faces_out'], max_rounds=3)['limited']
    assert check_run(subdivide, verts, faces, 'no room', factor=0.5, max_faces=0)['rounds'] == 0
    for scale in (1.0, 1e38):
        verts, faces = hostile(scale)[:2]
        info = check_run(subdivide, verts, faces, ('hostile', scale), factor=0.5)
        assert info['splits'] > 0 and info['converged'] and np.isfinite(want_of(verts, faces, dict(factor=0.5))[0]).all()
    # a float64 / non-contiguous mesh is taken like its float32 contiguous copy
    verts, faces = hostile()[:2]
    out_v, out_f, info = subdivide.split_long_edges(dev(verts.astype(np.float64)), dev(faces), factor=0.5)
    assert same(out_v, want_of(verts, faces, dict(factor=0.5))[0]) and same(out_f, want_of(verts, faces, dict(factor=0.5))[1])


@pytest.mark.parametrize('scale', [1.0, 1e38])
@pytest.mark.parametrize('n', [255, 256, 257, None])
def test_each_kernel_alone_on_a_prefix(n, scale):
    from ppsurf_amd import _lib
    verts, faces, max2, ev = hostile(scale)
    nv, nf, ne = verts.shape[0], faces.shape[0], ev['keys'].shape[0]
    assert (nf, ne) == (288, 456) and 16 <= int(ev['win'].sum()) < int(ev['cand'].sum()) and np.isfinite(ev['len2']).all()
    me, mf = (ne, nf) if n is None else (n, n)
    dv = dev(verts)
    # the edges: a prefix of the keys with the sentinel run at its end and five keys that name no edge of these vertices
    keys = np.concatenate([ev['keys'][:me], [S.SENTINEL]])
    live = np.nonzero(ev['cand'][:me])[0]
    a, b = keys[live[:5]] >> 32, keys[live[:5]] & 0xFFFFFFFF
    keys[live[:5]] = [(a[0] << 32) | nv, (b[1] << 32) | a[1], -keys[live[2]], (a[3] << 32) | a[3], (a[4] << 32) | (2 ** 32 - 1)]
    want_len2, want_prio = S.edge_priorities(keys, verts, max2)
    assert (want_prio[live[:5]] == S.NONE).all() and want_prio[-1] == S.NONE and (want_prio[live[5:]] == ev['prio'][live[5:]]).all()
    lbuf, dlen2 = guarded(me + 1, F64, -7.0)
    pbuf, dprio = guarded(me + 1, I64, -7)
    for _ in range(2):
        _lib.call('ppsx_subdivide_edges', dev(keys), me + 1, dv, nv, max2, dlen2, dprio)
        assert same(dlen2, want_len2) and same(dprio, bits(want_prio)) and untouched(lbuf, -7.0) and untouched(pbuf, -7)
    assert np.isfinite(want_len2).all()
    _lib.call('ppsx_subdivide_edges', dev(keys), me + 1, dv, nv, float('inf'), dlen2, dprio)          # the median's call: lengths alone
    assert same(dlen2, want_len2) and bool((dprio == NONE).all())
    # the votes: a prefix of the faces against the whole priority table, with run entries that point nowhere
    run_of = ev['run_of'][:mf].copy()
    run_of[0, 0], run_of[1, 1], run_of[2, 2], run_of[mf - 1, 0] = -1, ne, 2 ** 40, -2 ** 40
    want_choice, want_votes = S.choices(run_of, ev['prio'])
    dprio, drun = dev(bits(ev['prio'])), dev(run_of.reshape(-1))
    cbuf, dchoice = guarded(mf, I32, -7)
    vbuf, dvotes = guarded(ne, I32, 0)
    vbuf[0], vbuf[-1] = -7, -7
    for _ in range(2):
        dvotes.zero_()
        _lib.call('ppsx_subdivide_votes', drun, mf, dprio, ne, dchoice, dvotes)
        assert same(dchoice, want_choice.astype(np.int32)) and same(dvotes, want_votes.astype(np.int32)) and untouched(cbuf, -7) and untouched(vbuf, -7)
    # the winners: a prefix of the runs, one winner a vote short and one with a vote too many
    votes, owners = ev['votes'][:me].copy(), ev['owners'][:me]
    won = np.nonzero(ev['win'][:me])[0]
    votes[won[0]] -= 1
    votes[won[1]] += 1
    want_win = ((ev['prio'][:me] != S.NONE) & (votes == owners)).astype(np.uint8)
    assert want_win[won[0]] == want_win[won[1]] == 0 and want_win.sum() == won.shape[0] - 2
    wbuf, dwin = guarded(me, U8, 7)
    for _ in range(2):
        _lib.call('ppsx_subdivide_winners', dprio, dev(votes.astype(np.int32)), dev(owners), me, dwin)
        assert same(dwin, want_win) and untouched(wbuf, 7)
    # the hits: a prefix of the faces against the whole flag table; choices outside 0..2 and runs outside the table are no hits
    choice, run_of = ev['choice'][:mf].copy(), ev['run_of'][:mf].copy()
    hit = np.nonzero(ev['hit'][:mf])[0]
    choice[hit[0]], choice[hit[1]] = 3, -2
    run_of[hit[2], choice[hit[2]]], run_of[hit[3], choice[hit[3]]] = ne, -1
    want_hit = S.hits_of(run_of, choice, ev['win']).astype(np.uint8)
    assert want_hit.sum() == hit.shape[0] - 4
    hbuf, dhit = guarded(mf, U8, 7)
    dwin_all, dchoice, drun = dev(ev['win'].astype(np.uint8)), dev(choice.astype(np.int32)), dev(run_of.reshape(-1))
    for _ in range(2):
        _lib.call('ppsx_subdivide_hits', drun, dchoice, mf, dwin_all, ne, dhit)
        assert same(dhit, want_hit) and untouched(hbuf, 7)
    # the emit: the whole runs and a prefix of the faces, from the tables of the specification
    part = dict(ev, run_of=ev['run_of'][:mf], choice=ev['choice'][:mf], hit=ev['hit'][:mf])
    want_v, want_f, want_ends = S.emit(verts, faces[:mf], part)
    win, hit = ev['win'].astype(np.int64), part['hit'].astype(np.int64)
    nw, nh = int(win.sum()), int(hit.sum())
    nbuf, dnew = guarded(nw, F32, -7.0, 3)
    ebuf, dends = guarded(nw, I64, -7, 2)
    obuf, dout = guarded(mf + nh, I64, -7, 3)
    df = dev(faces[:mf])
    for _ in range(2):
        _lib.call('ppsx_subdivide_emit', dv, nv, dev(ev['keys']), dwin_all, dev(np.cumsum(win) - win), ne, nw, df, mf, dev(part['run_of'].reshape(-1)),
                  dev(part['choice'].astype(np.int32)), dev(hit.astype(np.uint8)), dev(np.cumsum(hit) - hit), nh, dnew, dends, dout)
        assert same(dnew, want_v[nv:]) and same(dends, want_ends) and same(dout, want_f)
        assert untouched(nbuf, -7.0) and untouched(ebuf, -7) and untouched(obuf, -7)
    assert same(df, faces[:mf]) and np.isfinite(want_v).all() and want_f.shape[0] == mf + nh


def test_votes_and_emit_alone_on_hand_made_tables():
    from ppsurf_amd import _lib
    hi = lambda w: w << 32
    # runs 0, 1 and 2 tie in the high word: the low word decides; run 3 is no candidate; run 4 has the smallest high word
    prio = np.array([hi(5) | 9, hi(5) | 8, hi(5) | 7, -1, hi(3) | 1], dtype=np.int64)
    run_of = np.array([[0, 1, 2], [3, 3, 3], [3, 0, 1], [4, 0, 1], [0, 0, 3], [7, -1, 0], [2, 2, 2], [5, 3, -9]], dtype=np.int64)
    cbuf, choice = guarded(8, I32, -7)
    votes = torch.zeros(5, dtype=I32, device=DEV)
    _lib.call('ppsx_subdivide_votes', dev(run_of.reshape(-1)), 8, dev(prio), 5, choice, votes)
    assert choice.cpu().tolist() == [2, -1, 2, 0, 0, 2, 0, -1] and votes.cpu().tolist() == [2, 1, 2, 0, 1] and untouched(cbuf, -7)
    want = S.choices(run_of, prio.view(np.uint64))
    assert want[0].tolist() == choice.cpu().tolist() and want[1].tolist() == votes.cpu().tolist()
    owners = np.array([2, 2, 2, 1, 1], dtype=np.int64)
    win = torch.full((5,), 7, dtype=U8, device=DEV)
    _lib.call('ppsx_subdivide_winners', dev(prio), votes, dev(owners), 5, win)
    assert win.cpu().tolist() == [1, 0, 1, 0, 1]
    votes[3] = 1                                                      # as many votes as owners, and still no candidate
    _lib.call('ppsx_subdivide_winners', dev(prio), votes, dev(owners), 5, win)
    assert win.cpu().tolist() == [1, 0, 1, 0, 1]
    # the emit: winners at the first and the last run and face, a winner whose key cannot be read, and flagged faces that must be copied
    nv, nf = 50, 300
    verts = np.random.default_rng(4).standard_normal((nv, 3)).astype(np.float32)
    faces = np.arange(3 * nf, dtype=np.int64).reshape(nf, 3) % 50
    keys = np.array([(0 << 32) | 1, (2 << 32) | 3, (4 << 32) | 50, (4 << 32) | 5, (6 << 32) | 7], dtype=np.int64)
    win = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    vslot = np.array([0, 1, 1, 2, 2], dtype=np.int64)
    run_of = np.full((nf, 3), 1, dtype=np.int64)
    choice, hit, fslot = np.full(nf, -1, dtype=np.int32), np.zeros(nf, dtype=np.uint8), np.zeros(nf, dtype=np.int64)
    run_of[0], choice[0], hit[0], fslot[0] = (0, 1, 1), 0, 1, 0                             # the first face, the first run
    run_of[nf - 1], choice[nf - 1], hit[nf - 1], fslot[nf - 1] = (1, 1, 4), 2, 1, 6         # the last face, the last run, the last new row
    run_of[4], choice[4], hit[4], fslot[4] = (1, 2, 1), 1, 1, 1                             # the run whose key names no vertex pair: the row m all the same
    choice[5], hit[5], fslot[5] = 3, 1, 2                                                  # a slot that is none
    run_of[6], choice[6], hit[6], fslot[6] = (5, 1, 1), 0, 1, 3                             # a run outside the table
    run_of[7], choice[7], hit[7], fslot[7] = (1, 1, 1), 1, 1, 4                             # a run that did not win
    run_of[8], choice[8], hit[8], fslot[8] = (0, 1, 1), 0, 0, 5                             # a winner's face without the flag
    run_of[9], choice[9], hit[9], fslot[9] = (4, 1, 1), 0, 1, 7                             # a row outside the new faces
    run_of[10], choice[10], hit[10], fslot[10] = (4, 1, 1), 0, 1, -1
    want_f = np.concatenate([faces, np.full((7, 3), -7, dtype=np.int64)])
    want_f[0], want_f[nf] = (faces[0, 0], nv, faces[0, 2]), (nv, faces[0, 1], faces[0, 2])
    want_f[nf - 1], want_f[nf + 6] = (nv + 2, faces[nf - 1, 1], faces[nf - 1, 2]), (faces[nf - 1, 0], faces[nf - 1, 1], nv + 2)
    want_f[4], want_f[nf + 1] = (faces[4, 0], faces[4, 1], nv + 1), (faces[4, 0], nv + 1, faces[4, 2])
    want_v = np.full((3, 3), -7.0, dtype=np.float32)
    want_v[0], want_v[2] = S.midpoints(verts, [0], [1])[0], S.midpoints(verts, [6], [7])[0]
    want_e = np.array([[0, 1], [-7, -7], [6, 7]], dtype=np.int64)
    nbuf, dnew = guarded(3, F32, -7.0, 3)
    ebuf, dends = guarded(3, I64, -7, 2)
    obuf, dout = guarded(nf + 7, I64, -7, 3)
    _lib.call('ppsx_subdivide_emit', dev(verts), nv, dev(keys), dev(win), dev(vslot), 5, 3, dev(faces), nf, dev(run_of.reshape(-1)), dev(choice), dev(hit),
              dev(fslot), 7, dnew, dends, dout)
    assert same(dnew, want_v) and same(dends, want_e) and same(dout, want_f)
    assert untouched(nbuf, -7.0) and untouched(ebuf, -7) and untouched(obuf, -7)


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, subdivide
    hv, hf, max2, ev = hostile()
    nv, nf, ne = hv.shape[0], hf.shape[0], ev['keys'].shape[0]
    nw, nh = int(ev['win'].sum()), int(ev['hit'].sum())
    verts, faces, keys, owners, run_of = dev(hv), dev(hf), dev(ev['keys']), dev(ev['owners']), dev(ev['run_of'].reshape(-1))
    len2, prio = torch.full((ne,), -7.0, dtype=F64, device=DEV), torch.full((ne,), -7, dtype=I64, device=DEV)
    choice, votes = torch.full((nf,), -7, dtype=I32, device=DEV), torch.zeros(ne, dtype=I32, device=DEV)
    win, hit = torch.full((ne,), 7, dtype=U8, device=DEV), torch.full((nf,), 7, dtype=U8, device=DEV)
    new_v, ends = torch.full((nw, 3), -7.0, dtype=F32, device=DEV), torch.full((nw, 2), -7, dtype=I64, device=DEV)
    out = torch.full((nf + nh, 3), -7, dtype=I64, device=DEV)
    vslot, fslot = dev(np.cumsum(ev['win']) - ev['win']), dev(np.cumsum(ev['hit']) - ev['hit'])
    big, huge = 2 ** 31, 2 ** 32

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def edges(keys=keys, ne=ne, verts=verts, nv=nv, max2=max2, len2=len2, prio=prio):
        return run('ppsx_subdivide_edges', keys, ne, verts, nv, max2, len2, prio)

    def vote(run_of=run_of, nf=nf, prio=prio, ne=ne, choice=choice, votes=votes):
        return run('ppsx_subdivide_votes', run_of, nf, prio, ne, choice, votes)

    def winners(prio=prio, votes=votes, owners=owners, ne=ne, win=win):
        return run('ppsx_subdivide_winners', prio, votes, owners, ne, win)

    def hits(run_of=run_of, choice=choice, nf=nf, win=win, ne=ne, hit=hit):
        return run('ppsx_subdivide_hits', run_of, choice, nf, win, ne, hit)

    def emit(verts=verts, nv=nv, keys=keys, win=win, vslot=vslot, ne=ne, nw=nw, faces=faces, nf=nf, run_of=run_of, choice=choice, hit=hit, fslot=fslot,
             nh=nh, new_v=new_v, ends=ends, out=out):
        return run('ppsx_subdivide_emit', verts, nv, keys, win, vslot, ne, nw, faces, nf, run_of, choice, hit, fslot, nh, new_v, ends, out)

    def clean():
        return (bool((len2 == -7.0).all()) and bool((prio == -7).all()) and bool((choice == -7).all()) and bool((votes == 0).all()) and bool((win == 7).all())
                and bool((hit == 7).all()) and bool((new_v == -7.0).all()) and bool((ends == -7).all()) and bool((out == -7).all()) and same(faces, hf))

    for kw in (dict(ne=-1), dict(nv=-1), dict(ne=huge), dict(nv=big), dict(max2=float('nan')), dict(keys=None), dict(verts=None), dict(len2=None),
               dict(prio=None)):
        assert edges(**kw) == 1, kw
        assert clean(), kw
    assert edges(ne=0) == 0 and edges(ne=0, keys=None, verts=None, len2=None, prio=None) == 0 and clean()
    for kw in (dict(nf=-1), dict(ne=-1), dict(nf=big), dict(ne=huge), dict(run_of=None), dict(prio=None), dict(choice=None), dict(votes=None)):
        assert vote(**kw) == 1, kw
        assert clean(), kw
    assert vote(nf=0) == 0 and vote(nf=0, run_of=None, prio=None, choice=None, votes=None) == 0 and clean()
    for kw in (dict(ne=-1), dict(ne=huge), dict(prio=None), dict(votes=None), dict(owners=None), dict(win=None)):
        assert winners(**kw) == 1, kw
        assert clean(), kw
    assert winners(ne=0) == 0 and winners(ne=0, prio=None, votes=None, owners=None, win=None) == 0 and clean()
    for kw in (dict(nf=-1), dict(ne=-1), dict(nf=big), dict(ne=huge), dict(run_of=None), dict(choice=None), dict(win=None), dict(hit=None)):
        assert hits(**kw) == 1, kw
        assert clean(), kw
    assert hits(nf=0) == 0 and hits(nf=0, run_of=None, choice=None, win=None, hit=None) == 0 and clean()
    for kw in (dict(nv=-1), dict(ne=-1), dict(nw=-1), dict(nf=-1), dict(nh=-1), dict(nv=big), dict(ne=huge), dict(nf=big), dict(nw=ne + 1), dict(nh=nf + 1),
               dict(nv=big - 1), dict(out=faces), dict(verts=None), dict(keys=None), dict(win=None), dict(vslot=None), dict(faces=None), dict(run_of=None),
               dict(choice=None), dict(hit=None), dict(fslot=None), dict(new_v=None), dict(ends=None), dict(out=None)):
        assert emit(**kw) == 1, kw
        assert clean(), kw
    assert emit(ne=0, nw=0, nf=0, nh=0) == 0 and clean()
    assert emit(ne=0, nw=0, nf=0, nh=0, verts=None, keys=None, win=None, vslot=None, faces=None, run_of=None, choice=None, hit=None, fslot=None, new_v=None,
                ends=None, out=None) == 0
    with pytest.raises(_lib.PpsError, match='ppsx_subdivide_winners failed with status 1'):
        _lib.call('ppsx_subdivide_winners', prio, votes, owners, -1, win)
    # the good calls after the refused ones
    assert edges() == 0 and vote() == 0 and winners() == 0 and hits() == 0 and emit() == 0
    assert same(len2, ev['len2']) and same(prio, bits(ev['prio'])) and same(choice, ev['choice'].astype(np.int32)) and same(votes, ev['votes'].astype(np.int32))
    assert same(win, ev['win'].astype(np.uint8)) and same(hit, ev['hit'].astype(np.uint8))
    want_v, want_f, want_e = S.emit(hv, hf, ev)
    assert same(new_v, want_v[nv:]) and same(ends, want_e) and same(out, want_f)
    # the Python layer
    with pytest.raises(ValueError, match='non-finite'):
        subdivide.split_long_edges(torch.cat([verts[:5], torch.full((1, 3), float('nan'), device=DEV)]), faces[:1], factor=1.0)
    with pytest.raises(ValueError, match='max_edge'):
        subdivide.split_long_edges(verts.cpu(), faces, max_edge=0)        # the parameter comes first
    with pytest.raises(subdivide.CpuTensorError, match='no CPU'):
        subdivide.split_long_edges(verts.cpu(), faces, factor=1.0)
    with pytest.raises(subdivide.CpuTensorError, match='no CPU'):
        subdivide.split_long_edges(verts, faces.cpu(), 1.0)


@pytest.mark.parametrize('double', [False, True])
def test_the_command_subdivides_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import meshio, subdivide
    verts, faces = S.base('cube decimated')
    faces = np.concatenate([faces[:30], [[0, 0, 1]], faces[30:]])        # a face with a repeated index (a PLY holds no index out of range)
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) + offset[None]
    nv = verts.shape[0]
    rgb = np.random.default_rng(5).integers(0, 256, size=(nv, 3)).astype(np.uint8)
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    stored, stored_f = meshio.read_ply_mesh(src, dtype=np.float64)
    assert np.array_equal(stored_f, faces)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    for extra, kw in ((['--factor', '0.5'], dict(factor=0.5)), (['--max_edge', '1.5', '--max_rounds', '3', '--max_faces', '5000'],
                                                                 dict(max_edge=1.5, max_rounds=3, max_faces=5000))):
        report = subdivide.main([src, dst] + extra)
        assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
        want_v, want_f, want_ends, want_info = S.subdivide_spec(local, faces, **kw)
        assert report == want_info and report['splits'] > 0 and report['faces_valid'] == 192 and report['faces_in'] == 193
        got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
        assert np.array_equal(got_f, want_f) and got_f[30].tolist() == [0, 0, 1]
        assert got_v[:nv].tobytes() == stored.tobytes()                                    # the given vertices: the file's own values
        new = want_v[nv:].astype(np.float64) + centre[None]
        assert got_v[nv:].tobytes() == (new if double else new.astype(np.float32).astype(np.float64)).tobytes()
        got_rgb = meshio.read_ply_vertex_colors(dst)
        assert np.array_equal(got_rgb[:nv], rgb) and np.array_equal(got_rgb, S.interpolate_colors(rgb, want_ends, want_info['added']))
        assert (b'property double x' in open(dst, 'rb').read(300)) == double
    # nothing to split: the file is written as read
    report = subdivide.main([src, dst, '--max_edge', '100'])
    capsys.readouterr()
    assert report['splits'] == 0 and report['converged'] and meshio.read_ply_mesh(dst, dtype=np.float64)[0].tobytes() == stored.tobytes()


def test_flip_and_orient_run_on_the_subdivided_mesh():
    from ppsurf_amd import flip, orient, subdivide
    verts, faces = S.base('cube decimated')
    v, f = dev(verts), dev(faces)
    out_v, out_f, info = subdivide.split_long_edges(v, f, factor=0.5)
    assert info['splits'] > 0 and info['converged'] and out_f.shape[0] == info['faces_out'] > 4 * faces.shape[0]
    flipped = flip.flip_edges(out_v, out_f)
    assert flipped[0] is out_v and flipped[1].shape == out_f.shape and flipped[2]['faces_valid'] == info['faces_out']
    before, after = orient.orient_mesh(v, f, 'outward')[2], orient.orient_mesh(out_v, out_f, 'outward')[2]
    assert after['components'] == after['components_closed'] == before['components'] == before['components_closed'] == 1
    assert after['faces_flipped'] == before['faces_flipped'] == 0 and after['components_non_orientable'] == 0 and after['faces_valid'] == info['faces_out']
