"""GPU tier of the orientation stage: ppsurf_amd/orient.py and the kernels of csrc/pps_orient.hip against the numpy
specification tests/orient_spec.py, byte for byte and twice; the labels against pieces.face_components; each kernel alone on hand-made
tables between canary rows; the argument rules of the C entries; `python -m ppsurf_amd.orient` end to end; and the normals of an oriented
mesh."""
import json

import numpy as np
import pytest
import torch

import orient_spec as S
import pieces_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64, U8, F64 = torch.int32, torch.int64, torch.uint8, torch.float64
_cache = {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def spec(name, mode):
    """(faces out, info) of the specification on a named case, computed once."""
    if (name, mode) not in _cache:
        _cache[(name, mode)] = S.orient_spec(*S.case(name), mode)[1:3]
    return _cache[(name, mode)]


def guarded(n, dtype, fill, *tail):
    """(buffer [n + 2, ...] filled with `fill`, its rows 1 .. n): an output between two canary rows."""
    buf = torch.full((n + 2,) + tail, fill, dtype=dtype, device=DEV)
    return buf, buf[1:n + 1]


def untouched(buf, fill):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


@pytest.mark.parametrize('name', S.CASES)
def test_orient_mesh_and_face_flips_match_the_spec_bytewise(name):
    from ppsurf_amd import orient, pieces
    verts, faces = S.case(name)
    v, f = dev(verts), dev(faces)
    want_label, want_flip, want_bad = S.flips_spec(faces, verts.shape[0])
    sound = want_label >= 0
    sound[sound] = want_bad[want_label[sound]] == 0                  # the faces of orientable components: there the flips are defined
    for _ in range(2):
        label, flip, bad = orient.face_flips(f, verts.shape[0])
        assert label.dtype == I32 and flip.dtype == U8 and bad.dtype == U8 and torch.equal(label, pieces.face_components(f, verts.shape[0]))
        assert label.cpu().numpy().tobytes() == want_label.tobytes() and bad.cpu().numpy().tobytes() == want_bad.tobytes()
        assert flip.cpu().numpy()[sound].tobytes() == want_flip[sound].tobytes() and int(flip[label < 0].sum().item()) == 0
        for mode in S.MODES:
            want_f, want_info = spec(name, mode)
            out_v, out_f, info = orient.orient_mesh(v, f, mode)
            assert out_v is v and out_f.dtype == I64 and out_f.shape == f.shape and info == want_info, (mode, info, want_info)
            assert out_f.cpu().numpy().tobytes() == want_f.tobytes(), mode
            assert (out_f is f) == (want_info['faces_flipped'] == 0), mode
            assert json.loads(json.dumps(info)) == info
    assert f.cpu().numpy().tobytes() == faces.tobytes() and v.cpu().numpy().tobytes() == verts.tobytes()          # the inputs are not written


def fixed_point(fa, fb, sign, word, nf):
    """The host loop of orient._flips on hand-made tables."""
    from ppsurf_amd import _lib
    changed = torch.zeros(1, dtype=I32, device=DEV)
    for rounds in range(1, 100):
        changed.zero_()
        _lib.call('ppsx_orient_hook', fa, fb, sign, int(fa.shape[0]), word, nf, changed)
        assert int(changed.item()) in (0, 1)
        if int(changed.item()) == 0:
            return rounds
        _lib.call('ppsx_orient_compress', word, nf)
    raise AssertionError('no fixed point')


def labelled(faces, nv, pairs=None, ok=None):
    """(device fa, fb, sign as computed by pair_sign between canaries, the words at the fixed point between canaries, bad between
    canaries, rounds) and the specification's (label, flip, bad) for the first `pairs` pairs of the specification's list."""
    from ppsurf_amd import _lib
    nf = faces.shape[0]
    fa, fb, ea, eb, s = (x[:pairs] for x in S.pair_list(faces, nv))
    n = fa.shape[0]
    ok = S.valid_faces(faces, nv) if ok is None else ok
    dfa, dfb, dea, deb = (dev(x.astype(np.int32)) for x in (fa, fb, ea, eb))
    sbuf, sign = guarded(n, U8, 7)
    _lib.call('ppsx_orient_pair_sign', dev(faces), nf, dfa, dfb, dea, deb, n, sign)
    assert sign.cpu().numpy().tobytes() == s.tobytes() and untouched(sbuf, 7)
    wbuf, word = guarded(nf, I64, -7)
    word.copy_(dev(np.where(ok, np.arange(nf) << 1, -1)))
    rounds = fixed_point(dfa, dfb, sign, word, nf)
    bbuf, bad = guarded(nf, U8, 0)
    bbuf[0], bbuf[-1] = 9, 9
    _lib.call('ppsx_orient_check', dfa, dfb, sign, n, word, nf, bad)
    assert untouched(wbuf, -7) and bbuf[0].item() == 9 and bbuf[-1].item() == 9
    return word.cpu().numpy(), bad.cpu().numpy(), rounds, S.flips_of_pairs(ok, fa, fb, s)


@pytest.mark.parametrize('pairs', [255, 256, 257, None])
def test_sign_hook_compress_and_check_alone_on_the_scrambled_torus(pairs):
    verts, faces = S.case('torus')
    word, bad, rounds, (label, flip, want_bad) = labelled(faces, verts.shape[0], pairs)
    assert rounds >= 2 and not want_bad.any() and not bad.any()
    assert word.tobytes() == ((label.astype(np.int64) << 1) | flip).tobytes()
    if pairs is None:
        assert (label == 0).all() and 0 < int(flip.sum()) < 256
    else:
        assert len(set(label.tolist())) > 1                          # a prefix of the pairs leaves several components


@pytest.mark.parametrize('order', ['reversed', 'permuted'])
def test_a_chain_of_1025_faces_needs_rounds_and_long_walks(order):
    verts, faces = S.case('strip ' + order)
    word, bad, rounds, (label, flip, want_bad) = labelled(faces, verts.shape[0])
    assert rounds >= 2 and not bad.any() and (label == 0).all() and np.array_equal(flip, (faces[:, 0] - faces[0, 0]) % 2)          # every other face
    assert word.tobytes() == ((label.astype(np.int64) << 1) | flip).tobytes()


def test_a_non_orientable_component_is_found_by_the_check():
    for name in ('moebius', 'klein'):
        verts, faces = S.case(name)
        word, bad, rounds, (label, flip, want_bad) = labelled(faces, verts.shape[0])
        assert (word >> 1 == 0).all() and bad.tolist() == want_bad.tolist() == [1] + [0] * (faces.shape[0] - 1)


def test_hook_compress_and_check_skip_bad_pairs_and_invalid_faces():
    from ppsurf_amd import _lib
    # nf = 8, face 3 invalid; pairs onto it, out of range on either side, and three good ones with their signs
    wbuf, word = guarded(8, I64, -7)
    start = np.array([0, 2, 4, -1, 8, 10, 12, 14], dtype=np.int64)
    word.copy_(dev(start))
    fa = dev(np.array([0, 2, 2, 4, -1, 6, 3, 8, 2 ** 31 - 1], dtype=np.int32))
    fb = dev(np.array([1, 1, 3, 9, 5, 5, 7, 0, 0], dtype=np.int32))
    sign = dev(np.array([1, 0, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8))
    changed = torch.zeros(1, dtype=I32, device=DEV)
    _lib.call('ppsx_orient_hook', fa, fb, sign, 9, word, 8, changed)
    one = word.cpu().numpy()
    # one round: the parents have only fallen, the flips state true relations, and the skipped faces are as they were
    assert int(changed.item()) == 1 and one[1] == 1 and one[2] in (1, 2 | 0) and one[6] == 11 and one[[0, 3, 4, 5, 7]].tolist() == [0, -1, 8, 10, 14]
    _lib.call('ppsx_orient_compress', word, 8)
    fixed_point(fa, fb, sign, word, 8)
    want = [0, 1, 1, -1, 8, 10, 11, 14]                               # flips 0 1 1 . 0 0 1 0 to the leaders 0 0 0 . 4 5 5 7
    assert word.cpu().numpy().tolist() == want and untouched(wbuf, -7)
    assert fixed_point(fa, fb, sign, word, 8) == 1 and word.cpu().numpy().tolist() == want          # a fixed point writes nothing
    bbuf, bad = guarded(8, U8, 0)
    _lib.call('ppsx_orient_check', fa, fb, sign, 9, word, 8, bad)
    assert not bool(bbuf.any())
    # compress alone: chains with flips, an untouched invalid face, a parent above its slot, where a walk ends as at a root
    word.copy_(dev(np.array([0, 1, 2 | 1, 4 | 1, -1, 14, 10 | 1, 6], dtype=np.int64)))
    _lib.call('ppsx_orient_compress', word, 8)
    assert word.cpu().numpy().tolist() == [0, 1, 0, 1, -1, 10, 11, 1] and untouched(wbuf, -7)
    # the check on a hand-made table: leaders 0 0 0 . 4 4 4 7, one pair of the second component contradicts
    word.copy_(dev(np.array([0, 1, 0, -1, 8, 9, 8, 14], dtype=np.int64)))
    ca, cb = dev(np.array([0, 1, 4, 5, 4, 3, 7, -1, 8], dtype=np.int32)), dev(np.array([1, 2, 5, 6, 6, 0, 3, 0, 1], dtype=np.int32))
    cs = dev(np.array([1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8))          # 4-6 has equal flips and the sign 1
    _lib.call('ppsx_orient_check', ca, cb, cs, 9, word, 8, bad)
    assert bbuf.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    # np = 0: nothing to do
    _lib.call('ppsx_orient_hook', None, None, None, 0, word, 8, changed, on=torch.device(DEV))
    # pair_sign: an entry or a slot out of range gives 0 and is not read through
    faces = dev(np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int64))
    sbuf, out = guarded(6, U8, 7)
    _lib.call('ppsx_orient_pair_sign', faces, 2, dev(np.array([0, 0, 2, -1, 0, 0], dtype=np.int32)), dev(np.array([1, 1, 0, 0, 1, 1], dtype=np.int32)),
              dev(np.array([0, 2, 0, 0, 3, 0], dtype=np.int32)), dev(np.array([0, 1, 0, 0, 0, -1], dtype=np.int32)), 6, out)
    assert out.cpu().numpy().tolist() == [1, 0, 0, 0, 0, 0] and untouched(sbuf, 7)


SIZES = (1, 3, 4, 5, 255, 256, 257, 1025)


def sums_fixture():
    """Components of SIZES faces side by side over seeded non-dyadic vertices: (verts, faces, flip, list, first, count, lead per block, start
    per component, the terms per component)."""
    rng = np.random.default_rng(51)
    verts = (rng.standard_normal((500, 3)) * 1.7 + 0.3).astype(np.float32)
    nf = sum(SIZES)
    faces = np.stack([rng.permutation(500)[:3] for _ in range(nf)]).astype(np.int64)
    flip = (rng.random(nf) < 0.5).astype(np.uint8)
    order = np.arange(nf)
    first, count, lead, start, terms, at = [], [], [], [0], [], 0
    for n in SIZES:
        members = order[at:at + n]
        terms.append(S.volume_terms(verts, faces, members, flip, members[0]))
        for b in range(0, n, S.BLOCK):
            first.append(at + b)
            count.append(min(S.BLOCK, n - b))
            lead.append(members[0])
        start.append(len(first))
        at += n
    return (verts, faces, flip, order.astype(np.int32), np.array(first, dtype=np.int64), np.array(count, dtype=np.int32), np.array(lead, dtype=np.int32),
            np.array(start, dtype=np.int64), terms)


def test_block_sums_and_component_sums_alone_in_the_stated_order():
    from ppsurf_amd import _lib
    verts, faces, flip, order, first, count, lead, start, terms = sums_fixture()
    nb, nc, nf = first.shape[0], len(SIZES), faces.shape[0]
    assert nb == 6 + 2 + 5 and count.tolist() == [1, 3, 4, 5, 255, 256, 256, 1, 256, 256, 256, 256, 1]
    want_blocks = np.concatenate([S.block_sums(t) for t in terms])
    want_vol = np.array([S.ordered_sum(t) for t in terms])
    assert any(S.ordered_sum(t) != np.sum(t) for t in terms)             # the order shows in the last bit
    sbuf, sums = guarded(nb, F64, -7.0)
    vbuf, vol = guarded(nc, F64, -7.0)
    dv, df, dflip = dev(verts), dev(faces), dev(flip)
    for _ in range(2):
        _lib.call('ppsx_orient_block_sums', dv, 500, df, nf, dflip, dev(order), nf, dev(first), dev(count), dev(lead), nb, sums)
        _lib.call('ppsx_orient_comp_sums', sums, nb, dev(start), nc, vol)
        assert sums.cpu().numpy().view(np.int64).tolist() == want_blocks.view(np.int64).tolist() and untouched(sbuf, -7.0)
        assert vol.cpu().numpy().view(np.int64).tolist() == want_vol.view(np.int64).tolist() and untouched(vbuf, -7.0)
    # blocks and entries that cannot be read through count as +0.0
    order2, faces2 = order.copy(), faces.copy()
    order2[[8, 300]] = [-1, nf]
    faces2[20] = [1, 1, 2]
    faces2[21] = [0, 1, 500]
    terms2 = []
    for c, n in enumerate(SIZES):
        at = int(np.sum(SIZES[:c]))
        t = terms[c].copy()
        for gone in (8, 300, 20, 21):
            if at <= gone < at + n:
                t[gone - at] = 0.0
        terms2.append(t)
    first2, count2, lead2 = first.copy(), count.copy(), lead.copy()
    first2[0], count2[1], count2[2], lead2[3], first2[12] = -1, 0, 257, nf, nf
    want2 = np.concatenate([S.block_sums(t) for t in terms2])
    want2[[0, 1, 2, 3, 12]] = 0.0
    _lib.call('ppsx_orient_block_sums', dv, 500, dev(faces2), nf, dflip, dev(order2), nf, dev(first2), dev(count2), dev(lead2), nb, sums)
    assert sums.cpu().numpy().view(np.int64).tolist() == want2.view(np.int64).tolist() and untouched(sbuf, -7.0)
    start2 = np.array([0, 6, 5, 8, 14, 13, 13, 13, 13], dtype=np.int64)          # rows that run backwards or past the end are +0.0
    _lib.call('ppsx_orient_comp_sums', dev(want_blocks), nb, dev(start2), nc, vol)
    got = vol.cpu().numpy()
    six, three = np.float64(0.0), np.float64(0.0)
    for b in range(6):
        six = six + want_blocks[b]
    for b in range(5, 8):
        three = three + want_blocks[b]
    assert got.view(np.int64).tolist() == np.array([six, 0.0, three, 0.0, 0.0, 0.0, 0.0, 0.0]).view(np.int64).tolist() and untouched(vbuf, -7.0)


@pytest.mark.parametrize('nf', [255, 256, 257])
def test_apply_alone(nf):
    from ppsurf_amd import _lib
    rng = np.random.default_rng(nf)
    faces = rng.integers(0, 1000, size=(nf, 3)).astype(np.int64)
    faces[::31] = [[-1, 2, 3]]
    faces[7::31, 2] = 1 << 40
    cid = (np.arange(nf) % 5).astype(np.int32)
    cid[::31] = -1
    cid[11::17] = 4                                                   # nc = 4: out of range
    cid[5::29] = -2
    flip = (rng.random(nf) < 0.5).astype(np.uint8)
    turn = np.array([0, 1, 2, 3], dtype=np.uint8)                     # 3 is no decision: nothing turns
    inside = (cid >= 0) & (cid < 4)
    t = turn[np.where(inside, cid, 0)]
    which = inside & (((t == 1) & (flip == 1)) | ((t == 2) & (flip == 0)))
    want = S.turned(faces, which)
    assert 0 < which.sum() < nf
    obuf, out = guarded(nf, I64, -7, 3)
    for _ in range(2):
        _lib.call('ppsx_orient_apply', dev(faces), nf, dev(cid), dev(flip), dev(turn), 4, out)
        assert out.cpu().numpy().tobytes() == want.tobytes() and untouched(obuf, -7)
    _lib.call('ppsx_orient_apply', dev(faces), nf, dev(cid), dev(flip), None, 0, out)          # no component: a copy
    assert out.cpu().numpy().tobytes() == faces.tobytes() and untouched(obuf, -7)


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, orient, topology
    hv, hf = S.case('torus')
    verts, faces = dev(hv), dev(hf)
    nv, nf = hv.shape[0], hf.shape[0]
    fa, fb, ea, eb, valid = topology.manifold_pair_edges(faces, nv)
    pairs = int(fa.shape[0])
    assert all(x.dtype == I32 and x.shape == (pairs,) for x in (fa, fb, ea, eb)) and valid.dtype == torch.bool and pairs == 3 * nf // 2
    sa, sb, sea, seb, ss = S.pair_list(hf, nv)
    swap = fa > fb                                                    # which owner comes first follows the sort
    got = set(zip(torch.where(swap, fb, fa).tolist(), torch.where(swap, fa, fb).tolist(), torch.where(swap, eb, ea).tolist(),
                  torch.where(swap, ea, eb).tolist()))
    flipped = sa > sb
    assert got == set(zip(np.where(flipped, sb, sa).tolist(), np.where(flipped, sa, sb).tolist(), np.where(flipped, seb, sea).tolist(),
                          np.where(flipped, sea, seb).tolist()))
    pa, pb, pvalid = topology.manifold_pairs(faces, nv)
    assert torch.equal(pa, fa) and torch.equal(pb, fb) and torch.equal(pvalid, valid)
    label, flip, bad_ = orient.face_flips(faces, nv)
    sign = torch.full((pairs,), 7, dtype=U8, device=DEV)
    word0 = torch.arange(nf, dtype=I64, device=DEV) << 1
    word = word0.clone()
    changed = torch.zeros(1, dtype=I32, device=DEV)
    bad = torch.zeros(nf, dtype=U8, device=DEV)
    order = torch.arange(nf, dtype=I32, device=DEV)
    first, count, lead = dev(np.array([0, 256], dtype=np.int64)), dev(np.array([256, 256], dtype=np.int32)), dev(np.array([0, 0], dtype=np.int32))
    sums, vol = torch.full((2,), -7.0, dtype=F64, device=DEV), torch.full((1,), -7.0, dtype=F64, device=DEV)
    start = dev(np.array([0, 2], dtype=np.int64))
    cid, turn = torch.zeros(nf, dtype=I32, device=DEV), dev(np.array([1], dtype=np.uint8))
    out = torch.full((nf, 3), -7, dtype=I64, device=DEV)
    big = 2 ** 31

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def pair_sign(faces=faces, nf=nf, fa=fa, fb=fb, ea=ea, eb=eb, np_=pairs, sign=sign):
        return run('ppsx_orient_pair_sign', faces, nf, fa, fb, ea, eb, np_, sign)

    def hook(fa=fa, fb=fb, sign=sign, np_=pairs, word=word, nf=nf, changed=changed):
        return run('ppsx_orient_hook', fa, fb, sign, np_, word, nf, changed)

    def compress(word=word, nf=nf):
        return run('ppsx_orient_compress', word, nf)

    def check(fa=fa, fb=fb, sign=sign, np_=pairs, word=word, nf=nf, bad=bad):
        return run('ppsx_orient_check', fa, fb, sign, np_, word, nf, bad)

    def block_sums(verts=verts, nv=nv, faces=faces, nf=nf, flip=flip, order=order, nl=nf, first=first, count=count, lead=lead, nb=2, sums=sums):
        return run('ppsx_orient_block_sums', verts, nv, faces, nf, flip, order, nl, first, count, lead, nb, sums)

    def comp_sums(sums=sums, nb=2, start=start, nc=1, vol=vol):
        return run('ppsx_orient_comp_sums', sums, nb, start, nc, vol)

    def apply(faces=faces, nf=nf, cid=cid, flip=flip, turn=turn, nc=1, out=out):
        return run('ppsx_orient_apply', faces, nf, cid, flip, turn, nc, out)

    for kw in (dict(np_=-1), dict(nf=-1), dict(np_=big), dict(nf=big), dict(faces=None), dict(fa=None), dict(fb=None), dict(ea=None), dict(eb=None)):
        assert pair_sign(**kw) == 1, kw
        assert bool((sign == 7).all()), kw
    assert pair_sign(sign=None) == 1 and pair_sign(np_=0) == 0 and pair_sign(np_=0, faces=None, fa=None, fb=None, ea=None, eb=None, sign=None) == 0
    assert bool((sign == 7).all())
    assert pair_sign() == 0 and sign.cpu().numpy().sum() == ss.sum() > 0
    for kw in (dict(np_=-1), dict(nf=-1), dict(np_=big), dict(nf=big), dict(fa=None), dict(fb=None), dict(sign=None), dict(changed=None)):
        assert hook(**kw) == 1, kw
        assert torch.equal(word, word0) and changed.item() == 0, kw
    assert hook(word=None) == 1 and hook(np_=0) == 0 and hook(nf=0) == 0 and hook(np_=0, fa=None, fb=None, sign=None, word=None, changed=None) == 0
    for kw in (dict(nf=-1), dict(nf=big), dict(word=None)):
        assert compress(**kw) == 1, kw
    assert compress(nf=0) == 0 and compress(nf=0, word=None) == 0 and torch.equal(word, word0) and changed.item() == 0
    for kw in (dict(np_=-1), dict(nf=-1), dict(np_=big), dict(nf=big), dict(fa=None), dict(fb=None), dict(sign=None), dict(word=None)):
        assert check(**kw) == 1, kw
    assert check(bad=None) == 1 and check(np_=0) == 0 and check(nf=0) == 0 and check(np_=0, fa=None, fb=None, sign=None, word=None, bad=None) == 0
    assert not bool(bad.any())
    for kw in (dict(nb=-1), dict(nl=-1), dict(nv=-1), dict(nf=-1), dict(nb=big), dict(nl=big), dict(nv=big), dict(nf=big), dict(verts=None),
               dict(faces=None), dict(flip=None), dict(order=None), dict(first=None), dict(count=None), dict(lead=None)):
        assert block_sums(**kw) == 1, kw
        assert bool((sums == -7).all()), kw
    assert block_sums(sums=None) == 1 and block_sums(nb=0) == 0 and bool((sums == -7).all())
    assert block_sums(nb=0, verts=None, faces=None, flip=None, order=None, first=None, count=None, lead=None, sums=None) == 0
    for kw in (dict(nc=-1), dict(nb=-1), dict(nc=big), dict(nb=big), dict(sums=None), dict(start=None)):
        assert comp_sums(**kw) == 1, kw
        assert vol.item() == -7, kw
    assert comp_sums(vol=None) == 1 and comp_sums(nc=0) == 0 and comp_sums(nc=0, sums=None, start=None, vol=None) == 0 and vol.item() == -7
    for kw in (dict(nf=-1), dict(nc=-1), dict(nf=big), dict(nc=big), dict(faces=None), dict(cid=None), dict(flip=None), dict(turn=None), dict(faces=out)):
        assert apply(**kw) == 1, kw
        assert bool((out == -7).all()), kw
    assert apply(out=None) == 1 and apply(nf=0) == 0 and apply(nf=0, faces=None, cid=None, flip=None, turn=None, out=None) == 0 and bool((out == -7).all())
    with pytest.raises(_lib.PpsError, match='ppsx_orient_compress failed with status 1'):
        _lib.call('ppsx_orient_compress', word, -1)
    # the good calls after the refused ones
    assert fixed_point(fa, fb, sign, word, nf) >= 2 and check() == 0 and not bool(bad.any())
    assert torch.equal((word >> 1).to(I32), label) and torch.equal((word & 1).to(U8), flip) and not bool(bad_.any())
    assert block_sums() == 0 and comp_sums() == 0          # 256 faces: the second block lies past the list and adds +0.0
    want = S.ordered_sum(S.volume_terms(hv, hf, np.arange(nf), flip.cpu().numpy(), 0))
    assert vol.cpu().numpy().view(np.int64).tolist() == [np.float64(want).view(np.int64)] and want != 0
    assert apply(turn=dev(np.array([1 if want > 0 else 2], dtype=np.uint8))) == 0          # the outward decision
    assert out.cpu().numpy().tobytes() == S.closed_mesh('torus')[1].tobytes()
    # the Python layer
    for fn in (lambda v: orient.orient_mesh(v, faces[:1]),):
        with pytest.raises(ValueError, match='non-finite'):
            fn(torch.cat([verts[:5], torch.full((1, 3), float('nan'), device=DEV)]))
    with pytest.raises(ValueError, match='mode'):
        orient.orient_mesh(verts.cpu(), faces, 'sideways')            # the parameter comes first
    with pytest.raises(orient.CpuTensorError, match='no CPU'):
        orient.orient_mesh(verts.cpu(), faces)
    with pytest.raises(orient.CpuTensorError, match='no CPU'):
        orient.orient_mesh(verts, faces.cpu(), 'majority')
    with pytest.raises(orient.CpuTensorError, match='no CPU'):
        orient.face_flips(faces.cpu(), nv)
    with pytest.raises(ValueError, match='nv'):
        orient.face_flips(faces, -1)


@pytest.mark.parametrize('double', [False, True])
def test_the_command_orients_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import meshio, orient
    verts, faces = S.case('scene')
    faces = np.concatenate([faces[:301], [[0, 0, 1]], faces[301:]])      # a face with a repeated index (a PLY holds no index out of range)
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) + offset[None]
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    stored, stored_f = meshio.read_ply_mesh(src, dtype=np.float64)
    assert np.array_equal(stored_f, faces)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    for mode in ('outward', 'inward'):
        report = orient.main([src, dst, '--mode', mode])
        assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
        _, want_f, want_info, _ = S.orient_spec(local, faces, mode)
        assert report == want_info and report['components'] == report['components_closed'] == 6 and report['faces_valid'] == 1260
        out_v, out_f, info = orient.orient_mesh(dev(local), dev(faces), mode)
        got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
        assert np.array_equal(got_f, want_f) and np.array_equal(got_f, out_f.cpu().numpy()) and info == report
        assert got_v.tobytes() == stored.tobytes() and np.array_equal(meshio.read_ply_vertex_colors(dst), rgb)
        assert (b'property double x' in open(dst, 'rb').read(300)) == double
    keep = np.ones(1261, dtype=bool)
    keep[301] = False
    assert S.orient_spec(local, faces, 'outward')[1][keep].tobytes() == pieces_spec.scene()[1].tobytes()
    assert orient.main([src, dst])['mode'] == 'outward'


def test_the_normals_of_an_oriented_sphere_point_outward():
    from ppsurf_amd import normals, orient
    verts, faces = S.case('sphere')
    v, f = dev(verts), dev(faces)
    centred = v - v.mean(dim=0, keepdim=True)
    before = (normals.vertex_normals(v, f)[0] * centred).sum(dim=1)
    assert int((before <= 0).sum().item()) > 0                        # scrambled: the normals fight each other
    out_v, out_f, info = orient.orient_mesh(v, f, 'outward')
    after = (normals.vertex_normals(out_v, out_f)[0] * centred).sum(dim=1)
    assert bool((after > 0).all()) and info['faces_flipped'] > 0
    inward = (normals.vertex_normals(v, orient.orient_mesh(v, f, 'inward')[1])[0] * centred).sum(dim=1)
    assert bool((inward < 0).all())
