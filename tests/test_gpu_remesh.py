"""GPU tier of the isotropic remeshing: ppsurf_amd/remesh.py and the kernels of csrc/pps_remesh.hip against the numpy
specification tests/remesh_spec.py, byte for byte and twice; each kernel alone on hand-made rows with guard entries around every output; the
argument rules of the C entries; `python -m ppsurf_amd.remesh` end to end; the stages downstream."""
import json

import numpy as np
import pytest
import torch

import decimate_spec as DS
import flip_spec
import remesh_spec as R
import smooth_spec
import subdivide_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64, F64, U8 = torch.int32, torch.int64, torch.float64, torch.uint8
D = np.float64
CANARY = 77
_cache = {}


def dev(a):
    a = np.array(a, order='C')
    if a.dtype == np.uint64:
        a = a.view(np.int64)                                          # the bits of a u64 travel in an int64 tensor
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64).tobytes()


def guarded(rows, cols, dtype):
    """(buffer, its inner rows): `rows` rows between two guard rows, all filled with CANARY."""
    buf = torch.full((rows + 2, cols) if cols else (rows + 2,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1]


def guards_intact(buf):
    return bool((buf[0] == CANARY).all()) and bool((buf[-1] == CANARY).all())


NAMES = ('sphere', 'torus', 'patch', 'fan', 'cube8', 'octahedron', 'tetrahedron', 'welded', 'lattice', 'needles', 'spindle')
BAD = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 642], [0, 1, 1 << 40], [-(1 << 40), 1, 2], [0, 1, (1 << 32) + 2]], dtype=np.int64)


def mesh(name):
    if name not in _cache:
        if name == 'needles':
            _cache[name] = R.needles()[:2]
        elif name == 'spindle':
            _cache[name] = R.spindle()
        elif name == 'lattice':
            _cache[name] = flip_spec.jittered_lattice(12)
        elif name == 'mixed':                                          # invalid faces mixed in and a -0.0 coordinate
            verts, faces = DS.named('sphere')[:2]
            signed = verts.copy()
            signed[17, 1] = -0.0
            _cache[name] = (signed, np.concatenate([faces[:301], BAD, faces[301:]]))
        else:
            _cache[name] = DS.named(name)[:2]
        _cache[name, 'L'] = subdivide_spec.median_edge(*_cache[name]) if name != 'mixed' else subdivide_spec.median_edge(*DS.named('sphere')[:2])
    return _cache[name]


def spec(kind, name, *args):
    key = (kind, name) + args
    if key not in _cache:
        v, f = mesh(name)
        L = _cache[name, 'L']
        if kind == 'collapse':
            low, high, rounds = args
            _cache[key] = R.collapse_spec(v, f, low * L, None if high is None else high * L, rounds)
        elif kind == 'relax':
            _cache[key] = R.relax_spec(v, f, *args)
        else:
            _cache[key] = R.remesh_spec(v, f, factor=args[0], iters=args[1])
    return _cache[key]


def same_mesh(got_v, got_f, want_v, want_f):
    return got_v.dtype == torch.float32 and got_f.dtype == I64 and bits(host(got_v)) == bits(want_v) and bits(host(got_f)) == bits(want_f)


# ---- the three functions against the specification ---------------------------------------------------------------------------------------------
COLLAPSE = [(name, 1.1, high, 1000) for name in NAMES + ('mixed',) for high in (None, 4.0 / 3.0)] + \
           [('sphere', 1.1, None, 1), ('sphere', 1.1, None, 3), ('mixed', 1.1, None, 1), ('needles', 0.5, None, 1000), ('fan', 3.0, None, 3)]


@pytest.mark.parametrize('name,low,high,rounds', COLLAPSE)
def test_collapse_short_edges_matches_the_spec_bytewise(name, low, high, rounds):
    from ppsurf_amd import remesh
    hv, hf = mesh(name)
    L = _cache[name, 'L']
    want_v, want_f, want_info = spec('collapse', name, low, high, rounds)
    v, f = dev(hv), dev(hf)
    for _ in range(2):
        out_v, out_f, info = remesh.collapse_short_edges(v, f, low * L, None if high is None else high * L, rounds)
        assert info == want_info, (info, want_info)
        assert same_mesh(out_v, out_f, want_v, want_f)
        assert json.loads(json.dumps(info)) == info and type(info['converged']) is bool
    if want_info['collapses'] == 0:
        assert out_v is v and out_f is f
    if (name, rounds) == ('sphere', 1):
        assert info['rounds'] == 1 and not info['converged']
    if (name, low) == ('needles', 0.5):
        assert info['vertices_out'] == info['vertices_in'] - R.PLANTED


@pytest.mark.parametrize('name', NAMES + ('mixed', 'four states'))
@pytest.mark.parametrize('iters', [1, 3])
def test_relax_tangential_matches_the_spec_bytewise(name, iters):
    from ppsurf_amd import remesh
    if name == 'four states':
        _cache.setdefault(name, R.four_states())
        _cache.setdefault((name, 'L'), 1.0)
    hv, hf = mesh(name)
    want_v, _, want_info = spec('relax', name, iters, 0.5)
    v, f = dev(hv), dev(hf)
    for _ in range(2):
        out_v, out_f, info = remesh.relax_tangential(v, f, iters, 0.5)
        assert info == want_info, (info, want_info)
        assert out_f is f and out_v.dtype == torch.float32 and bits(host(out_v)) == bits(want_v)
        assert json.loads(json.dumps(info)) == info
    if name == 'four states' and iters == 1:
        assert all(count > 0 for count in info['states'])
    out_v, out_f, info = remesh.relax_tangential(v, f, 0, 0.5)
    assert out_v is v and out_f is f and info == R.relax_spec(hv, hf, 0, 0.5)[2]


@pytest.mark.parametrize('name', NAMES + ('mixed',))
def test_remesh_isotropic_matches_the_spec_bytewise(name):
    from ppsurf_amd import remesh
    hv, hf = mesh(name)
    want_v, want_f, want_info = spec('remesh', name, 1.0, 2)
    v, f = dev(hv), dev(hf)
    for _ in range(2):
        out_v, out_f, info = remesh.remesh_isotropic(v, f, factor=1.0, iters=2)
        assert info == want_info, (info, want_info)
        assert same_mesh(out_v, out_f, want_v, want_f)
        assert json.loads(json.dumps(info)) == info and type(info['limited']) is bool


def test_the_loop_is_the_chain_of_the_four_public_functions():
    from ppsurf_amd import flip, remesh, subdivide
    hv, hf = mesh('needles')
    v, f = dev(hv), dev(hf)
    out_v, out_f, info = remesh.remesh_isotropic(v, f, target_edge=0.16, iters=2, relax_lam=0.4, flip_angle=30.0, max_faces=5000)
    V, F = v, f
    for step in info['iterations']:
        V, F, split = subdivide.split_long_edges(V, F, max_edge=info['high'], max_faces=5000)
        V, F, collapse = remesh.collapse_short_edges(V, F, info['low'], info['high'])
        V, F, flips = flip.flip_edges(V, F, max_angle=30.0)
        V, F, relax = remesh.relax_tangential(V, F, 1, 0.4)
        assert step == {'splits': split['splits'], 'collapses': collapse['collapses'], 'flips': flips['flips'], 'moved': relax['moved']}
    assert len(info['iterations']) == 2 and torch.equal(out_v.view(I32), V.view(I32)) and torch.equal(out_f, F)
    want = R.remesh_spec(hv, hf, target_edge=0.16, iters=2, relax_lam=0.4, flip_angle=30.0, max_faces=5000)
    assert info == want[2] and same_mesh(out_v, out_f, want[0], want[1])
    # what the loop cannot work on comes back as the same objects
    empty_f = torch.zeros(0, 3, dtype=I64, device=DEV)
    out_v, out_f, info = remesh.remesh_isotropic(v, empty_f, factor=1.0)
    assert out_v is v and out_f is empty_f and info == R.remesh_spec(hv, np.zeros((0, 3), np.int64), factor=1.0)[2]
    bad = dev(BAD)
    out_v, out_f, info = remesh.remesh_isotropic(v, bad, factor=1.0)
    assert out_v is v and out_f is bad and info == R.remesh_spec(hv, BAD, factor=1.0)[2]


# ---- the kernels alone -----------------------------------------------------------------------------------------------------------------------------
def prefix_case(ne):
    """test_gpu_decimate's construction: the first `ne` of the 1536 adjacency entries of a jittered torus lattice of 32 x 8 quads with the
    offsets clipped to them, every vertex called regular, the incidence rows whole; what the specification makes of these rows with and
    without an upper bound."""
    if ('prefix', ne) not in _cache:
        verts, faces = DS.torus(32, 8)
        P = verts.astype(D) * (1.0 + 0.05 * np.random.default_rng(2).standard_normal(verts.shape))
        nv = P.shape[0]
        r = R.mesh_rows(faces, nv)
        assert r['nbr'].shape[0] == 1536 and r['regular'].all()
        offsets, nbr = np.minimum(r['offsets'], ne), r['nbr'][:ne]
        L = math_median(P, faces)
        min2, max2 = R.bounds2(1.1 * L, 1.25 * L)
        regular = np.ones(nv, dtype=bool)
        free = R.short_edges_spec(P, faces, offsets, nbr, r['inc_offsets'], r['inc'], regular, min2, np.inf)
        bound = R.short_edges_spec(P, faces, offsets, nbr, r['inc_offsets'], r['inc'], regular, min2, max2)
        is_free, is_bound = free[:, 0] != R.NONE, bound[:, 0] != R.NONE
        # the upper bound refuses candidates that +inf admits, and admits others
        assert is_bound.any() and (is_free & ~is_bound).any() and not (is_bound & ~is_free).any()
        _cache['prefix', ne] = (P, faces, r, offsets, nbr.astype(np.int32), min2, max2, free, bound)
    return _cache['prefix', ne]


def math_median(P, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    e = np.unique(e, axis=0)
    d = P[e[:, 1]] - P[e[:, 0]]
    return float(np.sqrt(np.sort((d * d).sum(axis=1))[(e.shape[0] - 1) // 2]))


@pytest.mark.parametrize('ne', [255, 256, 257, 1280, 1536])
def test_short_edges_alone_on_a_prefix_of_the_rows(ne):
    from ppsurf_amd import _lib
    P, faces, r, offsets, nbr, min2, max2, free, bound = prefix_case(ne)
    nv, nf = P.shape[0], faces.shape[0]
    src = DS.sources(offsets).astype(np.int32)
    d_args = (dev(P), nv, dev(faces), nf, dev(offsets), dev(nbr), dev(src), ne, dev(r['inc_offsets']), dev(r['inc'].astype(np.int32)),
              r['inc'].shape[0], dev(np.ones(nv, dtype=bool)))
    pbuf, d_prio = guarded(ne, 3, I64)
    for _ in range(2):
        for upper, want in ((float('inf'), free), (float(max2), bound)):
            _lib.call('ppsx_remesh_short_edges', d_args[0], d_args[1], d_args[2], d_args[3], d_args[4], d_args[5], d_args[6], d_args[7], d_args[8],
                      d_args[9], d_args[10], d_args[11], float(min2), upper, d_prio)
            assert host(d_prio).tobytes() == want.tobytes() and guards_intact(pbuf)
    if ne == 1536:                                                     # the whole rows: the winners of the round through section 22's entries
        from ppsurf_amd import decimate
        rows = {'offsets': d_args[4], 'nbr': d_args[5], 'src': d_args[6]}
        flag = decimate._winners(rows, d_prio, nv)
        best = DS.ring_min_spec(offsets, r['nbr'], DS.vertex_min_spec(offsets, r['nbr'], bound))
        assert host(flag).astype(bool).tolist() == DS.winners_spec(offsets, r['nbr'], bound, best).tolist() and bool(flag.any())


def test_short_edges_alone_on_the_spindle_and_on_rows_that_cannot_be_read():
    from ppsurf_amd import _lib
    verts, faces = R.spindle()
    nv, nf = verts.shape[0], faces.shape[0]
    P = verts.astype(D)
    r = R.mesh_rows(faces, nv)
    assert np.diff(r['offsets'])[[0, nv - 1]].tolist() == [300, 300] and r['regular'].all()
    ne, ni = r['nbr'].shape[0], r['inc'].shape[0]
    src = DS.sources(r['offsets']).astype(np.int32)
    min2 = D(1.2) * D(1.2)                                            # the spokes of the apexes are shorter than this, most ring edges too
    want = R.short_edges_spec(P, faces, r['offsets'], r['nbr'], r['inc_offsets'], r['inc'], r['regular'], min2, np.inf)
    live = want[:, 0] != R.NONE
    spokes = P[r['nbr'][:300]] - P[0]
    # the 300 entries of the apex's row are short, so each walks the 300 faces and the 300 neighbours of the apex; the thin faces of the
    # other apex turn over, so none of them is a candidate, and the ring edges are
    assert ((spokes * spokes).sum(axis=1) < min2).all() and not live[:300].any() and live[300:].any()
    pbuf, d_prio = guarded(ne, 3, I64)
    fixed = (dev(P), nv, dev(faces), nf)
    tail = (dev(r['inc_offsets']), dev(r['inc'].astype(np.int32)), ni, dev(r['regular']), float(min2), float('inf'), d_prio)
    for _ in range(2):
        _lib.call('ppsx_remesh_short_edges', fixed[0], fixed[1], fixed[2], fixed[3], dev(r['offsets']), dev(r['nbr'].astype(np.int32)), dev(src), ne,
                  tail[0], tail[1], tail[2], tail[3], tail[4], tail[5], tail[6])
        assert host(d_prio).tobytes() == want.tobytes() and guards_intact(pbuf)
    # entries whose ends are out of range or in the wrong order are no candidates, and a neighbour out of range is skipped
    hostile_nbr, hostile_src = r['nbr'].astype(np.int32).copy(), src.copy()
    first = int(np.nonzero(live)[0][0])
    hostile_src[first] = -1
    second = int(np.nonzero(live)[0][1])
    hostile_nbr[second] = nv + 5
    _lib.call('ppsx_remesh_short_edges', fixed[0], fixed[1], fixed[2], fixed[3], dev(r['offsets']), dev(hostile_nbr), dev(hostile_src), ne,
              tail[0], tail[1], tail[2], tail[3], tail[4], tail[5], tail[6])
    got = host(d_prio).view(np.uint64)
    assert (got[[first, second]] == R.NONE).all() and guards_intact(pbuf)


def relax_case(kind):
    """(x f64 [nv,3], faces, rows, regular) of a pass on hand-made sizes: the 256-vertex torus with its last vertex cut off (its faces are
    then invalid and its entries out of range), whole, and with one more vertex that no face uses; the spindle; the four states."""
    if kind in ('255', '256', '257'):
        verts, faces = DS.torus(32, 8)
        x = verts.astype(D) * (1.0 + 0.05 * np.random.default_rng(3).standard_normal(verts.shape))
        r = R.mesh_rows(faces, 256)
        offsets, inc_offsets, regular = r['offsets'], r['inc_offsets'], r['regular']
        if kind == '255':
            x, offsets, inc_offsets, regular = x[:255], offsets[:256], inc_offsets[:256], regular[:255]
        if kind == '257':
            x = np.concatenate([x, [[9.0, 9.0, 9.0]]])
            offsets, inc_offsets, regular = np.append(offsets, offsets[-1]), np.append(inc_offsets, inc_offsets[-1]), np.append(regular, False)
        return x, faces, offsets, r['nbr'], inc_offsets, r['inc'], regular
    verts, faces = R.spindle() if kind == 'spindle' else R.four_states()
    r = R.mesh_rows(faces, verts.shape[0])
    return verts.astype(D), faces, r['offsets'], r['nbr'], r['inc_offsets'], r['inc'], r['regular']


@pytest.mark.parametrize('kind', ['255', '256', '257', 'spindle', 'four states'])
def test_relax_pass_alone(kind):
    from ppsurf_amd import _lib
    x, faces, offsets, nbr, inc_offsets, inc, regular = relax_case(kind)
    nv, nf, ne, ni = x.shape[0], faces.shape[0], nbr.shape[0], inc.shape[0]
    want_y, want_state = R.relax_pass_spec(x, faces, offsets, nbr, inc_offsets, inc, regular, 0.5)
    if kind == 'four states':
        assert np.bincount(want_state, minlength=4).tolist() == [48, 118, 3, 3]
    elif kind == 'spindle':
        assert want_state[[0, nv - 1]].tolist() == [1, 1] and ni == 3 * nf     # both apexes walk 300 faces and move
    else:
        assert int((want_state == 1).sum()) >= 200 and (kind != '257' or want_state[256] == 0)
    ybuf, d_y = guarded(nv, 3, F64)
    sbuf, d_state = guarded(nv, 0, U8)
    d_x = dev(x)
    for _ in range(2):
        _lib.call('ppsx_remesh_relax_pass', d_x, nv, dev(faces), nf, dev(offsets), dev(nbr.astype(np.int32)), ne, dev(inc_offsets),
                  dev(inc.astype(np.int32)), ni, dev(regular), 0.5, d_y, d_state)
        assert host(d_state).tolist() == want_state.tolist() and host(d_y).tobytes() == want_y.tobytes()
        assert guards_intact(ybuf) and guards_intact(sbuf) and host(d_x).tobytes() == x.tobytes()
    if kind == '256':                                                  # rows that cannot be read count as empty: the vertex has no mean and stays
        broken, broken_inc = offsets.copy(), inc_offsets.copy()
        broken[40], broken_inc[80] = offsets[-1] + 5, -1
        want_y, want_state = R.relax_pass_spec(x, faces, broken, nbr, broken_inc, inc, regular, 0.5)
        assert want_state[[39, 40, 79, 80]].tolist() == [2, 2, 2, 2]
        _lib.call('ppsx_remesh_relax_pass', d_x, nv, dev(faces), nf, dev(broken), dev(nbr.astype(np.int32)), ne, dev(broken_inc),
                  dev(inc.astype(np.int32)), ni, dev(regular), 0.5, d_y, d_state)
        assert host(d_state).tolist() == want_state.tolist() and host(d_y).tobytes() == want_y.tobytes() and guards_intact(ybuf) and guards_intact(sbuf)


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, remesh
    hv, hf = mesh('sphere')
    P, nv, nf = hv.astype(D), hv.shape[0], hf.shape[0]
    L = _cache['sphere', 'L']
    min2, max2 = R.bounds2(1.1 * L, None)
    r = R.round_spec(P, hf, nv, min2, max2)
    want_y, want_state = R.relax_pass_spec(P, hf, r['offsets'], r['nbr'], r['inc_offsets'], r['inc'], r['regular'], 0.5)
    ne, ni = r['nbr'].shape[0], r['inc'].shape[0]
    pos, f = dev(P), dev(hf)
    offsets, nbr, src = dev(r['offsets']), dev(r['nbr'].astype(np.int32)), dev(r['src'].astype(np.int32))
    inc_offsets, inc, regular = dev(r['inc_offsets']), dev(r['inc'].astype(np.int32)), dev(r['regular'])
    o_prio = torch.full((ne, 3), CANARY, dtype=I64, device=DEV)
    o_y, o_state = torch.full((nv, 3), float(CANARY), dtype=F64, device=DEV), torch.full((nv,), CANARY, dtype=U8, device=DEV)
    outputs = (o_prio, o_y, o_state)
    big, nan = 2 ** 31, float('nan')

    def untouched():
        torch.cuda.synchronize()
        return all(bool((o == CANARY).all()) for o in outputs) and host(pos).tobytes() == P.tobytes()

    def run(name, defaults, **kw):
        args = dict(defaults, **kw)
        rc = _lib.call(name, *args.values(), on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    entries = {
        'ppsx_remesh_short_edges': (dict(pos=pos, nv=nv, faces=f, nf=nf, offsets=offsets, nbr=nbr, src=src, ne=ne, inc_offsets=inc_offsets, inc=inc,
                                         ni=ni, regular=regular, min2=float(min2), max2=float('inf'), prio=o_prio),
                                    [dict(nv=-1), dict(nv=big), dict(nf=-1), dict(nf=big), dict(ne=-1), dict(ne=big), dict(ni=-1), dict(min2=nan),
                                     dict(min2=-1.0), dict(max2=nan), dict(max2=-1.0), dict(pos=None), dict(faces=None), dict(offsets=None),
                                     dict(nbr=None), dict(src=None), dict(inc_offsets=None), dict(inc=None), dict(regular=None), dict(prio=None)],
                                    dict(ne=0, pos=None, faces=None, offsets=None, nbr=None, src=None, inc_offsets=None, inc=None, regular=None,
                                         prio=None)),
        'ppsx_remesh_relax_pass': (dict(x=pos, nv=nv, faces=f, nf=nf, offsets=offsets, nbr=nbr, ne=ne, inc_offsets=inc_offsets, inc=inc, ni=ni,
                                        regular=regular, lam=0.5, y=o_y, state=o_state),
                                   [dict(nv=-1), dict(nv=big), dict(nf=-1), dict(nf=big), dict(ne=-1), dict(ni=-1), dict(lam=0.0), dict(lam=1.5),
                                    dict(lam=-0.5), dict(lam=nan), dict(x=None), dict(faces=None), dict(offsets=None), dict(nbr=None),
                                    dict(inc_offsets=None), dict(inc=None), dict(regular=None), dict(y=None), dict(state=None), dict(y=pos)],
                                   dict(nv=0, x=None, faces=None, offsets=None, nbr=None, inc_offsets=None, inc=None, regular=None, y=None,
                                        state=None)),
    }
    for name, (defaults, refused, nothing) in entries.items():
        assert list(defaults) == _lib.EXT_PARAMS[name][:-1], name
        for kw in refused:
            assert run(name, defaults, **kw) == 1, (name, kw)
            assert untouched(), (name, kw)
        assert run(name, defaults, **nothing) == 0 and untouched(), name          # zero work: 0, nothing launched, NULLs allowed
    with pytest.raises(_lib.PpsError, match='ppsx_remesh_relax_pass failed with status 1'):
        _lib.call('ppsx_remesh_relax_pass', pos, nv, f, nf, offsets, nbr, ne, inc_offsets, inc, ni, regular, 2.0, o_y, o_state)
    # the good calls after the refused ones
    for name, (defaults, _, _) in entries.items():
        assert run(name, defaults) == 0, name
    assert host(o_prio).tobytes() == r['prio'].tobytes() and int((r['prio'][:, 0] != R.NONE).sum()) > 0
    assert host(o_y).tobytes() == want_y.tobytes() and host(o_state).tolist() == want_state.tolist()
    # the Python layer: the parameters come first, then the device guard, then the mesh
    verts = dev(hv)
    for call, match in ((lambda v, f: remesh.collapse_short_edges(v, f, 0.0), 'min_edge'), (lambda v, f: remesh.relax_tangential(v, f, 1, 2.0), 'lam'),
                        (lambda v, f: remesh.remesh_isotropic(v, f), 'exactly one')):
        with pytest.raises(ValueError, match=match):
            call(verts.cpu(), f)
    for call in (lambda v, f: remesh.collapse_short_edges(v, f, 0.1), lambda v, f: remesh.relax_tangential(v, f, 1, 0.5),
                 lambda v, f: remesh.remesh_isotropic(v, f, factor=1.0)):
        with pytest.raises(remesh.CpuTensorError, match='no CPU'):
            call(verts.cpu(), f)
        with pytest.raises(remesh.CpuTensorError, match='no CPU'):
            call(verts, f.cpu())
        with pytest.raises(ValueError, match='non-finite'):
            call(torch.cat([verts[:5], torch.full((1, 3), float('nan'), device=DEV)]), f[:1])


# ---- the command -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('stage', ['remesh', 'collapse', 'relax'])
def test_the_command_on_a_coloured_ply(tmp_path, capsys, double, stage):
    from ppsurf_amd import meshio, remesh
    verts, faces = mesh('needles')
    faces = np.concatenate([faces[:301], [[0, 0, 1]], faces[301:]])          # a face with a repeated index (a PLY holds no index out of range)
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) + offset[None]
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    argv = {'remesh': ['--factor', '1.0', '--iters', '2'], 'collapse': ['--factor', '0.5'], 'relax': ['--factor', '1.0', '--iters', '3', '--relax_lam', '0.4']}
    report = remesh.main([src, dst] + argv[stage] + ['--stage', stage])
    assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
    stored, stored_f = meshio.read_ply_mesh(src, dtype=np.float64)
    assert np.array_equal(stored_f, faces)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    if stage == 'remesh':
        origin, want_v, want_f, want_rgb, want_info = R.remesh_rows_spec(local, faces, factor=1.0, iters=2, colors=rgb)
        assert sum(step['splits'] for step in want_info['iterations']) > 0 and sum(step['collapses'] for step in want_info['iterations']) >= R.PLANTED
        assert (origin < 0).any()
    elif stage == 'collapse':
        target = 0.5 * subdivide_spec.median_edge(local, np.where(R.valid_faces(faces, local.shape[0])[:, None], faces, -1))
        origin, want_v, want_f, want_info = R.collapse_rows_spec(local, faces, (4.0 * target) / 5.0, None)
        want_rgb = rgb[origin]
        assert want_info['collapses'] == R.PLANTED and want_info['max_edge'] is None and want_info['faces_out'] == 1280 - 2 * R.PLANTED
    else:
        want_v, want_f, want_info = R.relax_spec(local, faces, 3, 0.4)
        origin, want_rgb = np.arange(local.shape[0]), rgb
        assert want_info['moved'] > 600
    assert report == want_info, (report, want_info)
    got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
    assert np.array_equal(got_f, want_f) and got_v.shape == want_v.shape
    # a vertex whose float32 bytes are those of the row it came from is written as read; every other one from its float32 position
    unmoved = origin >= 0
    unmoved[unmoved] = (want_v[unmoved].view(np.int32) == local[origin[unmoved]].view(np.int32)).all(axis=1)
    if stage == 'collapse':
        assert 500 < int(unmoved.sum()) < want_v.shape[0]
    assert np.array_equal(got_v[unmoved], stored[origin[unmoved]])
    moved = want_v[~unmoved].astype(np.float64) + centre[None]
    assert np.array_equal(got_v[~unmoved], moved.astype(np.float32).astype(np.float64) if not double else moved)
    assert np.array_equal(meshio.read_ply_vertex_colors(dst), want_rgb)
    assert (b'property double x' in open(dst, 'rb').read(300)) == double
    with pytest.raises(SystemExit):
        remesh.main([src, dst])                                        # no target: no default is proposed


# ---- downstream --------------------------------------------------------------------------------------------------------------------------------------
def test_the_remeshed_sphere_crosses_nothing_and_stays_one_closed_component():
    from ppsurf_amd import intersect, orient, remesh
    hv, hf = mesh('needles')
    v, f = dev(hv), dev(hf)
    out_v, out_f, info = remesh.remesh_isotropic(v, f, factor=1.0)
    want = spec('remesh', 'needles', 1.0, 5)
    assert info == want[2] and same_mesh(out_v, out_f, want[0], want[1])
    assert intersect.self_intersections(out_v, out_f)[1]['pairs'] == 0
    before, after = orient.orient_mesh(v, f, 'outward')[2], orient.orient_mesh(out_v, out_f, 'outward')[2]
    assert before['components'] == after['components'] == 1 and before['components_closed'] == after['components_closed'] == 1
    assert after['faces_flipped'] == 0 == before['faces_flipped']
    assert R.edge_cv(host(out_v), host(out_f)) < R.edge_cv(hv, hf)
