"""GPU tier of the self-intersection stage: ppsurf_amd/intersect.py and the kernels of csrc/pps_intersect.hip against the
numpy specification tests/intersect_spec.py, byte for byte and twice; the same bytes under every test switch (table capacity, cell edge,
which faces are large); max_pairs; each kernel alone on prefixes of the two-sphere case between canary rows, the emit from hand-made
offsets and counts; the argument rules of the three C entries; `python -m ppsurf_amd.intersect` end to end; and fill.fill_holes on the
mesh that remove_self_intersections cut."""
import json

import numpy as np
import pytest
import torch

import intersect_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32
LIVE_CASES = tuple(n for n in S.CASES if n not in ('empty', 'nothing live'))
_cache = {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def guarded(n, dtype, fill, *tail):
    """(buffer [n + 2, ...] filled with `fill`, its rows 1 .. n): an output between two canary rows."""
    buf = torch.full((n + 2,) + tail, fill, dtype=dtype, device=DEV)
    return buf, buf[1:n + 1]


def untouched(buf, fill):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


def same(t, want):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


def want_of(verts, faces, max_pairs=S.MAX_PAIRS):
    key = (verts.tobytes(), faces.tobytes(), max_pairs)
    if key not in _cache:
        _cache[key] = S.intersect_spec(verts, faces, max_pairs)
    return _cache[key]


def check_run(intersect, verts, faces, what, times=2, **kw):
    max_pairs = kw.get('max_pairs', S.MAX_PAIRS)
    want_flags, want_pairs, want_info = want_of(verts, faces, max_pairs)
    v, f = dev(verts), dev(faces)
    for _ in range(times):
        flags, pairs, info = intersect.self_intersections(v, f, return_pairs=True, **kw)
        assert info == want_info, (what, info, want_info)
        assert flags.dtype == torch.bool and flags.shape == (faces.shape[0],) and pairs.dtype == I64 and pairs.shape == want_pairs.shape, what
        assert same(flags, want_flags) and same(pairs, want_pairs), what
        assert json.loads(json.dumps(info)) == info and type(info['pairs_listed']) is bool and all(type(x) in (int, bool) for x in info.values())
    assert same(v, verts) and same(f, faces), what                                        # the inputs are not written
    return want_info


def switches(intersect, verts, faces):
    """(extent of the default split, number of small faces there, sorted extents of the live faces)."""
    lo, hi, ext, live = intersect.face_boxes(dev(verts), dev(faces))
    assert same(lo, S.boxes(verts, faces)[0]) and same(ext, S.boxes(verts, faces)[2])
    edge = intersect.cell_edge(ext, live)
    extents = np.sort(ext.cpu().numpy()[live.cpu().numpy() != 0])
    return edge, int((extents <= edge).sum()), extents


@pytest.mark.parametrize('name', S.CASES)
def test_self_intersections_match_the_spec_bytewise(name):
    from ppsurf_amd import intersect
    verts, faces = S.case(name)
    info = check_run(intersect, verts, faces, name)
    two = intersect.self_intersections(dev(verts), dev(faces))
    assert len(two) == 2 and same(two[0], want_of(verts, faces)[0]) and two[1] == info
    # a float64 / non-contiguous mesh is taken like its float32 contiguous copy
    wide = dev(np.concatenate([verts.astype(np.float64), np.zeros((verts.shape[0], 1))], axis=1))[:, :3]
    assert not wide.is_contiguous()
    flags, pairs, got = intersect.self_intersections(wide, dev(faces), return_pairs=True)
    assert got == info and same(flags, want_of(verts, faces)[0]) and same(pairs, want_of(verts, faces)[1])


def test_hand_made_pairs_match_the_spec():
    from ppsurf_amd import intersect
    for name, verts, faces, want in S.hand_cases():
        info = check_run(intersect, verts, faces, name)
        assert want_of(verts, faces)[1].tolist() == want and info['pairs'] == len(want), name
    # the pure power-of-two scalings: the same flags and pairs at the edges of the float range
    verts, faces = S.case('two icospheres')
    for scale in (2.0 ** 100, 2.0 ** -100, 2.0 ** 127):
        scaled = (verts.astype(np.float64) * scale).astype(np.float32)
        assert np.isfinite(scaled[:-2]).all() and np.abs(scaled[:-2]).max() > 0
        assert check_run(intersect, scaled, faces, scale, times=1)['pairs'] == want_of(verts, faces)[2]['pairs'] == 88
    # at 2^127 the anchors' box is wider than the largest float: no cell edge serves, and every live face is walked as a list entry
    lo, hi, ext, live = intersect.face_boxes(dev(scaled), dev(faces))
    lists = intersect._Lists(lo, ext, live, intersect.cell_edge(ext, live), None, None)
    assert lists.grid is None and lists.small.shape[0] == 0 and lists.large.shape[0] == 640 and bool(torch.isfinite(ext).all())


@pytest.mark.parametrize('name', LIVE_CASES)
def test_the_switches_change_no_byte(name):
    from ppsurf_amd import _lib, intersect
    verts, faces = S.case(name)
    edge, ns, extents = switches(intersect, verts, faces)
    assert edge > 0 and ns > 0
    smallest = 1 << int(ns).bit_length()                                                  # the smallest power of two > ns
    default = int(_lib.lib().pps_cloud_table_capacity(ns))
    assert smallest > ns and smallest // 2 <= ns and default >= 2 * ns
    for capacity in (smallest, 4 * default):
        check_run(intersect, verts, faces, (name, 'capacity', capacity), times=1, capacity=capacity)
    # 50 x: every anchor in a few cells and never more cells than anchors; 1 x: the long faces open more cells than there are anchors
    for times in (1.0, 3.0, 50.0):
        check_run(intersect, verts, faces, (name, 'cell', times), times=1, cell=times * edge)
        check_run(intersect, verts, faces, (name, 'cell and capacity', times), times=1, cell=times * edge, capacity=smallest)
    none_large, half_large, all_large = float(extents[-1]), float(extents[(extents.shape[0] - 1) // 2]), -1.0
    for large_above in (none_large, half_large, all_large):
        check_run(intersect, verts, faces, (name, 'large_above', large_above), times=1, large_above=large_above)
    check_run(intersect, verts, faces, (name, 'half large, wide cells'), times=1, large_above=half_large, cell=7.0 * none_large)
    half_small = int((extents <= half_large).sum())
    check_run(intersect, verts, faces, (name, 'half large, tight table'), times=1, large_above=half_large, capacity=1 << half_small.bit_length())


def test_the_lists_do_what_the_switches_say():
    """The switch tests prove nothing if the switches are ignored: the lists they build are looked at here."""
    from ppsurf_amd import intersect
    verts, faces = S.case('large triangle')
    lo, hi, ext, live = intersect.face_boxes(dev(verts), dev(faces))
    edge, ns, extents = switches(intersect, verts, faces)
    lists = intersect._Lists(lo, ext, live, edge, None, None)
    assert lists.large.cpu().tolist() == [int(np.argmax(ext.cpu().numpy()))] and lists.small.shape[0] == ns == 320     # the triangle alone is large
    assert float(lists.grid.h) >= edge and lists.grid.capacity >= 2 * ns
    assert intersect._Lists(lo, ext, live, -1.0, None, None).grid is None and intersect._Lists(lo, ext, live, -1.0, None, None).large.shape[0] == 321
    assert intersect._Lists(lo, ext, live, float(extents[-1]), None, None).large.shape[0] == 0
    assert 50.0 * edge <= float(intersect._Lists(lo, ext, live, edge, 50.0 * edge, 512).grid.h) <= 50.0 * edge * (1.0 + 1e-6)
    assert intersect._Lists(lo, ext, live, edge, None, 512).grid.capacity == 512
    with pytest.raises(ValueError, match='below large_above'):
        intersect.self_intersections(dev(verts), dev(faces), cell=0.5 * edge)


def test_max_pairs_one_below_the_count_lists_nothing():
    from ppsurf_amd import intersect
    verts, faces = S.case('two cubes 1.5')
    total = want_of(verts, faces)[2]['pairs']
    assert total == 90
    short = check_run(intersect, verts, faces, 'one short', max_pairs=total - 1)
    assert not short['pairs_listed'] and short['pairs'] == total and short['faces_intersecting'] == 60
    assert want_of(verts, faces, total - 1)[1].shape == (0, 2) and same(dev(want_of(verts, faces, total - 1)[0]), want_of(verts, faces)[0])
    assert check_run(intersect, verts, faces, 'exact', max_pairs=total)['pairs_listed']
    flags, info = intersect.self_intersections(dev(verts), dev(faces), max_pairs=0)
    assert not info['pairs_listed'] and same(flags, want_of(verts, faces)[0])


def prefix_tables(n, large_above, cell=None, capacity=None):
    """The first n faces (all for None) of the two-sphere case in a fixed random order, so that a prefix holds faces of both spheres, with
    the specification's boxes and per-face results and the lists on the device."""
    from ppsurf_amd import intersect
    verts, faces = S.case('two icospheres')
    faces = np.ascontiguousarray(faces[np.random.default_rng(7).permutation(faces.shape[0])])
    faces = faces if n is None else np.ascontiguousarray(faces[:n])
    lo, hi, ext, live = S.boxes(verts, faces)
    lists = intersect._Lists(dev(lo), dev(ext), dev(live), large_above, cell, capacity)
    return verts, faces, (lo, hi, ext, live), S.per_face(verts, faces), lists


@pytest.mark.parametrize('n', [255, 256, 257, None])
def test_each_kernel_alone_on_a_prefix(n):
    from ppsurf_amd import _lib
    verts, faces, (lo, hi, ext, live), (want_flag, want_count, want_boxed, want_pairs), _ = prefix_tables(n, 1.0)
    nv, nf = verts.shape[0], faces.shape[0]
    assert S.case('two icospheres')[1].shape[0] == 647 and want_pairs.shape[0] > 0 and 0 < live.sum() < nf
    dv, df = dev(verts), dev(faces)
    lbuf, dlo = guarded(nf, F32, -7.0, 3)
    hbuf, dhi = guarded(nf, F32, -7.0, 3)
    ebuf, dext = guarded(nf, F32, -7.0)
    vbuf, dlive = guarded(nf, U8, 7)
    for _ in range(2):
        _lib.call('ppsx_intersect_boxes', dv, nv, df, nf, dlo, dhi, dext, dlive)
        assert same(dlo, lo) and same(dhi, hi) and same(dext, ext) and same(dlive, live)
        assert untouched(lbuf, -7.0) and untouched(hbuf, -7.0) and untouched(ebuf, -7.0) and untouched(vbuf, 7)
    median = float(np.sort(ext[live != 0])[(int(live.sum()) - 1) // 2])
    for large_above, cell in ((1.0, None), (median, None), (median, 3.0), (-1.0, None)):
        lists = prefix_tables(n, large_above, cell)[4]
        assert (lists.grid is None) == (large_above < 0) and lists.small.shape[0] + lists.large.shape[0] == int(live.sum())
        fbuf, dflag = guarded(nf, U8, 7)
        cbuf, dcount = guarded(nf, I32, -7)
        bbuf, dboxed = guarded(nf, I32, -7)
        for _ in range(2):
            _lib.call('ppsx_intersect_count', dv, nv, df, nf, dlo, dhi, dlive, *lists.args(), dflag, dcount, dboxed)
            assert same(dflag, want_flag) and same(dcount, want_count) and same(dboxed, want_boxed), (n, large_above, cell)
            assert untouched(fbuf, 7) and untouched(cbuf, -7) and untouched(bbuf, -7)
        # the emit from hand-made tables: one spare row after the pairs of every face, one face a pair short, one that starts before the
        # table, one that would run over its end
        owners = np.nonzero(want_count)[0]
        assert owners.shape[0] >= 4
        short = owners[np.argmax(want_count[owners])]
        before, over = [o for o in owners if o != short][:2]
        count = want_count.copy()
        count[short] -= 1
        offsets = np.cumsum(want_count.astype(np.int64) + 1) - (want_count + 1)
        total = int(offsets[-1] + want_count[-1] + 1)
        offsets[before], offsets[over] = -1, total - count[over] + 1
        pbuf, dpairs = guarded(total, I64, -7, 2)
        for _ in range(2):
            dpairs.fill_(-7)
            _lib.call('ppsx_intersect_emit', dv, nv, df, nf, dlo, dhi, dlive, *lists.args(), dev(count), dev(offsets), total, dpairs)
            got = dpairs.cpu().numpy()
            written = np.zeros(total, dtype=bool)
            for f in owners:
                mine = want_pairs[want_pairs[:, 0] == f]
                if f in (before, over):
                    continue
                rows = got[offsets[f]:offsets[f] + count[f]]
                written[offsets[f]:offsets[f] + count[f]] = True
                keys = {tuple(r) for r in rows.tolist()}
                assert len(keys) == count[f] and keys <= {tuple(r) for r in mine.tolist()}, (n, f)       # distinct pairs of f, in the walk's order
                if f != short:
                    assert np.array_equal(rows[np.argsort(rows[:, 1])], mine), (n, f)
            assert (got[~written] == -7).all() and untouched(pbuf, -7), n                                   # the pair too many, the spare rows, the two refused faces
    assert same(dv, verts) and same(df, faces)


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, intersect
    n = None
    hv, hf, (hlo, hhi, hext, hlive), (want_flag, want_count, want_boxed, want_pairs), _ = prefix_tables(n, 1.0)
    median = float(np.sort(hext[hlive != 0])[(int(hlive.sum()) - 1) // 2])
    L = prefix_tables(n, median)[4]
    small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl = L.args()
    assert ns > 0 and nl > 0
    nv, nf, total = hv.shape[0], hf.shape[0], want_pairs.shape[0]
    verts, faces = dev(hv), dev(hf)
    lo, hi, ext, live = (torch.full((nf, 3), -7.0, dtype=F32, device=DEV), torch.full((nf, 3), -7.0, dtype=F32, device=DEV),
                         torch.full((nf,), -7.0, dtype=F32, device=DEV), torch.full((nf,), 7, dtype=U8, device=DEV))
    glo_in, ghi_in, glive = dev(hlo), dev(hhi), dev(hlive)
    flag, count, boxed = torch.full((nf,), 7, dtype=U8, device=DEV), torch.full((nf,), -7, dtype=I32, device=DEV), torch.full((nf,), -7, dtype=I32, device=DEV)
    pairs = torch.full((total, 2), -7, dtype=I64, device=DEV)
    good_count, good_offsets = dev(want_count), dev(np.cumsum(want_count.astype(np.int64)) - want_count)
    big = 2 ** 31

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def boxes(verts=verts, nv=nv, faces=faces, nf=nf, lo=lo, hi=hi, ext=ext, live=live):
        return run('ppsx_intersect_boxes', verts, nv, faces, nf, lo, hi, ext, live)

    def walk(emit, verts=verts, nv=nv, faces=faces, nf=nf, lo=glo_in, hi=ghi_in, live=glive, small=small, ns=ns, glo=glo, ghi=ghi, h=h, inv_h=inv_h,
             table=table, capacity=capacity, order=order, offsets=offsets, large=large, nl=nl, flag=flag, count=count, boxed=boxed,
             good_count=good_count, pair_offsets=good_offsets, np_=total, pairs=pairs):
        head = (verts, nv, faces, nf, lo, hi, live, small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl)
        if emit:
            return run('ppsx_intersect_emit', *head, good_count, pair_offsets, np_, pairs)
        return run('ppsx_intersect_count', *head, flag, count, boxed)

    def clean():
        return (bool((lo == -7.0).all()) and bool((hi == -7.0).all()) and bool((ext == -7.0).all()) and bool((live == 7).all()) and bool((flag == 7).all())
                and bool((count == -7).all()) and bool((boxed == -7).all()) and bool((pairs == -7).all()) and same(faces, hf) and same(verts, hv))

    for kw in (dict(nf=-1), dict(nv=-1), dict(nf=big), dict(nv=big), dict(verts=None), dict(faces=None), dict(lo=None), dict(hi=None), dict(ext=None),
               dict(live=None)):
        assert boxes(**kw) == 1, kw
        assert clean(), kw
    assert boxes(nf=0) == 0 and boxes(nf=0, verts=None, faces=None, lo=None, hi=None, ext=None, live=None) == 0 and clean()
    shared = (dict(nf=-1), dict(nv=-1), dict(ns=-1), dict(nl=-1), dict(nf=big), dict(nv=big), dict(ns=nf + 1), dict(nl=nf - ns + 1), dict(h=-1.0),
              dict(h=float('nan')), dict(h=0.0), dict(inv_h=0.0), dict(h=float('inf')), dict(capacity=capacity - 1), dict(capacity=0),
              dict(capacity=1 << (int(ns).bit_length() - 1)), dict(verts=None), dict(faces=None), dict(lo=None), dict(hi=None), dict(live=None),
              dict(small=None), dict(glo=None), dict(ghi=None), dict(table=None), dict(order=None), dict(offsets=None), dict(large=None))
    for emit, more in ((False, (dict(flag=None), dict(count=None), dict(boxed=None))),
                       (True, (dict(np_=-1), dict(good_count=None), dict(pair_offsets=None), dict(pairs=None)))):
        for kw in shared + more:
            assert walk(emit, **kw) == 1, (emit, kw)
            assert clean(), (emit, kw)
        nothing = dict(verts=None, faces=None, lo=None, hi=None, live=None, small=None, ns=0, glo=None, ghi=None, table=None, capacity=0, order=None,
                       offsets=None, large=None, nl=0, flag=None, count=None, boxed=None, good_count=None, pair_offsets=None, pairs=None)
        assert walk(emit, nf=0, ns=0, nl=0) == 0 and walk(emit, nf=0, **nothing) == 0 and clean()
    assert walk(True, np_=0) == 0 and walk(True, np_=0, pairs=None) == 0 and clean()
    with pytest.raises(_lib.PpsError, match='ppsx_intersect_boxes failed with status 1'):
        _lib.call('ppsx_intersect_boxes', verts, nv, faces, -1, lo, hi, ext, live)
    # the good calls after the refused ones
    assert boxes() == 0 and walk(False) == 0 and walk(True) == 0
    assert same(lo, hlo) and same(hi, hhi) and same(ext, hext) and same(live, hlive)
    assert same(flag, want_flag) and same(count, want_count) and same(boxed, want_boxed)
    keys = torch.sort((pairs[:, 0] << 32) | pairs[:, 1])[0]
    assert same(torch.stack([keys >> 32, keys & 0xFFFFFFFF], dim=1), want_pairs)
    # the Python layer: the parameter comes first, CPU tensors are refused, non-finite vertices are taken
    for bad in (-1, 2 ** 31, 1.5, True, None):
        with pytest.raises(ValueError, match='max_pairs'):
            intersect.self_intersections(verts.cpu(), faces, max_pairs=bad)
    with pytest.raises(intersect.CpuTensorError, match='no CPU'):
        intersect.self_intersections(verts.cpu(), faces)
    with pytest.raises(intersect.CpuTensorError, match='no CPU'):
        intersect.remove_self_intersections(verts, faces.cpu())
    assert not bool(torch.isfinite(verts).all())


def test_remove_returns_the_given_tensors_and_the_kept_rows():
    from ppsurf_amd import intersect
    verts, faces = S.case('two cubes 1.5')
    want_flags, _, want_info = want_of(verts, faces)
    v, f = dev(verts), dev(faces)
    for _ in range(2):
        out_v, out_f, rows, info = intersect.remove_self_intersections(v, f)
        want_f, want_rows = S.removed(faces, want_flags)
        assert out_v is v and same(out_f, want_f) and same(rows, want_rows) and rows.dtype == I64
        assert info == dict(want_info, faces_out=want_f.shape[0]) and json.loads(json.dumps(info)) == info
    assert same(v, verts) and same(f, faces)
    verts, faces = S.case('icosphere')
    v, f = dev(verts), dev(faces)
    out_v, out_f, rows, info = intersect.remove_self_intersections(v, f)
    assert out_v is v and out_f is f and rows.cpu().tolist() == list(range(faces.shape[0])) and info['faces_out'] == info['faces_in'] == 327
    empty = intersect.remove_self_intersections(v, f[:0])
    assert empty[1].shape == (0, 3) and empty[2].shape == (0,) and empty[3]['faces_in'] == 0


@pytest.mark.parametrize('double', [False, True])
def test_the_command_reports_removes_and_selects_on_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import intersect, meshio
    verts, faces = S.clean('two icospheres')
    faces = np.concatenate([faces[:30], [[0, 0, 1]], faces[30:]])        # a face with a repeated index (a PLY holds no index out of range)
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) + offset[None]
    nv = verts.shape[0]
    rgb = np.random.default_rng(5).integers(0, 256, size=(nv, 3)).astype(np.uint8)
    src, dst, npy = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply'), str(tmp_path / 'pairs.npy')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    stored, stored_f = meshio.read_ply_mesh(src, dtype=np.float64)
    assert np.array_equal(stored_f, faces)
    centre = (stored.min(axis=0) + stored.max(axis=0)) * 0.5
    local = (stored - centre[None]).astype(np.float32)
    want_flags, want_pairs, want_info = S.intersect_spec(local, faces)
    assert want_info['pairs'] > 40 and want_info['faces_live'] == 640 and want_info['faces_in'] == 641

    def last_line():
        return json.loads(capsys.readouterr().out.strip().split('\n')[-1])

    report = intersect.main([src])                                      # report only
    assert last_line() == report == want_info
    report = intersect.main([src, '--pairs_out', npy, '--max_pairs', '100000'])
    assert last_line() == report == dict(want_info, max_pairs=100000) and np.array_equal(np.load(npy), want_pairs) and np.load(npy).dtype == np.int64
    for extra, keep in (([], ~want_flags), (['--action', 'remove'], ~want_flags), (['--action', 'select', '--pairs_out', npy], want_flags)):
        report = intersect.main([src, dst] + extra)
        assert last_line() == report == want_info
        got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
        assert np.array_equal(got_f, faces[keep]) and got_v.tobytes() == stored.tobytes()       # the vertices: the file's own values
        assert np.array_equal(meshio.read_ply_vertex_colors(dst), rgb)
        assert (b'property double x' in open(dst, 'rb').read(300)) == double
    assert np.array_equal(np.load(npy), want_pairs)
    short = intersect.main([src, '--pairs_out', npy, '--max_pairs', str(want_info['pairs'] - 1)])
    capsys.readouterr()
    assert not short['pairs_listed'] and np.load(npy).shape == (0, 2)


def test_fill_runs_on_the_mesh_that_remove_cut():
    from ppsurf_amd import fill, intersect
    verts, faces = S.clean('two icospheres')
    flags = S.intersect_spec(verts, faces)[0]
    kept = S.removed(faces, flags)[0]
    assert S.intersect_spec(verts, kept)[2]['pairs'] == 0                # the specification first: nothing crosses among the kept faces
    v, f = dev(verts), dev(faces)
    out_v, out_f, rows, info = intersect.remove_self_intersections(v, f)
    assert same(out_f, kept) and info['faces_intersecting'] == 88 and info['faces_out'] == 640 - 88
    assert intersect.self_intersections(out_v, out_f)[1]['pairs'] == 0
    filled = fill.fill_holes(out_v, out_f, 64)
    left = intersect.self_intersections(filled[0], filled[1])[1]
    assert left['faces_in'] >= info['faces_out'] and left['faces_live'] <= left['faces_in'] and left['pairs'] >= 0      # it runs; what remains is reported
