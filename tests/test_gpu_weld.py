"""GPU tier of the weld stage: ppsurf_amd/weld.py and the kernels of csrc/pps_weld.hip against the numpy specification
tests/weld_spec.py, byte for byte and twice, at eps = 0 and eps > 0; the labels under other cell edges and table capacities; hook and
compress alone between canary rows; the face kernel alone; the argument rules of the C entries; `python -m ppsurf_amd.weld` end to end on a
coloured PLY and on an STL; and the stages that did nothing on a soup -- pieces, orient, decimate -- after the weld."""
import json

import numpy as np
import pytest
import torch

import orient_spec
import weld_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
_cache = {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def spec(name, eps):
    """(verts out, faces out, info, parts) of the specification on a named case at eps, computed once."""
    if (name, eps) not in _cache:
        verts, faces, _ = S.case(name)
        _cache[(name, eps)] = S.weld_spec(verts, faces, eps, name in S.DROP)
    return _cache[(name, eps)]


def guarded(n, dtype, fill, *tail):
    """(buffer [n + 2, ...] filled with `fill`, its rows 1 .. n): an output between two canary rows."""
    buf = torch.full((n + 2,) + tail, fill, dtype=dtype, device=DEV)
    return buf, buf[1:n + 1]


def untouched(buf, fill):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


def both_eps(name):
    """0 and a positive eps for a named case: its own where it has one, else 10^-3, far below every edge of the fixtures."""
    own = S.case(name)[2]
    return (0.0, own if own > 0 else 1.0e-3)


@pytest.mark.parametrize('name', S.CASES)
def test_weld_mesh_and_vertex_clusters_match_the_spec_bytewise(name):
    from ppsurf_amd import weld
    verts, faces, _ = S.case(name)
    v, f = dev(verts), dev(faces)
    for eps in both_eps(name):
        want_v, want_f, want_info, parts = spec(name, eps)
        for _ in range(2):
            leader = weld.vertex_clusters(v, eps)
            assert leader.dtype == I32 and leader.cpu().numpy().tobytes() == parts['leader'].tobytes(), eps
            out_v, out_f, info = weld.weld_mesh(v, f, eps, name in S.DROP)
            assert info == want_info and json.loads(json.dumps(info)) == info, (eps, info, want_info)
            assert out_v.dtype == torch.float32 and out_f.dtype == I64
            assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes(), eps
            assert (out_v is v) == parts['same'] and (out_f is f) == parts['same'], eps
    assert f.cpu().numpy().tobytes() == faces.tobytes() and v.cpu().numpy().tobytes() == verts.tobytes()          # the inputs are not written


@pytest.mark.parametrize('name', ['sphere soup jitter', 'cloud eps', 'chain 1025 shuffled', 'crowd eps', 'cube soup'])
def test_the_grid_does_not_show_in_the_labels(name):
    from ppsurf_amd import trim, weld
    verts, _, eps = S.case(name)
    v = dev(verts)
    want = spec(name, eps)[3]['leader']
    grid = trim.SupportGrid(v)
    h = float(grid.edge_for(max(min(eps, float(grid.ext)), weld.H_FLOOR)))
    default = int(grid.capacity)
    assert default >= 2 * verts.shape[0] and h >= min(eps, float(grid.ext))
    for cell, capacity in ((None, None), (3.7 * h, None), (0.3 * h, None), (None, 4 * default), (3.7 * h, default // 2 if default // 2 > verts.shape[0] else 2 * default)):
        if cell is not None and float(grid.ext) / cell >= 2 ** 20 - 1:
            continue                                                    # (a finer grid than the rule of pps_cells.h takes)
        leader, rounds = weld._clusters(v, eps, cell=cell, capacity=capacity)
        assert leader.cpu().numpy().tobytes() == want.tobytes() and rounds >= 2, (cell, capacity)


def lists(verts, eps, cell=None, capacity=None):
    """The cell lists weld._clusters builds for device vertices."""
    from ppsurf_amd import trim, weld
    grid = trim.SupportGrid(verts, capacity)
    return grid.build(grid.edge_for(max(min(eps, float(grid.ext)), weld.H_FLOOR)) if cell is None else trim._f32_not_below(cell))


def hook(grid, eps, label, changed, order=None, n=None):
    from ppsurf_amd import _lib
    _lib.call('ppsx_weld_hook', grid.pts, grid.n if n is None else n, grid._vec3(grid.lo), grid._vec3(grid.hi), float(grid.h), float(grid.inv_h),
              grid._table, grid.capacity, grid.order if order is None else order, grid.offsets, eps, label, changed)


def fixed_point(grid, eps, label, order=None):
    """The host loop of weld._clusters on given lists and labels."""
    from ppsurf_amd import _lib
    changed = torch.zeros(1, dtype=I32, device=DEV)
    for rounds in range(1, 100):
        changed.zero_()
        hook(grid, eps, label, changed, order)
        assert int(changed.item()) in (0, 1)
        if int(changed.item()) == 0:
            return rounds
        _lib.call('ppsx_labels_compress', label, grid.n)
    raise AssertionError('no fixed point')


def labelled(verts, eps, cell=None):
    """(labels at the fixed point, rounds) of hook and compress alone, the labels between canary rows."""
    n = verts.shape[0]
    grid = lists(dev(verts), eps, cell)
    lbuf, label = guarded(n, I32, -7)
    label.copy_(torch.arange(n, dtype=I32, device=DEV))
    rounds = fixed_point(grid, eps, label)
    assert untouched(lbuf, -7)
    assert fixed_point(grid, eps, label) == 1                          # a fixed point writes nothing and says so at once
    return label.cpu().numpy(), rounds


@pytest.mark.parametrize('n', [255, 256, 257])
def test_hook_and_compress_alone_on_a_lattice_with_walls(n):
    pts = S.case('cloud')[0][:n]                                       # integer coordinates 0 .. 5: with h = 1 every point lies on a cell wall or at hi
    for eps in (0.0, 1.0):                                             # at eps = 1 the lattice neighbours are linked at d2 == eps2 across a wall
        got, rounds = labelled(pts, eps, cell=1.0)
        want = S.clusters_spec(pts, eps)
        assert got.tobytes() == want.tobytes() and rounds >= 2 and 1 <= len(set(want.tolist())) < n, eps
    assert (S.clusters_spec(pts, 1.0) == 0).all() and not (S.clusters_spec(pts, float(np.nextafter(1.0, 0.0))) == 0).all()
    assert labelled(pts, float(np.nextafter(1.0, 0.0)), cell=1.0)[0].tobytes() == S.clusters_spec(pts, 0.0).tobytes()


@pytest.mark.parametrize('order', ['ascending', 'reversed', 'shuffled'])
def test_a_chain_of_1025_points_is_one_cluster(order):
    pts = S.chain(1025, order)
    got, rounds = labelled(pts, S.CHAIN_EPS)
    assert (got == 0).all() and rounds >= 2
    got, _ = labelled(pts, 0.8 * S.CHAIN_EPS)                         # below the spacing: nothing is linked
    assert got.tolist() == list(range(1025))


def test_hook_and_compress_on_crowds_walls_and_single_vertices():
    from ppsurf_amd import _lib, weld
    crowd = S.case('crowd')[0]
    for eps in (0.0, 0.01):
        grid = lists(dev(crowd), eps)
        assert float(grid.ext) == 0.0 and float(grid.h) == weld.H_FLOOR                                # an extent of 0: the floor on the cell edge
        got, rounds = labelled(crowd, eps)
        assert (got == 0).all() and rounds >= 2
    # a linked pair that straddles a wall at d2 == eps2: h = 5 over lo = 0 puts (4, 4, 0) in cell (0, 0, 0) and (7, 8, 0) in (1, 1, 0)
    far = np.stack([100.0 + 10.0 * np.arange(40), np.full(40, 50.0), np.full(40, 50.0)], axis=1)          # 40 lone points: 45 vertices in all
    pts = np.concatenate([np.array([[0, 0, 0], [4, 4, 0], [7, 8, 0], [20, 20, 20], [20, 15, 20]]), far]).astype(np.float32)
    want = [0, 1, 1, 3, 3] + list(range(5, 45))
    assert S.clusters_spec(pts, 5.0).tolist() == want
    for cell in (5.0, 2.0, 1000.0):                                    # 5.0: 27 cells; 2.0: more cells than vertices, so every vertex walks the rows below it
        assert labelled(pts, 5.0, cell)[0].tolist() == want, cell
        assert labelled(pts, float(np.nextafter(5.0, 0.0)), cell)[0].tolist() == list(range(45)), cell
    # an eps far above the box and above the float32 range: one cluster, the cell edge is the box's
    assert labelled(pts, 1.0e6)[0].tolist() == [0] * 45 and labelled(pts, 1.0e300)[0].tolist() == [0] * 45
    # a single vertex, and none
    got, rounds = labelled(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), 0.5)
    assert got.tolist() == [0] and rounds == 1
    changed = torch.zeros(1, dtype=I32, device=DEV)
    _lib.call('ppsx_weld_hook', None, 0, None, None, 1.0, 1.0, None, 64, None, None, 0.0, None, changed)
    assert changed.item() == 0


def test_labels_and_order_entries_out_of_range_are_skipped_not_read_through():
    from ppsurf_amd import _lib
    pts = S.case('cloud')[0][:257]
    hi, lo = S.linked_pairs(pts, 0.0)
    grid = lists(dev(pts), 0.0)
    # order entries out of range: the rows they stood for are never visited as the lower end of a link
    rows = np.unique(lo)[[0, 1, 5, -1]]                                # four rows that are the lower end of a link
    gone = np.nonzero(np.isin(grid.order.cpu().numpy(), rows))[0]      # their positions in `order`
    order = grid.order.clone()
    order[dev(gone)] = dev(np.array([-1, 257, 1 << 40, -(1 << 62)], dtype=np.int64))
    lbuf, label = guarded(257, I32, -7)
    label.copy_(torch.arange(257, dtype=I32, device=DEV))
    fixed_point(grid, 0.0, label, order)
    keep = ~np.isin(lo, rows)
    assert label.cpu().numpy().tobytes() == S.clusters_of_pairs(257, hi[keep], lo[keep]).tobytes() and untouched(lbuf, -7)
    assert not np.array_equal(S.clusters_of_pairs(257, hi[keep], lo[keep]), S.clusters_spec(pts, 0.0))
    # labels out of range: a negative one takes its vertex out, one above its slot ends a walk like a root and falls with the first hook
    start = np.arange(257, dtype=np.int32)
    out = np.array([3, 40, 41, 200])
    start[out] = [-1, -(1 << 31), -5, -2]
    above = np.array([7, 90, 256])
    start[above] = [300, (1 << 31) - 1, 257]
    label.copy_(dev(start))
    fixed_point(grid, 0.0, label)
    live = ~np.isin(hi, out) & ~np.isin(lo, out)
    want = S.clusters_of_pairs(257, hi[live], lo[live])
    want[out] = start[out]                                             # (compress stores its own index into a root with a label above it)
    assert label.cpu().numpy().tobytes() == want.tobytes() and untouched(lbuf, -7)


@pytest.mark.parametrize('nf', [255, 256, 257])
def test_the_face_kernel_alone(nf):
    from ppsurf_amd import _lib
    nv = 100
    rng = np.random.default_rng(nf)
    faces = rng.integers(0, nv, size=(nf, 3)).astype(np.int64)
    faces[::31] = [[-1, 2, 3]]
    faces[7::31, 2] = 1 << 40
    faces[9::31, 1] = nv
    newrow = (np.arange(nv) // 2).astype(np.int64)                     # pairs of rows merge
    newrow[[10, 50]] = [-1, nv]                                        # entries out of range: their faces get code 1
    want, code = S.faces_spec(faces, nv, newrow)
    assert set(code.tolist()) == {0, 1, 2} and (want[code != 0] == faces[code != 0]).all() and (code[np.isin(faces, [10, 50]).any(axis=1)] == 1).all()
    obuf, out = guarded(nf, I64, -7, 3)
    cbuf, got = guarded(nf, U8, 9)
    for _ in range(2):
        _lib.call('ppsx_weld_faces', dev(faces), nf, nv, dev(newrow), out, got)
        assert out.cpu().numpy().tobytes() == want.tobytes() and got.cpu().numpy().tobytes() == code.tobytes()
        assert untouched(obuf, -7) and untouched(cbuf, 9)
    _lib.call('ppsx_weld_faces', dev(faces), nf, 0, None, out, got)          # no vertex: every face is invalid, newrow is not read
    assert out.cpu().numpy().tobytes() == faces.tobytes() and bool((got == 1).all()) and untouched(obuf, -7) and untouched(cbuf, 9)


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, weld
    pts, faces, _ = S.case('torus soup')
    n, nf = pts.shape[0], faces.shape[0]
    grid = lists(dev(pts), 0.0)
    f = dev(faces)
    label0 = torch.arange(n, dtype=I32, device=DEV)
    label = label0.clone()
    changed = torch.zeros(1, dtype=I32, device=DEV)
    newrow = torch.zeros(n, dtype=I64, device=DEV)
    out, code = torch.full((nf, 3), -7, dtype=I64, device=DEV), torch.full((nf,), 9, dtype=U8, device=DEV)
    lo, hi = grid._vec3(grid.lo), grid._vec3(grid.hi)
    big = 2 ** 31

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def hook_(pts=grid.pts, n=n, lo=lo, hi=hi, h=float(grid.h), inv_h=float(grid.inv_h), table=grid._table, capacity=grid.capacity, order=grid.order,
              offsets=grid.offsets, eps=0.0, label=label, changed=changed):
        return run('ppsx_weld_hook', pts, n, lo, hi, h, inv_h, table, capacity, order, offsets, eps, label, changed)

    def faces_(faces=f, nf=nf, nv=n, newrow=newrow, out=out, code=code):
        return run('ppsx_weld_faces', faces, nf, nv, newrow, out, code)

    for kw in (dict(n=-1), dict(n=big), dict(eps=-1.0e-300), dict(eps=float('nan')), dict(pts=None), dict(lo=None), dict(hi=None), dict(table=None),
               dict(order=None), dict(offsets=None), dict(changed=None), dict(h=0.0), dict(inv_h=0.0), dict(h=float('inf')), dict(capacity=n),
               dict(capacity=grid.capacity - 1), dict(capacity=0), dict(h=1.0e-7, inv_h=1.0e7)):
        assert hook_(**kw) == 1, kw
        assert torch.equal(label, label0) and changed.item() == 0, kw
    assert hook_(label=None) == 1 and hook_(n=0) == 0 and changed.item() == 0
    assert hook_(n=0, pts=None, lo=None, hi=None, table=None, order=None, offsets=None, label=None, changed=None) == 0
    for kw in (dict(nf=-1), dict(nv=-1), dict(nf=big), dict(nv=big), dict(faces=None), dict(newrow=None), dict(code=None), dict(faces=out)):
        assert faces_(**kw) == 1, kw
        assert bool((out == -7).all()) and bool((code == 9).all()), kw
    assert faces_(out=None) == 1 and faces_(nf=0) == 0 and faces_(nf=0, faces=None, newrow=None, out=None, code=None) == 0
    assert bool((out == -7).all()) and bool((code == 9).all())
    # the good calls after the refused ones
    assert fixed_point(grid, 0.0, label) >= 2 and label.cpu().numpy().tobytes() == spec('torus soup', 0.0)[3]['leader'].tobytes()
    assert faces_() == 0 and bool((code == 2).all()) and out.cpu().numpy().tobytes() == faces.tobytes()          # every row is row 0: all collapse
    # the Python layer
    v = dev(pts)
    with pytest.raises(ValueError, match='non-finite'):
        weld.weld_mesh(torch.cat([v[:5], torch.full((1, 3), float('nan'), device=DEV)]), f[:1])
    with pytest.raises(ValueError, match='non-finite'):
        weld.vertex_clusters(torch.cat([v[:5], torch.full((1, 3), float('inf'), device=DEV)]))
    with pytest.raises(ValueError, match='eps'):
        weld.weld_mesh(v.cpu(), f, -1.0)                               # the parameter comes first
    with pytest.raises(weld.CpuTensorError, match='no CPU'):
        weld.weld_mesh(v.cpu(), f)
    with pytest.raises(weld.CpuTensorError, match='no CPU'):
        weld.weld_mesh(v, f.cpu(), 0.5)
    with pytest.raises(weld.CpuTensorError, match='no CPU'):
        weld.vertex_clusters(v.cpu())


@pytest.mark.parametrize('double', [False, True])
def test_the_command_welds_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import meshio, weld
    verts, faces, _ = S.case('sphere soup')
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
    for eps, drop in ((0.0, False), (1.0e-3, True)):
        report = weld.main([src, dst] + (['--eps', str(eps)] if eps else []) + (['--drop_duplicates'] if drop else []))
        assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
        _, want_f, want_info, parts = S.weld_spec(local, faces, eps, drop)
        assert {k: report[k] for k in want_info} == want_info and set(report) == set(want_info) | {'pairs_in', 'pairs_out', 'closed'}
        assert report['faces_invalid'] == 1 and report['faces_out'] == 1280 and report['pairs_in'] == 0 and report['pairs_out'] == 1920 and report['closed'] is True
        got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
        assert np.array_equal(got_f, want_f) and got_v.tobytes() == stored[parts['rows']].tobytes()
        assert np.array_equal(meshio.read_ply_vertex_colors(dst), rgb[parts['rows']])
        assert (b'property double x' in open(dst, 'rb').read(300)) == double
    assert report['vertices_out'] == 642


@pytest.mark.parametrize('ascii_', [False, True])
def test_the_command_turns_an_stl_into_a_closed_surface(tmp_path, capsys, ascii_):
    from ppsurf_amd import meshio, weld
    src, dst = str(tmp_path / 'tetra.stl'), str(tmp_path / 'out.ply')
    corners = S.tetra_stl(src, ascii_)
    report = weld.main([src, dst])
    assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
    assert report['vertices_in'] == 12 and report['vertices_out'] == 4 and report['faces_in'] == report['faces_out'] == 4
    assert report['pairs_in'] == 0 and report['pairs_out'] == 6 and report['closed'] is True and report['eps'] == 0.0
    got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
    want_v, want_f = spec('tetra soup', 0.0)[:2]
    assert got_v.shape == (4, 3) and np.array_equal(got_f, want_f) and np.array_equal(got_v, want_v.astype(np.float64)) and np.array_equal(got_v[got_f].reshape(12, 3), corners)
    assert meshio.read_ply_vertex_colors(dst) is None


def test_the_stages_that_did_nothing_on_a_soup_work_after_the_weld():
    from ppsurf_amd import decimate, orient, pieces, weld
    verts, faces, _ = S.case('sphere soup')                            # the scrambled sphere, every face on private corners
    v, f = dev(verts), dev(faces)
    nf = faces.shape[0]
    assert pieces.face_components(f, verts.shape[0]).cpu().numpy().tolist() == list(range(nf))          # one component per face
    assert orient.orient_mesh(v, f, 'outward')[2]['components_closed'] == 0
    assert decimate.decimate_mesh(v, f, nf // 2)[2]['collapses'] == 0
    out_v, out_f, info = weld.weld_mesh(v, f)
    nv = int(out_v.shape[0])
    assert nv == 642 and info['faces_out'] == nf
    assert bool((pieces.face_components(out_f, nv) == 0).all())                                         # one component
    ov, of, oinfo = orient.orient_mesh(out_v, out_f, 'outward')
    assert oinfo['components'] == oinfo['components_closed'] == 1 and oinfo['components_non_orientable'] == 0 and oinfo['faces_flipped'] > 0
    assert all(vol > 0 for vol in orient_spec.signed_volumes(ov.cpu().numpy(), of.cpu().numpy()).values())
    dv, df, dinfo = decimate.decimate_mesh(ov, of, nf // 2)
    assert dinfo['reached'] and int(df.shape[0]) <= nf // 2 and dinfo['collapses'] > 0
