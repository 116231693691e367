"""GPU tier of the manifold split: ppsurf_amd/manifold.py and the kernels of csrc/pps_manifold.hip against the numpy
specification tests/manifold_spec.py, byte for byte and twice; the hook alone between canary rows on pair lists with entries out of
range; the face kernel alone; the argument rules of the C entries; `python -m ppsurf_amd.manifold` end to end on a coloured PLY; and the
stages downstream -- orient, decimate's regular vertices -- before and after the split."""
import json

import numpy as np
import pytest
import torch

import manifold_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32, I64 = torch.int32, torch.int64
_cache = {}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


def spec(name):
    """(verts out, faces out, info, parts) of the specification on a named case, computed once."""
    if name not in _cache:
        _cache[name] = S.split_spec(*S.case(name))
    return _cache[name]


def guarded(n, dtype, fill, *tail):
    """(buffer [n + 2, ...] filled with `fill`, its rows 1 .. n): an output between two canary rows."""
    buf = torch.full((n + 2,) + tail, fill, dtype=dtype, device=DEV)
    return buf, buf[1:n + 1]


def untouched(buf, fill):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


@pytest.mark.parametrize('name', S.CASES)
def test_split_nonmanifold_and_corner_fans_match_the_spec_bytewise(name):
    from ppsurf_amd import manifold
    verts, faces = S.case(name)
    v, f = dev(verts), dev(faces)
    want_v, want_f, want_info, parts = spec(name)
    for _ in range(2):
        label = manifold.corner_fans(f, verts.shape[0])
        assert label.dtype == I32 and label.shape == (3 * faces.shape[0],) and label.cpu().numpy().tobytes() == parts['label'].tobytes()
        out_v, out_f, info, source = manifold.split_nonmanifold(v, f, return_source=True)
        assert info == want_info and json.loads(json.dumps(info)) == info, (info, want_info)
        assert out_v.dtype == torch.float32 and out_f.dtype == I64 and source.dtype == I64
        assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes()
        assert source.cpu().numpy().tobytes() == parts['source'].tobytes()
        assert (out_v is v) == parts['same'] and (out_f is f) == parts['same']
        assert len(manifold.split_nonmanifold(v, f)) == 3
    assert f.cpu().numpy().tobytes() == faces.tobytes() and v.cpu().numpy().tobytes() == verts.tobytes()          # the inputs are not written
    # no edge with three owners is left, and the device finds nothing to do on its own result
    nv_out = int(out_v.shape[0])
    again_v, again_f, again = manifold.split_nonmanifold(out_v, out_f)
    assert again_v is out_v and again_f is out_f and again['edges_nonmanifold_in'] == 0 and again['vertices_split'] == 0 and again['vertices_out'] == nv_out
    assert again['edges_border_in'] == info['edges_border_out'] and again['edges_manifold_in'] == info['edges_manifold_out']


def hook(f, nv, pairs, label, changed, np_=None):
    from ppsurf_amd import _lib
    fa, fb, ea, eb = pairs
    _lib.call('ppsx_manifold_hook', f, int(f.shape[0]), nv, fa, fb, ea, eb, int(fa.shape[0]) if np_ is None else np_, label, changed)


def fixed_point(f, nv, pairs, label):
    """The host loop of manifold._fans on a given pair list and given labels."""
    from ppsurf_amd import _lib
    changed = torch.zeros(1, dtype=I32, device=DEV)
    for rounds in range(1, 100):
        changed.zero_()
        hook(f, nv, pairs, label, changed)
        assert int(changed.item()) in (0, 1)
        if int(changed.item()) == 0:
            return rounds
        _lib.call('ppsx_labels_compress', label, int(label.shape[0]))
    raise AssertionError('no fixed point')


def labelled(faces, nv, pairs, start=None):
    """(labels at the fixed point of hook and compress alone, rounds): the labels between canary rows, the pairs as int32 on the device."""
    start = S.start_labels(faces, nv) if start is None else start
    f = dev(faces)
    on = tuple(dev(np.asarray(p).astype(np.int32)) for p in pairs)
    lbuf, label = guarded(3 * faces.shape[0], I32, -7)
    label.copy_(dev(start))
    rounds = fixed_point(f, nv, on, label)
    assert untouched(lbuf, -7)
    assert fixed_point(f, nv, on, label) == 1                          # a fixed point writes nothing and says so at once
    assert f.cpu().numpy().tobytes() == faces.tobytes()
    return label.cpu().numpy(), rounds


@pytest.mark.parametrize('npairs', [255, 256, 257])
def test_the_hook_alone_between_canary_rows(npairs):
    verts, faces = S.case('simplified torus 8 shuffled')
    nv, nf = verts.shape[0], faces.shape[0]
    full = S.pair_list(faces, nv)
    assert full[0].shape[0] == 410 > npairs
    pairs = tuple(p[:npairs] for p in full)
    got, rounds = labelled(faces, nv, pairs)
    want = S.fans_of_pairs(faces, nv, *pairs)
    assert got.tobytes() == want.tobytes() and rounds >= 2 and not np.array_equal(want, S.fans_spec(faces, nv))
    # the pairs in both owner orders, and every pair twice: the same fans
    fa, fb, ea, eb = pairs
    swapped = (np.concatenate([fb, fa, fa]), np.concatenate([fa, fb, fb]), np.concatenate([eb, ea, ea]), np.concatenate([ea, eb, eb]))
    assert labelled(faces, nv, swapped)[0].tobytes() == want.tobytes()
    # entries out of range, a slot of 3 and -1, a pair that names no common edge: skipped, never read through
    bad = [p.copy() for p in pairs]
    bad[0][[0, 1]] = [-1, nf]
    bad[1][[2, 3]] = [1 << 30, -(1 << 31)]
    bad[2][[4, 5]] = [3, -1]
    bad[3][[6, 7]] = [3, 1 << 30]
    bad[2][8] = (bad[2][8] + 1) % 3                                    # another slot of fa: not the edge fb names
    bad[1][9] = bad[0][9]                                              # fa paired with itself in another slot
    bad[3][9] = (bad[2][9] + 1) % 3
    keep = np.ones(npairs, dtype=bool)
    keep[:10] = False
    want_bad = S.fans_of_pairs(faces, nv, *(p[keep] for p in pairs))
    assert S.fans_of_pairs(faces, nv, *bad).tobytes() == want_bad.tobytes() and not np.array_equal(want_bad, want)
    assert labelled(faces, nv, bad)[0].tobytes() == want_bad.tobytes()
    # negative labels: their corners take no part and are never touched
    start = S.start_labels(faces, nv)
    out = np.unique(np.concatenate([3 * fa[:40:4] + ea[:40:4], 3 * fb[1:40:4] + (eb[1:40:4] + 1) % 3]))
    start[out] = np.resize(np.array([-1, -(1 << 31), -5, -2], dtype=np.int32), out.shape[0])
    want_neg = S.fans_of_pairs(faces, nv, *pairs, start=start)
    assert np.array_equal(want_neg[out], start[out]) and not np.array_equal(want_neg >= 0, want >= 0)
    assert labelled(faces, nv, pairs, start)[0].tobytes() == want_neg.tobytes()
    # vertex indices out of range in the faces the pairs point at (their labels left as they were): the pair is skipped
    broken = faces.copy()
    broken[fa[0], ea[0]] = nv
    broken[fb[1], (eb[1] + 1) % 3] = -1
    start = S.start_labels(faces, nv)
    want_broken = S.fans_of_pairs(broken, nv, *pairs, start=start)
    assert not np.array_equal(want_broken, want) and labelled(broken, nv, pairs, start)[0].tobytes() == want_broken.tobytes()
    assert labelled(faces, 0, pairs, start)[0].tobytes() == start.tobytes()          # no vertex: every pair is skipped


@pytest.mark.parametrize('order', ['ascending', 'reversed', 'permuted'])
def test_a_strip_of_1025_faces_takes_rounds(order):
    verts, faces = S.case('strip ' + order)
    got, rounds = labelled(faces, verts.shape[0], S.pair_list(faces, verts.shape[0]))
    assert got.tobytes() == spec('strip ' + order)[3]['label'].tobytes() and rounds >= 2
    assert int((got == np.arange(got.shape[0])).sum()) == verts.shape[0]                  # one fan per vertex


@pytest.mark.parametrize('nf', [255, 256, 257])
def test_the_face_kernel_alone(nf):
    from ppsurf_amd import _lib
    nv, nv_out = 100, 130
    rng = np.random.default_rng(nf)
    faces = rng.integers(0, nv, size=(nf, 3)).astype(np.int64)
    faces[::31] = [[-1, 2, 3]]
    faces[7::31, 2] = 1 << 40
    faces[9::31, 1] = nv
    label = rng.integers(0, 3 * nf, size=3 * nf).astype(np.int32)
    label[5::17] = -1                                                  # a corner that keeps its entry
    label[11::53] = -(1 << 31)
    label[3 * 20 + 1] = 3 * nf                                         # no corner: the face is copied
    label[3 * 40] = (1 << 31) - 1
    newrow = rng.integers(0, nv_out, size=3 * nf).astype(np.int64)
    newrow[label[[3 * 50, 3 * 60 + 2, 3 * 70 + 1]]] = [-1, nv_out, 1 << 40]          # entries out of range: their faces are copied
    want = S.faces_spec(faces, nv, label, newrow, nv_out)
    changed = (want != faces).any(axis=1)
    assert changed.sum() > nf // 2 and not changed[[0, 20, 31, 38, 40, 50, 60, 70]].any() and (want[changed] < nv_out).all() and (want[changed] >= nv).any()
    obuf, out = guarded(nf, I64, -7, 3)
    f, lab, rows = dev(faces), dev(label), dev(newrow)
    for _ in range(2):
        _lib.call('ppsx_manifold_faces', f, nf, nv, lab, rows, nv_out, out)
        assert out.cpu().numpy().tobytes() == want.tobytes() and untouched(obuf, -7)
    _lib.call('ppsx_manifold_faces', f, nf, 0, lab, rows, nv_out, out)          # no vertex: every face is invalid and copied
    assert out.cpu().numpy().tobytes() == faces.tobytes() and untouched(obuf, -7)
    _lib.call('ppsx_manifold_faces', f, nf, nv, lab, rows, 0, out)              # no row out: every face is copied
    assert out.cpu().numpy().tobytes() == faces.tobytes() and untouched(obuf, -7)
    assert f.cpu().numpy().tobytes() == faces.tobytes() and lab.cpu().numpy().tobytes() == label.tobytes()


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib, manifold
    verts, faces = S.case('simplified torus 8')
    nv, nf = verts.shape[0], faces.shape[0]
    f = dev(faces)
    fa, fb, ea, eb = (dev(p.astype(np.int32)) for p in S.pair_list(faces, nv))
    npairs = int(fa.shape[0])
    label0 = dev(S.start_labels(faces, nv))
    label = label0.clone()
    changed = torch.zeros(1, dtype=I32, device=DEV)
    newrow = torch.zeros(3 * nf, dtype=I64, device=DEV)
    out = torch.full((nf, 3), -7, dtype=I64, device=DEV)
    big, third = 2 ** 31, (2 ** 31 - 1) // 3 + 1

    def run(name, *args):
        rc = _lib.call(name, *args, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    def hook_(faces=f, nf=nf, nv=nv, fa=fa, fb=fb, ea=ea, eb=eb, np_=npairs, label=label, changed=changed):
        return run('ppsx_manifold_hook', faces, nf, nv, fa, fb, ea, eb, np_, label, changed)

    def faces_(faces=f, nf=nf, nv=nv, label=label, newrow=newrow, nv_out=nv, out=out):
        return run('ppsx_manifold_faces', faces, nf, nv, label, newrow, nv_out, out)

    for kw in (dict(nf=-1), dict(nv=-1), dict(np_=-1), dict(nf=big), dict(nv=big), dict(np_=big), dict(nf=third), dict(faces=None), dict(fa=None),
               dict(fb=None), dict(ea=None), dict(eb=None), dict(changed=None)):
        assert hook_(**kw) == 1, kw
        assert torch.equal(label, label0) and changed.item() == 0, kw
    assert hook_(label=None) == 1 and hook_(np_=0) == 0 and hook_(nf=0) == 0 and changed.item() == 0 and torch.equal(label, label0)
    assert hook_(np_=0, faces=None, fa=None, fb=None, ea=None, eb=None, label=None, changed=None) == 0
    assert hook_(nf=third - 1, np_=0) == 0 and hook_(nf=third, np_=0) == 1                    # the counts are checked before the work
    for kw in (dict(nf=-1), dict(nv=-1), dict(nv_out=-1), dict(nf=big), dict(nv=big), dict(nv_out=big), dict(nf=third), dict(faces=None),
               dict(label=None), dict(newrow=None), dict(faces=out)):
        assert faces_(**kw) == 1, kw
        assert bool((out == -7).all()), kw
    assert faces_(out=None) == 1 and faces_(nf=0) == 0 and faces_(nf=0, faces=None, label=None, newrow=None, out=None) == 0
    assert bool((out == -7).all())
    with pytest.raises(_lib.PpsError, match='ppsx_manifold_faces failed with status 1'):
        _lib.call('ppsx_manifold_faces', f, -1, nv, label, newrow, nv, out)
    # the good calls after the refused ones
    assert fixed_point(f, nv, (fa, fb, ea, eb), label) >= 2 and label.cpu().numpy().tobytes() == spec('simplified torus 8')[3]['label'].tobytes()
    parts = spec('simplified torus 8')[3]
    assert faces_(newrow=dev(parts['newrow']), nv_out=150) == 0 and out.cpu().numpy().tobytes() == spec('simplified torus 8')[1].tobytes()
    # the Python layer
    v = dev(verts)
    with pytest.raises(ValueError, match='non-finite'):
        manifold.split_nonmanifold(torch.cat([v[:5], torch.full((1, 3), float('nan'), device=DEV)]), f[:1])
    with pytest.raises(manifold.CpuTensorError, match='no CPU'):
        manifold.split_nonmanifold(v.cpu(), f)
    with pytest.raises(manifold.CpuTensorError, match='no CPU'):
        manifold.split_nonmanifold(v, f.cpu())
    with pytest.raises(manifold.CpuTensorError, match='no CPU'):
        manifold.corner_fans(f.cpu(), nv)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match='nv and the number of faces'):
            manifold.corner_fans(f, bad)


@pytest.mark.parametrize('double', [False, True])
def test_the_command_splits_a_coloured_ply(tmp_path, capsys, double):
    from ppsurf_amd import manifold, meshio
    verts, faces = S.case('simplified torus 8')
    faces = np.concatenate([faces[:101], [[0, 0, 1]], faces[101:]])      # a face with a repeated index (a PLY holds no index out of range)
    offset = np.array([5.0e5, -2.5e5, 120.0]) if double else np.array([10.0, -20.0, 5.0])
    verts = verts.astype(np.float64) + offset[None]
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    src, dst, dst2 = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply'), str(tmp_path / 'again.ply')
    meshio.write_ply_mesh_colored(src, verts, faces, rgb, double=double)
    stored, stored_f = meshio.read_ply_mesh(src, dtype=np.float64)
    assert np.array_equal(stored_f, faces)
    report = manifold.main([src, dst])
    assert json.loads(capsys.readouterr().out.strip().split('\n')[-1]) == report
    _, want_f, want_info, parts = S.split_spec(stored.astype(np.float32), faces)
    assert report == want_info and report['vertices_out'] == 150 and report['faces_in'] == 285 and report['faces_valid'] == 284
    assert report['edges_nonmanifold_in'] == 8 and report['edges_border_out'] == 32
    got_v, got_f = meshio.read_ply_mesh(dst, dtype=np.float64)
    assert np.array_equal(got_f, want_f) and got_v.tobytes() == stored[parts['source']].tobytes()          # the vertices as read, not the float32 copies
    assert np.array_equal(meshio.read_ply_vertex_colors(dst), rgb[parts['source']])                       # a new row has its source's colour
    assert (b'property double x' in open(dst, 'rb').read(300)) == double
    # the command on its own output: nothing to do, the file comes back
    again = manifold.main([dst, dst2])
    capsys.readouterr()
    assert again['vertices_split'] == 0 and again['vertices_out'] == 150 and again['edges_nonmanifold_in'] == 0
    assert meshio.read_ply_mesh(dst2, dtype=np.float64)[0].tobytes() == got_v.tobytes() and np.array_equal(meshio.read_ply_mesh(dst2, dtype=np.float64)[1], got_f)
    assert np.array_equal(meshio.read_ply_vertex_colors(dst2), rgb[parts['source']])


def regular_count(v, f):
    from ppsurf_amd import decimate
    return int(decimate._rows(f.contiguous(), int(v.shape[0]))['regular'].sum().item())


def test_the_stages_downstream_on_two_cubes_welded_along_an_edge():
    from ppsurf_amd import decimate, manifold, orient, pieces
    verts, faces = S.case('welded edge')
    v, f = dev(verts), dev(faces)
    assert orient.orient_mesh(v, f, 'outward')[2]['components_closed'] == 0 and regular_count(v, f) == 12
    assert decimate.decimate_mesh(v, f, 24)[2]['locked_vertices'] == 2
    out_v, out_f, info = manifold.split_nonmanifold(v, f)
    assert info['vertices_out'] == 16 and info['closed_out'] is True
    oinfo = orient.orient_mesh(out_v, out_f, 'outward')[2]
    assert oinfo['components'] == oinfo['components_closed'] == 2 and oinfo['components_non_orientable'] == 0
    assert regular_count(out_v, out_f) == 16 and decimate.decimate_mesh(out_v, out_f, 24)[2]['locked_vertices'] == 0
    assert pieces.face_components(out_f, 16).cpu().numpy().tolist() == [0] * 12 + [12] * 12


def test_the_regular_vertices_of_a_simplified_sphere_rise():
    from ppsurf_amd import manifold
    verts, faces = S.case('simplified sphere 6')
    v, f = dev(verts), dev(faces)
    assert verts.shape[0] == 132 and regular_count(v, f) == 129
    out_v, out_f, info = manifold.split_nonmanifold(v, f)
    assert info['vertices_out'] == 134 and info['edges_nonmanifold_in'] == 1 and regular_count(out_v, out_f) == 131
