"""The command frame of the mesh stages without a GPU (ppsurf_amd/mesh_cli.py): the record of the loader and the four writers, each file
byte for byte what the stage's own meshio.write_ply_mesh call wrote before the frame existed."""
import numpy as np
import pytest


def _mesh(double):
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((5, 3)) + np.array([1.0e6, -2.0e6, 3.0e6])          # a centre of the order of 1e6: the float64 add shows
    if not double:
        verts = verts.astype(np.float32).astype(np.float64)
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]], dtype=np.int32)              # as read_mesh_file returns them
    colors = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    return verts, faces, colors


def _load(monkeypatch, verts, faces, colors, double, prog='python -m ppsurf_amd.x'):
    from ppsurf_amd import _lib, mesh_cli, meshio
    seen = []
    monkeypatch.setattr(_lib, 'need_gpu', lambda p: seen.append(p))
    monkeypatch.setattr(meshio, 'read_mesh_file', lambda path: (verts, faces, colors, double))
    mesh = mesh_cli.load('in.ply', prog)
    assert seen == [prog]
    return mesh


@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('colored', [False, True])
def test_the_writers_write_the_bytes_of_the_direct_calls(tmp_path, monkeypatch, double, colored):
    from ppsurf_amd import meshio
    verts, faces, colors = _mesh(double)
    colors = colors if colored else None
    mesh = _load(monkeypatch, verts, faces, colors, double)
    centre = meshio.box_centre(verts)
    assert mesh.verts is verts and mesh.colors is colors and mesh.double is double and mesh.path == 'in.ply'
    assert mesh.faces.dtype == np.int64 and mesh.faces.shape == (3, 3) and np.array_equal(mesh.faces, faces)
    assert mesh.centre.dtype == np.float64 and np.array_equal(mesh.centre, centre)
    assert mesh.local32.dtype == np.float32 and np.array_equal(mesh.local32, meshio.centred_f32(verts, centre))

    def same(write, *direct, **kw):
        a, b = str(tmp_path / 'frame.ply'), str(tmp_path / 'direct.ply')
        write(a)
        meshio.write_ply_mesh(b, *direct, double=double, **kw)
        got, want = open(a, 'rb').read(), open(b, 'rb').read()
        assert got == want and len(got) > 100

    rng = np.random.default_rng(6)
    # as read: plain, with re-wound faces (orient), with normals (normals)
    same(lambda p: mesh.write_as_read(p), verts, faces, colors_u8=colors)
    turned = np.ascontiguousarray(mesh.faces[:, [0, 2, 1]])
    same(lambda p: mesh.write_as_read(p, faces=turned), verts, turned, colors_u8=colors)
    nrm = rng.standard_normal((5, 3)).astype(np.float32)
    same(lambda p: mesh.write_as_read(p, normals=nrm), verts, faces, normals=nrm, colors_u8=colors)
    # gathered through rows: a subset in ascending order (pieces, weld), source rows with repeats (manifold)
    for rows, out_f in ((np.array([0, 1, 3, 4]), np.array([[0, 1, 2], [2, 1, 3]])),
                        (np.array([0, 1, 2, 3, 4, 1, 1, 3]), np.array([[0, 1, 2], [2, 5, 3], [7, 6, 4]]))):
        same(lambda p: mesh.write_rows(p, rows, out_f), verts[rows], out_f, colors_u8=None if colors is None else np.asarray(colors)[rows])
    # moved: float32 positions of the centred frame put back on the centre in float64 (smooth, denoise)
    out_v = mesh.local32 + rng.standard_normal((5, 3)).astype(np.float32) * np.float32(0.01)
    same(lambda p: mesh.write_moved(p, out_v), out_v.astype(np.float64) + centre[None], faces, colors_u8=colors)
    if double:                                                            # the add is a float64 add: a float32 one would lose the move
        moved = out_v.astype(np.float64) + centre[None]
        assert not np.array_equal(moved, (out_v + centre.astype(np.float32)[None]).astype(np.float64))


@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('colored', [False, True])
def test_write_origin_writes_the_bytes_of_the_three_mains(tmp_path, monkeypatch, double, colored):
    """decimate, subdivide and remesh each wrote their result themselves before `write_origin`: restated here as the direct calls."""
    from ppsurf_amd import meshio
    verts, faces, colors = _mesh(double)
    colors = colors if colored else None
    mesh = _load(monkeypatch, verts, faces, colors, double)
    centre, local32 = mesh.centre, mesh.local32
    rng = np.random.default_rng(7)

    def same(origin, out_v, out_f, out_c, pos):
        a, b = str(tmp_path / 'frame.ply'), str(tmp_path / 'direct.ply')
        before = origin.copy()
        mesh.write_origin(a, origin, out_v, out_f, out_c)
        meshio.write_ply_mesh(b, pos, out_f, double=double, colors_u8=out_c)
        got, want = open(a, 'rb').read(), open(b, 'rb').read()
        assert got == want and len(got) > 100 and np.array_equal(origin, before)

    def ulp(x):
        return np.nextafter(x, np.float32(np.inf))

    # decimate: a subset in ascending order; row 1 of it moved by one ulp in one coordinate, the others not at all
    kept, out_f = np.array([0, 1, 3, 4]), np.array([[0, 1, 2], [2, 1, 3]])
    out_v = local32[kept].copy()
    out_v[1, 2] = ulp(out_v[1, 2])
    moved = (out_v.view(np.int32) != local32[kept].view(np.int32)).any(axis=1)
    assert moved.tolist() == [False, True, False, False]
    pos = np.asarray(verts, dtype=np.float64)[kept]
    pos[moved] = out_v[moved].astype(np.float64) + centre[None]
    same(kept, out_v, out_f, None if colors is None else np.asarray(colors)[kept], pos)
    assert np.array_equal(pos[0], verts[0]) and not np.array_equal(pos[1], verts[1])
    # subdivide: every row kept with its bytes, two appended
    new = rng.standard_normal((2, 3)).astype(np.float32)
    out_v, out_f = np.concatenate([local32, new]), np.array([[0, 1, 5], [5, 1, 2], [2, 1, 6], [6, 1, 3], [3, 1, 4]])
    out_c = None if colors is None else np.concatenate([colors, rng.integers(0, 256, (2, 3)).astype(np.uint8)])
    same(np.concatenate([np.arange(5, dtype=np.int64), np.full(2, -1, dtype=np.int64)]), out_v, out_f, out_c,
         np.concatenate([verts, new.astype(np.float64) + centre[None]]))
    # remesh: a permuted subset with new rows between; row 0 of the file moved, rows 3, 4 and 1 not
    origin, out_f = np.array([3, -1, 0, 4, -1, 1], dtype=np.int64), np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5]])
    out_v = np.stack([local32[3], new[0], local32[0], local32[4], new[1], local32[1]])
    out_v[2, 0] = ulp(out_v[2, 0])
    pos = np.stack([verts[o] if o >= 0 and out_v[i].tobytes() == local32[o].tobytes() else out_v[i].astype(np.float64) + centre
                    for i, o in enumerate(origin)])
    assert [bool(np.array_equal(pos[i], verts[o])) for i, o in enumerate(origin)] == [True, False, False, True, False, True]
    same(origin, out_v, out_f, None if colors is None else rng.integers(0, 256, (6, 3)).astype(np.uint8), pos)


def test_the_loader_checks_the_gpu_first_and_refuses_non_finite_vertices(monkeypatch):
    from ppsurf_amd import _lib, mesh_cli, meshio
    verts, faces, colors = _mesh(False)
    order = []
    monkeypatch.setattr(_lib, 'need_gpu', lambda prog: order.append(('need_gpu', prog)))

    def reader(path):
        order.append(('read', path))
        return verts, faces, colors, False

    mesh = mesh_cli.load('some/mesh.obj', 'python -m ppsurf_amd.weld', reader=reader)                  # weld's reader, for one
    assert order == [('need_gpu', 'python -m ppsurf_amd.weld'), ('read', 'some/mesh.obj')] and mesh.colors is colors
    for bad in (np.nan, np.inf, -np.inf):
        broken = verts.copy()
        broken[3, 1] = bad
        monkeypatch.setattr(meshio, 'read_mesh_file', lambda path: (broken, faces, None, False))
        with pytest.raises(SystemExit) as e:
            mesh_cli.load('bad.ply', 'python -m ppsurf_amd.smooth')
        assert str(e.value) == 'bad.ply has non-finite vertices'
    # an empty mesh loads: the centre is the origin
    monkeypatch.setattr(meshio, 'read_mesh_file', lambda path: (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), None, False))
    empty = mesh_cli.load('empty.ply', 'python -m ppsurf_amd.fill')
    assert empty.faces.shape == (0, 3) and empty.local32.shape == (0, 3) and np.array_equal(empty.centre, np.zeros(3))
