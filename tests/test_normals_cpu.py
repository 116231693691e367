"""CPU tier of the oriented normals: hand-checked cases and properties of the numpy specification
tests/normals_spec.py, the argument rules of `vertex_normals` / `point_normals`, the models' `gen_normals`, the command's argument errors, the
two PLY writers and the extension entries of the C ABI."""
import ctypes
import inspect

import numpy as np
import pytest

import eval_spec
import normals_spec as N
import call_sites

TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32)
FACE = np.array([[0, 1, 2]], dtype=np.int64)
TET_V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], dtype=np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int64)


def test_a_single_triangle_has_its_face_normal_three_times():
    assert N.corner_keys(FACE, 3).tolist() == [0, 1 << 32, 2 << 32]
    offsets, inc = N.incidence(FACE, 3)
    assert offsets.tolist() == [0, 1, 2, 3] and inc.tolist() == [0, 0, 0]
    for weight in N.WEIGHTS:
        got = N.vertex_normals(TRI, FACE, weight)
        assert got.dtype == np.float32 and got.tolist() == [[0, 0, 1]] * 3
        assert N.vertex_normals(TRI, FACE[:, ::-1], weight).tolist() == [[0, 0, -1]] * 3          # the winding decides the side
    # the sums before the normalisation: twice the area, and twice the area over |e1|^2 |e2|^2
    assert N.accumulate(TRI, FACE, 'area').tolist() == [[0, 0, 16]] * 3
    assert N.accumulate(TRI, FACE, 'max').tolist() == [[0, 0, 16 / 256], [0, 0, 16 / 512], [0, 0, 16 / 512]]


def test_a_closed_tetrahedron():
    offsets, inc = N.incidence(TET_F, 4)
    assert np.diff(offsets).tolist() == [3] * 4 and inc.tolist() == [0, 1, 3, 0, 1, 2, 0, 2, 3, 1, 2, 3]
    # area weights: the three axis faces (16 each) and the slanted one (16, 16, 16) -- at the origin's corner the three axis faces, at the
    # others two axis faces and the slanted face, whose sum is the corner's own axis
    assert N.accumulate(TET_V, TET_F, 'area').tolist() == [[-16, -16, -16], [16, 0, 0], [0, 16, 0], [0, 0, 16]]
    s = np.float32(np.float64(16.0) / np.sqrt(np.float64(768.0)))
    assert N.vertex_normals(TET_V, TET_F, 'area').tolist() == [[-s, -s, -s], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    # Max's weights: 1 / 256 at the origin, 1 / 512 for the axis faces and 1 / 1024 for the slanted face at the other corners
    assert N.accumulate(TET_V, TET_F, 'max').tolist() == [[-1 / 16] * 3, [1 / 64, -1 / 64, -1 / 64], [-1 / 64, 1 / 64, -1 / 64], [-1 / 64, -1 / 64, 1 / 64]]
    assert N.vertex_normals(TET_V, TET_F, 'max').tolist() == [[-s, -s, -s], [s, -s, -s], [-s, s, -s], [-s, -s, s]]
    assert np.all(np.einsum('ij,ij->i', N.vertex_normals(TET_V, TET_F, 'max'), TET_V - TET_V.mean(axis=0)) > 0)          # outward


def test_unreferenced_vertices_and_those_of_invalid_faces_are_zero():
    verts = np.concatenate([TRI, np.array([[7, 7, 7], [-0.0, 1e-30, 3], [5, 5, 5], [6, 6, 6], [8, 8, 9]], dtype=np.float32)])
    faces = np.array([[0, 1, 2], [3, 4, -1], [4, 5, 8], [5, 6, 6], [7, 7, 7], [1 << 40, 5, 6], [0, 1, (1 << 32) + 2]], dtype=np.int64)
    assert N.valid_faces(faces, 8).tolist() == [True] + [False] * 6
    keys = N.corner_keys(faces, 8)
    assert (keys[3:] == N.SENTINEL).all() and keys[:3].tolist() == [0, 1 << 32, 2 << 32]
    for weight in N.WEIGHTS:
        got = N.vertex_normals(verts, faces, weight)
        assert got[:3].tolist() == [[0, 0, 1]] * 3 and got[3:].tobytes() == bytes(60)
        assert N.vertex_info(verts, faces, weight) == {'vertices': 8, 'faces_valid': 1, 'zero_normals': 5, 'weight': weight}
        assert N.vertex_normals(np.zeros((0, 3), np.float32), faces, weight).shape == (0, 3)
        assert N.vertex_normals(verts, np.zeros((0, 3), np.int64), weight).tobytes() == bytes(96)


def test_duplicated_cancelling_and_degenerate_faces():
    sq = np.array([[0, 0, 0], [4, 0, 0], [4, 4, 1], [0, 4, 0]], dtype=np.float32)
    two = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    dup = np.concatenate([two, two[:1]])
    offsets, inc = N.incidence(dup, 4)
    assert inc[offsets[0]:offsets[1]].tolist() == [0, 1, 2] and inc[offsets[1]:offsets[2]].tolist() == [0, 2]          # the duplicate is a face
    g0, g1 = np.array([0.0, -4.0, 16.0]), np.array([-4.0, 0.0, 16.0])          # (4,0,0) x (4,4,1) and (4,4,1) x (0,4,0)
    assert N.accumulate(sq, two, 'area')[0].tolist() == (g0 + g1).tolist()
    assert N.accumulate(sq, dup, 'area')[0].tolist() == (g0 + g1 + g0).tolist()          # counted twice
    assert N.accumulate(sq, dup, 'area')[1].tolist() == (2 * N.accumulate(sq, two, 'area')[1]).tolist()
    # two coincident faces of opposite winding: exact zeros, not a rounding residue
    both = np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64)
    verts, _ = N.noisy_sphere(0)
    for weight in N.WEIGHTS:
        assert N.accumulate(verts, both, weight).tobytes() == bytes(12 * 24) and N.vertex_normals(verts, both, weight).tobytes() == bytes(12 * 12)
        assert N.vertex_info(verts, both, weight)['zero_normals'] == 12
    # a face with two corners at the same POSITION (distinct indices: the face is valid): at the doubled corners one edge has length 0, so
    # d = 0 and the face adds nothing under 'max'; under 'area' it adds its zero cross product
    twin = np.array([[0, 0, 0], [4, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32)
    flat = np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int64)
    assert N.valid_faces(flat, 4).all()
    assert N.accumulate(twin, flat[:1], 'max').tobytes() == bytes(4 * 24) and N.accumulate(twin, flat[:1], 'area').tobytes() == bytes(4 * 24)
    assert N.vertex_normals(twin, flat, 'max').tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1]]
    assert N.vertex_normals(twin, flat, 'area').tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1]]


def test_reversed_winding_negates_every_normal_exactly():
    verts, faces = N.noisy_sphere(3)
    for weight in N.WEIGHTS:
        a, b = N.vertex_normals(verts, faces, weight), N.vertex_normals(verts, faces[:, ::-1], weight)
        assert np.array_equal(b, -a) and a.any(axis=1).all()
        c = N.vertex_normals(verts, faces[:, [1, 2, 0]], weight)          # a rotated face is the same face: the same corners follow i
        assert c.tobytes() == a.tobytes()


def test_the_open_fan_lists_the_hubs_faces_in_ascending_order():
    verts, faces = N.fan(300)
    assert verts.shape == (301, 3) and faces.shape == (300, 3)
    perm = np.random.default_rng(2).permutation(300)
    for fs in (faces, faces[perm]):
        offsets, inc = N.incidence(fs, 301)
        assert inc[offsets[0]:offsets[1]].tolist() == list(range(300)) and np.diff(offsets)[1:].tolist() == [2] * 300
    # the hub's sum runs in that order: the hand-written loop
    x = verts.astype(np.float64)
    acc = np.zeros(3)
    for t in range(300):
        a, b, c = faces[t]
        assert a == 0
        acc = acc + np.array([(x[b] - x[0])[1] * (x[c] - x[0])[2] - (x[b] - x[0])[2] * (x[c] - x[0])[1],
                              (x[b] - x[0])[2] * (x[c] - x[0])[0] - (x[b] - x[0])[0] * (x[c] - x[0])[2],
                              (x[b] - x[0])[0] * (x[c] - x[0])[1] - (x[b] - x[0])[1] * (x[c] - x[0])[0]])
    assert np.array_equal(N.accumulate(verts, faces, 'area')[0], acc)
    assert N.vertex_normals(verts, faces, 'area')[0, 2] > 0.99
    cv, cf = N.fan(300, closed=True)
    assert np.diff(N.incidence(cf, 302)[0]).tolist() == [300] + [4] * 300 + [300]


def test_quality_on_spheres():
    """Measured with this specification: on icosphere(3) projected to the unit sphere (float32 vertices) the largest angle to the radial
    direction is 0.6769 degrees with 'area' and 1.23e-05 degrees with 'max' (Max's weights are exact for vertices on a sphere; what is left
    is the float32 rounding of the vertices and of the result).  On noisy_sphere(3): |len - 1| at most 4.19e-08 ('area') / 3.91e-08 ('max'),
    the smallest n . v 0.918 / 0.921.  The angle bounds are 1.5 x the measured values."""
    iv, faces = eval_spec.icosphere(3)
    radial = iv / np.linalg.norm(iv, axis=1)[:, None]
    worst = {w: float(N.angle_deg(N.vertex_normals(iv.astype(np.float32), faces, w), radial).max()) for w in N.WEIGHTS}
    print('icosphere(3): largest angle to the radius, degrees: {}'.format(worst))
    assert worst['max'] < worst['area']
    assert worst['area'] <= 1.5 * 0.6769 and worst['max'] <= 1.5 * 1.23e-05
    verts, faces = N.noisy_sphere(3)
    for weight in N.WEIGHTS:
        n = N.vertex_normals(verts, faces, weight).astype(np.float64)
        length, dots = np.linalg.norm(n, axis=1), np.einsum('ij,ij->i', n, verts.astype(np.float64))
        print('noisy_sphere(3) {}: |len - 1| <= {:.3e}, n . v >= {:.4f}'.format(weight, np.abs(length - 1).max(), dots.min()))
        assert np.all(np.abs(length - 1.0) <= 1e-7) and np.all(dots > 0)


def test_the_blend_of_eight_vertices_beats_the_nearest_vertex():
    """Measured with this specification: 500 seeded points within 1 % of the unit sphere against icosphere(3) (float32), 'area' normals: the
    mean angle to the radial direction is 0.977 degrees at k = 8 and 3.064 degrees at k = 1 ('max': 0.987 / 3.061).  Bound: 1.5 x."""
    iv, faces = eval_spec.icosphere(3)
    rng = np.random.default_rng(1)
    p = rng.standard_normal((500, 3))
    u = p / np.linalg.norm(p, axis=1)[:, None]
    pts = (u * (1.0 + 0.01 * rng.standard_normal(500))[:, None]).astype(np.float32)
    for weight, bound in (('area', 1.5 * 0.977), ('max', 1.5 * 0.987)):
        mean = {k: float(N.angle_deg(N.point_normals(pts, iv.astype(np.float32), faces, k, weight), u).mean()) for k in (1, 8)}
        print('{}: mean angle to the radius, degrees: {}'.format(weight, mean))
        assert mean[8] < mean[1] and mean[8] <= bound
        assert N.point_info(pts, iv.astype(np.float32), faces, 8, weight) == {'points': 500, 'vertices': 642, 'k': 8, 'zero_normals': 0, 'weight': weight}


def test_the_blend_spec_on_hand_made_rows():
    nrm = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, 0, 0]], dtype=np.float32)
    idx = np.array([[0, 1], [-1, 2], [5, 1 << 40], [0, 3], [1, 0], [4, 4], [3, 0]], dtype=np.int64)
    d2 = np.array([[0.25, 0.25], [0.0, 1.0], [0.0, 0.0], [0.5, 0.5], [0.0, 4.0], [1.0, 1.0], [0.0, 0.0]], dtype=np.float32)
    out = N.blend(idx, d2, nrm)
    h = np.float32(np.float64(4.0) / np.sqrt(np.float64(32.0)))
    assert out.dtype == np.float32 and out[0].tolist() == [0, h, h]                  # equal weights
    assert out[1].tolist() == [1, 0, 0]                                              # the invalid entry is skipped although its d2 is 0
    assert out[2].tolist() == [0, 0, 0]                                              # no valid neighbour
    assert out[3].tolist() == [0, 0, 0]                                              # opposite normals at equal distance cancel exactly
    assert out[4].tolist() == [0, 1, np.float32(0.25 / (1.0 / 1e-30))]               # an exact hit weighs 1e30 against 0.25: 2.5e-31 is left of the other
    assert out[5].tolist() == [0, 0, 0] and out[6].tolist() == [0, 0, 0]             # zero normals; two exact hits that cancel
    assert N.blend(idx[:, :1], d2[:, :1], nrm)[[0, 3, 4, 6]].tolist() == nrm[[0, 0, 1, 3]].tolist()          # k = 1: the nearest vertex's normal
    tv = TET_V + np.float32(0.25)
    assert N.point_normals(tv[1:2], TET_V, TET_F, 1, 'area').tolist() == [[1, 0, 0]]
    assert N.point_normals(tv, TET_V, TET_F, 8, 'area').shape == (4, 3)              # k is cut to the 4 vertices
    assert N.point_normals(tv[:0], TET_V, TET_F).shape == (0, 3)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_rules_of_the_python_functions():
    import torch
    from ppsurf_amd import normals
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in ('angle', 'AREA', None, 0, b'area'):
        with pytest.raises(ValueError, match='weight'):
            normals.vertex_normals(v, f, bad)
        with pytest.raises(ValueError, match='weight'):
            normals.point_normals(v, v, f, weight=bad)
    for bad in (0, -1, 257, 2.5, '8', None, True):
        with pytest.raises(ValueError, match='k must be'):
            normals.point_normals(v, v, f, k=bad)
    assert normals._checked_k(np.int64(256)) == 256 and normals._checked_k(1) == 1 and normals.WEIGHTS == {'area': 0, 'max': 1}
    # good scalars, CPU tensors: the device guard of the other modules
    for fn in (lambda: normals.vertex_normals(v, f), lambda: normals.point_normals(v, v, f, k=1, weight='max'), lambda: normals.vertex_incidence(f, 3),
               lambda: normals.blend_normals(torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1), v)):
        with pytest.raises(PpsError, match='no CPU'):
            fn()
    with pytest.raises(ValueError, match='vertex_normals: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        normals.vertex_normals(v, f)                                   # a ValueError like the other argument errors, with the guard's message


def test_models_take_gen_normals():
    from source.poco_model import PocoModel
    from source.ppsurf_model import PPSurfModel
    kw = dict(output_names=['imp_surf_sign'], in_channels=3, out_channels=2, k=64, lambda_l1=0.0, debug=False,
              in_file='datasets/abc_minimal/testset.txt', results_dir='results', padding_factor=0.05, name='m', network_latent_size=32,
              gen_subsample_manifold_iter=10, gen_subsample_manifold=10000, gen_resolution_global=129, rec_batch_size=25000, gen_refine_iter=10,
              workers=0)
    pps = dict(kw, pointnet_latent_size=32, num_pts_local=50)
    for model in (PocoModel(**kw), PPSurfModel(**pps)):
        assert model.gen_normals is None and model.last_normals is None
    assert PocoModel(gen_normals='area', **kw).gen_normals == 'area' and PPSurfModel(gen_normals='max', **pps).gen_normals == 'max'
    m = PPSurfModel(gen_normals='max', gen_smooth_iters='3', gen_trim_factor=2, gen_max_faces=100, gen_color_k=4, **pps)
    assert (m.gen_normals, m.gen_smooth_iters, m.gen_trim_factor, m.gen_max_faces, m.gen_color_k) == ('max', 3, 2.0, 100, 4)
    for bad in ('angle', 'Area', '', 0, 1, True, 0.5):
        with pytest.raises(ValueError, match='gen_normals'):
            PocoModel(gen_normals=bad, **kw)
        with pytest.raises(ValueError, match='gen_normals'):
            PPSurfModel(gen_normals=bad, **pps)
    for cls in (PocoModel, PPSurfModel):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[-5:] == ['gen_max_faces', 'gen_color_k', 'gen_normals', 'gen_trim_factor', 'gen_smooth_iters']
        assert params['gen_normals'].default is None


@pytest.mark.parametrize('argv', [['m.ply'], [], ['m.ply', 'o.obj'], ['m.ply', 'o'], ['m.ply', 'o.ply', '--weight', 'angle'],
                                  ['m.ply', 'o.ply', '--weight'], ['m.ply', 'o.ply', '--points', 's.ply'], ['m.ply', 'o.ply', '--points_out', 's.ply'],
                                  ['m.ply', 'o.ply', '--points', 's.ply', '--points_out', 's.xyz'], ['m.ply', 'o.ply', '--k', '0'],
                                  ['m.ply', 'o.ply', '--k', '257'], ['m.ply', 'o.ply', '--k', '2.5'], ['m.ply', 'o.ply', '--iters', '2']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import normals
    with pytest.raises(SystemExit) as e:
        normals.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_normals_entries_are_declared_and_every_call_site_has_their_argument_count():
    from ppsurf_amd import _lib, build
    I, I64, P, D = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_normals_corner_keys'] == (I, [P, I64, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_normals_vertex'] == (I, [P, I64, P, I64, P, P, I64, I, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_normals_blend'] == (I, [P, P, I64, I, P, I64, D, P, P])
    assert _lib.EXT_PARAMS['ppsx_normals_corner_keys'] == ['faces', 'nf', 'nv', 'keys', 'stream']
    assert _lib.EXT_PARAMS['ppsx_normals_vertex'] == ['verts', 'nv', 'faces', 'nf', 'offsets', 'inc', 'ni', 'weight', 'out', 'stream']
    assert _lib.EXT_PARAMS['ppsx_normals_blend'] == ['idx', 'd2', 'm', 'k', 'normals', 'nv', 'eps', 'out', 'stream']
    assert not any(n.startswith('pps_normals') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_normals')                    # every ppsurf_amd/*.py: the key entries are called from topology.py
    for name, where in sites.items():
        for path, line, nargs in where:
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    seen = {name: len(where) for name, where in sites.items()}
    assert seen == {'ppsx_normals_corner_keys': 1, 'ppsx_normals_vertex': 1, 'ppsx_normals_blend': 1}
    assert 'pps_normals.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and {'ppsx_normals_corner_keys', 'ppsx_normals_vertex', 'ppsx_normals_blend'} <= set(_lib._ext_entries)


# ---- the writers -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('double', [False, True])
def test_the_writers_round_trip(tmp_path, double):
    from ppsurf_amd import meshio
    verts, faces = N.noisy_sphere(1)
    verts = verts.astype(np.float64) * 3.0 + (np.array([5.0e5, -2.5e5, 120.0]) if double else np.zeros(3))
    nrm = N.vertex_normals(verts - verts.mean(axis=0), faces, 'max')
    rgb = np.random.default_rng(5).integers(0, 256, size=(verts.shape[0], 3)).astype(np.uint8)
    kept = verts if double else verts.astype(np.float32).astype(np.float64)
    plain, coloured, cloud = str(tmp_path / 'n.ply'), str(tmp_path / 'nc.ply'), str(tmp_path / 'p.ply')
    meshio.write_ply_mesh_normals(plain, verts, faces, nrm, double=double)
    meshio.write_ply_mesh_normals(coloured, verts, faces, nrm, colors_u8=rgb, double=double)
    meshio.write_ply_points_normals(cloud, verts, nrm, double=double)
    for path, has_faces, has_colours in ((plain, True, False), (coloured, True, True), (cloud, False, False)):
        head = open(path, 'rb').read(600).split(b'end_header')[0].decode('ascii')
        props = [line.split()[1:] for line in head.split('\n') if line.startswith('property') and 'list' not in line]
        pos = 'double' if double else 'float'
        assert props == [[pos, a] for a in 'xyz'] + [['float', a] for a in ('nx', 'ny', 'nz')] + (
            [['uchar', a] for a in ('red', 'green', 'blue', 'alpha')] if has_colours else [])
        got = meshio.read_ply_vertices(path)
        assert got.shape == (verts.shape[0], 6) and np.array_equal(got[:, :3], kept) and got[:, 3:].astype(np.float32).tobytes() == nrm.tobytes()
        v, f = meshio.read_ply_mesh(path, dtype=np.float64)
        assert np.array_equal(v, kept) and np.array_equal(f, faces if has_faces else np.zeros((0, 3)))
        colours = meshio.read_ply_vertex_colors(path)
        assert np.array_equal(colours, rgb) if has_colours else colours is None
        assert np.array_equal(meshio.load_pts(path), got)
    # an rgba array keeps its alpha
    rgba = np.concatenate([rgb, np.full((rgb.shape[0], 1), 7, dtype=np.uint8)], axis=1)
    meshio.write_ply_mesh_normals(coloured, verts, faces, nrm, colors_u8=rgba, double=double)
    assert np.array_equal(meshio.read_ply_vertex_colors(coloured), rgb)
    assert np.array_equal(meshio._ply_vertex_columns(coloured)['alpha'], rgba[:, 3])


def test_the_existing_writers_still_produce_the_same_bytes(tmp_path):
    """Every public writer against bytes laid out by hand from the published format: write_ply_mesh / write_ply_mesh_colored /
    write_ply_points, and the two normals writers, float and double, write_ply_mesh_normals with and without colours."""
    from ppsurf_amd import meshio
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0.5]], dtype=np.float64)
    faces = np.array([[0, 1, 2]], dtype=np.int64)
    rgb = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.uint8)
    nrm = np.array([[0, 0, 1], [0.6, 0, -0.8], [0.1, -0.25, 0.5]], dtype=np.float64)
    normal_props = 'property float nx\nproperty float ny\nproperty float nz\n'
    no_faces = 'element face 0\nproperty list uchar int vertex_indices\nend_header\n'
    face_bytes = b'\x03' + np.array([0, 1, 2], dtype='<i4').tobytes()
    for double in (False, True):
        ftype, name = ('<f8', 'double') if double else ('<f4', 'float')
        head = 'ply\nformat binary_little_endian 1.0\ncomment ppsurf_amd\nelement vertex 3\nproperty {0} x\nproperty {0} y\nproperty {0} z\n'.format(name)
        tail = 'element face 1\nproperty list uchar int vertex_indices\nend_header\n'
        path = str(tmp_path / 'm.ply')
        meshio.write_ply_mesh(path, verts, faces, double=double)
        assert open(path, 'rb').read() == (head + tail).encode('ascii') + verts.astype(ftype).tobytes() + face_bytes
        meshio.write_ply_mesh_colored(path, verts, faces, rgb, double=double)
        rows = b''.join(verts[i].astype(ftype).tobytes() + rgb[i].tobytes() + b'\xff' for i in range(3))
        colour_props = 'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n'
        assert open(path, 'rb').read() == (head + colour_props + tail).encode('ascii') + rows + face_bytes
        meshio.write_ply_mesh_normals(path, verts, faces, nrm, double=double)
        rows = b''.join(verts[i].astype(ftype).tobytes() + nrm[i].astype('<f4').tobytes() for i in range(3))
        assert open(path, 'rb').read() == (head + normal_props + tail).encode('ascii') + rows + face_bytes
        meshio.write_ply_mesh_normals(path, verts, faces, nrm, colors_u8=rgb, double=double)
        rows = b''.join(verts[i].astype(ftype).tobytes() + nrm[i].astype('<f4').tobytes() + rgb[i].tobytes() + b'\xff' for i in range(3))
        assert open(path, 'rb').read() == (head + normal_props + colour_props + tail).encode('ascii') + rows + face_bytes
        general = str(tmp_path / 'g.ply')                                # the general form writes the same file
        meshio.write_ply_mesh(general, verts, faces, double=double, normals=nrm, colors_u8=rgb)
        assert open(general, 'rb').read() == open(path, 'rb').read()
        meshio.write_ply_points_normals(path, verts, nrm, double=double)
        rows = b''.join(verts[i].astype(ftype).tobytes() + nrm[i].astype('<f4').tobytes() for i in range(3))
        assert open(path, 'rb').read() == (head + normal_props + no_faces).encode('ascii') + rows
    meshio.write_ply_points(path, verts)
    head = 'ply\nformat binary_little_endian 1.0\ncomment ppsurf_amd\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
    assert open(path, 'rb').read() == (head + 'element face 0\nproperty list uchar int vertex_indices\nend_header\n').encode('ascii') + verts.astype('<f4').tobytes()
