"""CPU tier of the feature-preserving denoising: the numpy specification tests/denoise_spec.py against values written
out by hand and against plain scalar loops, what it does to a noisy cube (against Taubin's filter too), its edge cases, the argument rules
of `denoise_mesh` and of the command, and the extension entries of the C ABI."""
import ctypes
import math

import numpy as np
import pytest

import call_sites
import denoise_spec as S
import smooth_spec

# a tent: two roof faces over the ridge 1-2, unit normals (-0.6, 0, 0.8) and (0.6, 0, 0.8) (cross products (-3, 0, 4) and (3, 0, 4))
TENT_V = np.array([[0, 0, 0], [4, 0, 3], [4, 1, 3], [8, 0, 0]], dtype=np.float32)
TENT_F = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int64)
# a pyramid: four faces around the apex 0, unit normals (+-0.6, 0, 0.8) and (0, +-0.6, 0.8) (cross products (24, 0, 32), ...)
PYR_V = np.array([[0, 0, 3], [4, -4, 0], [4, 4, 0], [-4, 4, 0], [-4, -4, 0]], dtype=np.float32)
PYR_F = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], dtype=np.int64)


def dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def loop_filter_pass(normals, neighbours, T):
    """The normal pass in plain Python floats: normals a list of [x, y, z], neighbours[i] the ascending list N(i)."""
    out = []
    for i, n in enumerate(normals):
        acc = [0.0, 0.0, 0.0]
        for j in neighbours[i]:
            d = dot(n, normals[j])
            if d > T:
                w = (d - T) * (d - T)
                acc = [acc[c] + w * normals[j][c] for c in range(3)]
        L = math.sqrt(dot(acc, acc))
        out.append([acc[c] / L for c in range(3)] if L > 0 and math.isfinite(L) else list(n))
    return out


def loop_vertex_pass(x, faces, normals, rows):
    """The vertex pass in plain Python floats: rows[v] the ascending list of the valid faces of vertex v."""
    out = []
    for v, xv in enumerate(x):
        acc = [0.0, 0.0, 0.0]
        for k in rows[v]:
            a, b, c = faces[k]
            ck = [((x[a][q] + x[b][q]) + x[c][q]) / 3.0 for q in range(3)]
            t = dot(normals[k], [ck[q] - xv[q] for q in range(3)])
            acc = [acc[q] + normals[k][q] * t for q in range(3)]
        out.append([xv[q] + acc[q] / float(len(rows[v])) for q in range(3)] if rows[v] else list(xv))
    return out


def test_the_tent_by_hand():
    n = S.face_normals(TENT_V, TENT_F)
    assert n.dtype == np.float64 and n.tolist() == [[-0.6, 0.0, 0.8], [0.6, 0.0, 0.8]]
    offsets, nb = S.neighbourhoods(TENT_F, 4)
    assert offsets.tolist() == [0, 2, 4] and nb.tolist() == [0, 1, 0, 1]
    # T = 0.5: the two normals have d = -0.36 + 0.64 = 0.28 <= T, so the pair contributes nothing; each face sums itself alone with
    # w = (1 - 0.5)^2 = 0.25 (0.36 + 0.64 is 1.0 exactly in fp64) and gets its own normal back, up to the rounding of acc / L
    assert dot(n[0], n[1]) < 0.5 and dot(n[0], n[0]) == 1.0
    acc = [0.25 * -0.6, 0.25 * 0.0, 0.25 * 0.8]
    L = math.sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2])
    got = S.filter_pass(n, offsets, nb, 0.5)
    assert got[0].tolist() == [acc[0] / L, acc[1] / L, acc[2] / L] and got[1].tolist() == [-acc[0] / L, acc[1] / L, acc[2] / L]
    assert np.allclose(got, n, rtol=0, atol=1e-15)
    assert S.filtered_normals_spec(TENT_V, TENT_F, 0.5, 5).tolist() == loop_filter_pass(loop_filter_pass(loop_filter_pass(loop_filter_pass(
        loop_filter_pass(n.tolist(), [[0, 1], [0, 1]], 0.5), [[0, 1], [0, 1]], 0.5), [[0, 1], [0, 1]], 0.5), [[0, 1], [0, 1]], 0.5), [[0, 1], [0, 1]], 0.5)
    # T = 0: d = 0.28 > 0, w = 0.28^2; face 0 sums itself first and face 1 second, face 1 sums face 0 first
    d = (-0.6 * 0.6 + 0.0 * 0.0) + 0.8 * 0.8
    w = (d - 0.0) * (d - 0.0)
    acc0 = [0.0 + 1.0 * -0.6 + w * 0.6, 0.0, 0.0 + 1.0 * 0.8 + w * 0.8]
    acc1 = [0.0 + w * -0.6 + 1.0 * 0.6, 0.0, 0.0 + w * 0.8 + 1.0 * 0.8]
    want = []
    for acc in (acc0, acc1):
        L = math.sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2])
        want.append([acc[0] / L, acc[1] / L, acc[2] / L])
    got = S.filter_pass(n, offsets, nb, 0.0)
    assert got.tolist() == want
    # in closed form: (-0.6 (1 - 0.0784), 0, 0.8 (1 + 0.0784)) normalised -- the roof flattens a little
    c = np.array([-0.6 * (1 - 0.0784), 0.0, 0.8 * (1 + 0.0784)])
    assert np.allclose(got[0], c / np.linalg.norm(c), rtol=0, atol=1e-15) and got[0][0] == -got[1][0] and abs(got[0][0]) < 0.6
    # the vertex update with those normals: the ridge vertices 1 and 2 have both faces, the feet one each
    rows = [[0], [0, 1], [0, 1], [1]]
    x = TENT_V.astype(np.float64).tolist()
    for _ in range(3):
        x = loop_vertex_pass(x, TENT_F.tolist(), want, rows)
    out = S.denoise_spec(TENT_V, TENT_F, 0.0, 1, 3)
    assert out.dtype == np.float32 and out.tobytes() == np.array(x, dtype=np.float64).astype(np.float32).tobytes()
    assert out[1, 2] < 3.0 and out[0, 2] > 0.0                        # the ridge comes down and the feet come up: towards the flatter planes


def test_the_pyramid_by_hand():
    n = S.face_normals(PYR_V, PYR_F)
    assert n.tolist() == [[0.6, 0.0, 0.8], [0.0, 0.6, 0.8], [-0.6, 0.0, 0.8], [0.0, -0.6, 0.8]]
    offsets, nb = S.neighbourhoods(PYR_F, 5)
    assert offsets.tolist() == [0, 4, 8, 12, 16] and nb.tolist() == [0, 1, 2, 3] * 4          # the apex joins all four; no face twice
    # T = 0.5, face 0: itself d = 1, w = 0.25; face 1 d = 0.64, w = 0.14^2; face 2 (opposite) d = 0.28 <= T, nothing; face 3 like face 1
    d = (0.6 * 0.0 + 0.0 * 0.6) + 0.8 * 0.8
    w = (d - 0.5) * (d - 0.5)
    assert abs(w - 0.0196) < 1e-15 and dot(n[0], n[2]) < 0.5
    acc = [0.0, 0.0, 0.0]
    for wj, nj in ((0.25, [0.6, 0.0, 0.8]), (w, [0.0, 0.6, 0.8]), (w, [0.0, -0.6, 0.8])):
        acc = [acc[0] + wj * nj[0], acc[1] + wj * nj[1], acc[2] + wj * nj[2]]
    L = math.sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2])
    got = S.filter_pass(n, offsets, nb, 0.5)
    assert got[0].tolist() == [acc[0] / L, acc[1] / L, acc[2] / L]
    c = np.array([0.15, 0.0, 0.2 + 2 * 0.0196 * 0.8])
    assert np.allclose(got[0], c / np.linalg.norm(c), rtol=0, atol=1e-15)
    assert got.tolist() == loop_filter_pass(n.tolist(), [[0, 1, 2, 3]] * 4, 0.5)
    # T = 0.7: only the face itself is left; T = 0: the opposite face joins in
    assert np.allclose(S.filter_pass(n, offsets, nb, 0.7), n, rtol=0, atol=1e-15)
    assert S.filter_pass(n, offsets, nb, 0.0).tolist() == loop_filter_pass(n.tolist(), [[0, 1, 2, 3]] * 4, 0.0)
    # the whole filter against the plain loops, and the apex (four faces) comes down
    normals = n.tolist()
    for _ in range(2):
        normals = loop_filter_pass(normals, [[0, 1, 2, 3]] * 4, 0.5)
    assert S.filtered_normals_spec(PYR_V, PYR_F, 0.5, 2).tolist() == normals
    x = PYR_V.astype(np.float64).tolist()
    rows = [[0, 1, 2, 3], [0, 3], [0, 1], [1, 2], [2, 3]]
    for _ in range(2):
        x = loop_vertex_pass(x, PYR_F.tolist(), normals, rows)
    out = S.denoise_spec(PYR_V, PYR_F, 0.5, 2, 2)
    assert out.tobytes() == np.array(x, dtype=np.float64).astype(np.float32).tobytes() and out[0, 2] < 3.0


def test_a_face_whose_sum_is_zero_keeps_its_normal():
    # face 1 is valid but has no area: its normal is zero, every d is 0 <= T, the sum is zero and the zero normal stays; it adds nothing to
    # its neighbours either, though it sits in their neighbourhoods
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [1, 1, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 4]], dtype=np.int64)
    n = S.face_normals(verts, faces)
    assert n[0].tolist() == [0, 0, 1] and n[1].tolist() == [0, 0, 0] and np.isclose(np.linalg.norm(n[2]), 1.0)
    offsets, nb = S.neighbourhoods(faces, 5)
    assert nb.tolist() == [0, 1, 2] * 3
    for T in (0.0, 0.5):
        got = S.filter_pass(n, offsets, nb, T)
        assert got[1].tolist() == [0, 0, 0]
        assert got.tolist() == loop_filter_pass(n.tolist(), [[0, 1, 2]] * 3, T)
    info = S.info_spec(verts, faces, 0.5, 2, 2)
    assert info['faces_valid'] == 3 and info['degenerate_faces'] == 1
    # vertex 3 has only the area-free face: its sum is zero, it keeps its bytes
    assert S.denoise_spec(verts, faces, 0.0, 2, 2)[3].tobytes() == verts[3].tobytes()


def test_the_cube():
    for n, nv in ((1, 8), (2, 26), (5, 152), (8, 386)):
        verts, faces, normals = S.cube(n)
        assert verts.shape == (nv, 3) and faces.shape == (12 * n * n, 3) and normals.shape == faces.shape
        assert np.array_equal(np.unique(faces), np.arange(nv))                                 # welded: every vertex used
        assert np.array_equal(S.face_normals(verts, faces), normals) and (np.abs(normals).sum(axis=1) == 1).all()
        centroid = verts[faces].mean(axis=1)
        assert ((centroid - n / 2.0) * normals).sum(axis=1).tolist() == [n / 2.0] * faces.shape[0]   # outward
        assert (np.diff(smooth_spec.adjacency(faces, nv)[2]) == 0).all()                      # closed: every edge has two faces
        assert S.cube_surface_distance(verts, n).max() == 0.0
    assert S.cube_surface_distance(np.array([[4, 4, 9.5], [4, 4, 7.0], [-3, -4, 1], [4, 4, 4]]), 8).tolist() == [1.5, 1.0, 5.0, 4.0]


def test_a_noisy_cube_gets_its_faces_and_its_edges_back():
    n = 8
    verts, faces, normals = S.cube(n)
    assert verts.shape == (386, 3) and faces.shape == (768, 3)
    noisy = (verts + np.random.default_rng(7).normal(0, 0.1, verts.shape)).astype(np.float32)
    out = S.denoise_spec(noisy, faces, 0.5, 5, 10)
    taubin = smooth_spec.smooth_spec(noisy, faces, 10)
    edge = ((verts == 0) | (verts == n)).sum(axis=1) >= 2              # the vertices on the cube's edges and corners
    assert int(edge.sum()) == 12 * (n - 1) + 8
    angle = {k: S.mean_normal_angle(v, faces, normals) for k, v in (('noisy', noisy), ('denoised', out), ('taubin', taubin))}
    dist = {k: float(S.cube_surface_distance(v[edge], n).mean()) for k, v in (('noisy', noisy), ('denoised', out), ('taubin', taubin))}
    print('mean face-normal error, degrees: {}'.format({k: round(v, 3) for k, v in angle.items()}))
    print('mean distance of the edge and corner vertices from the surface: {}'.format({k: round(v, 4) for k, v in dist.items()}))
    assert angle['denoised'] <= 0.25 * angle['noisy']
    assert dist['denoised'] <= 0.7 * dist['noisy']
    assert dist['denoised'] <= dist['taubin']
    assert out.dtype == np.float32 and np.isfinite(out).all()


def test_zero_iterations():
    verts, faces = smooth_spec.noisy_sphere(1)
    assert S.denoise_spec(verts, faces, 0.5, 5, 0).tobytes() == verts.tobytes()
    assert S.info_spec(verts, faces, 0.5, 5, 0)['moved_vertices'] == 0
    assert np.array_equal(S.filtered_normals_spec(verts, faces, 0.5, 0), S.face_normals(verts, faces))
    # an exact flat grid: every normal is (0, 0, 1) and every centroid lies in the plane, so without the filter nothing moves -- nor with it
    g = np.arange(6, dtype=np.float32)
    grid = np.stack(list(np.meshgrid(g + 1, g + 2, indexing='ij')) + [np.full((6, 6), 3.0, dtype=np.float32)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(5), np.arange(5), indexing='ij')
    q = (i * 6 + j).reshape(-1)
    tri = np.concatenate([np.stack([q, q + 6, q + 7], axis=1), np.stack([q, q + 7, q + 1], axis=1)]).astype(np.int64)
    assert (S.face_normals(grid, tri) == [0, 0, 1]).all()
    assert S.denoise_spec(grid, tri, 0.5, 0, 7).tobytes() == grid.tobytes()
    assert S.denoise_spec(grid, tri, 0.5, 3, 7).tobytes() == grid.tobytes()
    # on a noisy mesh the filtered normals differ from the faces' own and the vertices do move
    assert S.info_spec(verts, faces, 0.5, 1, 1)['moved_vertices'] > 0


def test_invalid_and_duplicated_faces_and_isolated_vertices():
    verts, faces = smooth_spec.noisy_sphere(1)
    nv = verts.shape[0]
    bad = np.array([[-1, 1, 2], [0, nv, 2], [0, 1, 1 << 40], [3, 3, 5], [4, 5, 4], [6, 6, 6]], dtype=np.int64)
    mixed = np.concatenate([bad[:3], faces[:30], bad[3:]])
    n = S.filtered_normals_spec(verts, mixed, 0.5, 3)
    assert (n[:3] == 0).all() and (n[33:] == 0).all()                  # an invalid face: zeros throughout
    # the invalid faces take no part: the valid ones keep their ascending order, so the result is that of the valid faces alone
    assert np.array_equal(n[3:33], S.filtered_normals_spec(verts, faces[:30], 0.5, 3))
    out = S.denoise_spec(verts, mixed, 0.5, 3, 4)
    assert out.tobytes() == S.denoise_spec(verts, faces[:30], 0.5, 3, 4).tobytes()
    unused = np.setdiff1d(np.arange(nv), np.unique(faces[:30]))
    assert unused.size > 0 and out[unused].tobytes() == verts[unused].tobytes()            # isolated vertices keep their bytes
    info = S.info_spec(verts, mixed, 0.5, 3, 4)
    assert info == {'vertices': nv, 'faces_valid': 30, 'degenerate_faces': 0, 'moved_vertices': info['moved_vertices'], 'threshold': 0.5,
                    'normal_iters': 3, 'vertex_iters': 4} and 0 < info['moved_vertices'] <= nv - unused.size
    assert S.denoise_spec(verts, bad, 0.5, 3, 4).tobytes() == verts.tobytes()
    # a duplicated face is two faces: both sit in every neighbourhood that holds one, and the copy weighs in a second time
    dup = np.concatenate([PYR_F, PYR_F[:1]])
    offsets, nb = S.neighbourhoods(dup, 5)
    assert nb.tolist() == [0, 1, 2, 3, 4] * 5
    n = S.filter_pass(S.face_normals(PYR_V, dup), offsets, nb, 0.5)
    assert np.array_equal(n[0], n[4]) and n[1][0] > S.filter_pass(S.face_normals(PYR_V, PYR_F), *S.neighbourhoods(PYR_F, 5), 0.5)[1][0]
    assert n.tolist() == loop_filter_pass(S.face_normals(PYR_V, dup).tolist(), [[0, 1, 2, 3, 4]] * 5, 0.5)
    # empty meshes
    assert S.denoise_spec(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)).shape == (0, 3)
    assert S.denoise_spec(verts, np.zeros((0, 3), np.int64)).tobytes() == verts.tobytes()
    assert S.filtered_normals_spec(verts, np.zeros((0, 3), np.int64), 0.5, 2).shape == (0, 3)


def test_denoise_mesh_argument_rules():
    import torch
    from ppsurf_amd import denoise
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for bad in (1.0, -0.1, 1.5, float('nan'), float('inf'), '0.5', None, True):
        with pytest.raises(ValueError, match='threshold'):
            denoise.denoise_mesh(v, f, threshold=bad)
        with pytest.raises(ValueError, match='threshold'):
            denoise.filtered_face_normals(v, f, bad, 1)
    for bad in (-1, 1001, 2.5, float('nan'), '3', None, True):
        with pytest.raises(ValueError, match='normal_iters'):
            denoise.denoise_mesh(v, f, normal_iters=bad)
        with pytest.raises(ValueError, match='normal_iters'):
            denoise.filtered_face_normals(v, f, 0.5, bad)
        with pytest.raises(ValueError, match='vertex_iters'):
            denoise.denoise_mesh(v, f, vertex_iters=bad)
    assert denoise._checked_params(0, 0, np.int64(1000)) == (0.0, 0, 1000) and denoise._checked_params(np.float32(0.5), 1000, 0) == (0.5, 1000, 0)
    assert denoise._checked_params(math.nextafter(1.0, 0.0), 5, 10)[0] < 1.0
    # good scalars, CPU tensors: the device guard of the other mesh stages, after the parameters
    for fn in (lambda: denoise.denoise_mesh(v, f), lambda: denoise.denoise_mesh(v, f, 0.0, 0, 0), lambda: denoise.filtered_face_normals(v, f)):
        with pytest.raises(denoise.CpuTensorError, match='no CPU'):
            fn()
    assert issubclass(denoise.CpuTensorError, PpsError) and issubclass(denoise.CpuTensorError, ValueError)
    with pytest.raises(ValueError, match='denoise_mesh: tensor on cpu; inputs must be device tensors, there is no CPU path'):
        denoise.denoise_mesh(v, f)


@pytest.mark.parametrize('argv', [['m.ply'], ['m.ply', 'o.obj'], ['m.ply', 'o.ply', '--threshold', '1'], ['m.ply', 'o.ply', '--threshold', '-0.1'],
                                  ['m.ply', 'o.ply', '--threshold', 'nan'], ['m.ply', 'o.ply', '--threshold', 'half'],
                                  ['m.ply', 'o.ply', '--normal_iters', '-1'], ['m.ply', 'o.ply', '--normal_iters', '1001'],
                                  ['m.ply', 'o.ply', '--normal_iters', '2.5'], ['m.ply', 'o.ply', '--normal_iters', 'True'],
                                  ['m.ply', 'o.ply', '--vertex_iters', '-1'], ['m.ply', 'o.ply', '--vertex_iters', '1001'],
                                  ['m.ply', 'o.ply', '--vertex_iters', '2.5'], ['m.ply', 'o.ply', '--vertex_iters', 'True']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import denoise
    with pytest.raises(SystemExit) as e:
        denoise.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_the_denoise_entries_are_declared_and_every_call_site_lies_in_denoise_py():
    from ppsurf_amd import _lib, build
    I, I64, P, D = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_denoise_face_normals'] == (I, [P, I64, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_denoise_filter_pass'] == (I, [P, I64, I64, P, P, I64, P, D, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_denoise_vertex_pass'] == (I, [P, I64, P, I64, P, P, P, I64, P, P])
    assert _lib.EXT_PARAMS['ppsx_denoise_face_normals'] == ['verts', 'nv', 'faces', 'nf', 'normals', 'stream']
    assert _lib.EXT_PARAMS['ppsx_denoise_filter_pass'] == ['faces', 'nf', 'nv', 'offsets', 'inc', 'ni', 'normals', 'threshold', 'out', 'stream']
    assert _lib.EXT_PARAMS['ppsx_denoise_vertex_pass'] == ['x', 'nv', 'faces', 'nf', 'normals', 'offsets', 'inc', 'ni', 'out', 'stream']
    assert not any(n.startswith('pps_denoise') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    sites = call_sites.ext_call_sites('ppsx_denoise')
    for name, where in sites.items():
        for path, line, nargs in where:
            assert path == 'denoise.py', '{}:{}:{}'.format(path, line, name)
            assert nargs == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}:{}'.format(path, line, name)
    assert {name: len(where) for name, where in sites.items()} == {'ppsx_denoise_face_normals': 1, 'ppsx_denoise_filter_pass': 1,
                                                                   'ppsx_denoise_vertex_pass': 1}
    assert 'pps_denoise.hip' in build.SOURCES
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and {'ppsx_denoise_face_normals', 'ppsx_denoise_filter_pass', 'ppsx_denoise_vertex_pass'} <= set(_lib._ext_entries)
