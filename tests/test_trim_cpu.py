"""CPU tier of the trim by support: properties of the numpy specification tests/trim_spec.py, the lower-median rank of
the spacing, the models' `gen_trim_factor`, the command's argument errors and the extension entries of the C ABI."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest

import trim_spec as S
from golden_util import REPO

TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32)
FACE = np.array([[0, 1, 2]], dtype=np.int64)


def test_a_point_on_the_triangle_is_supported_for_any_radius():
    on = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [0, 1, 0], [2, 2, 0], [1, 1, 0], [0.5, 2.25, 0], [3.5, 0.25, 0]], dtype=np.float32)
    for p in on:
        s, t, d2 = S.closest_on_triangle(p[None], *TRI)
        assert d2[0] == 0.0 and np.array_equal(TRI[0] + s[0] * (TRI[1] - TRI[0]) + t[0] * (TRI[2] - TRI[0]), p)
        for r in (1e-200, 1e-30, 1e-6, 1.0):                          # 1e-200 squared is 0: d2 = 0 still passes <=
            assert S.face_support_spec(p[None], TRI, FACE, r).tolist() == [True]
    off = np.array([[1, 1, 1e-3]], dtype=np.float32)
    assert S.face_support_spec(off, TRI, FACE, 1e-4).tolist() == [False] and S.face_support_spec(off, TRI, FACE, 2e-3).tolist() == [True]


@pytest.mark.parametrize('name,tri,p,dist', S.threshold_cases(), ids=[c[0] for c in S.threshold_cases()])
def test_the_threshold_is_exact(name, tri, p, dist):
    d2 = S.closest_on_triangle(p[None], *tri)[2][0]
    assert d2 == dist * dist                                          # every operation exact on dyadic coordinates
    below = np.nextafter(np.float64(dist), 0.0)
    assert below < dist and below * below < d2
    assert S.face_support_spec(p[None], tri, FACE, dist).tolist() == [True]
    assert S.face_support_spec(p[None], tri, FACE, below).tolist() == [False]
    # the regions are the ones the names say
    s, t, _ = S.closest_on_triangle(p[None], *tri)
    assert {'interior': 0 < s[0] < 1 and 0 < t[0] < 1, 'edge': 0 < s[0] < 1 and t[0] == 0, 'vertex': s[0] == 0 and t[0] == 0}[name]


def test_a_zero_area_face_never_raises_and_is_its_longest_edge():
    import warnings
    pts = np.array([[0.5, 0.25, 0], [3, 0, 1], [-2, 0, 0], [1, 1, 1]], dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        point = np.array([[1, 1, 1]] * 3, dtype=np.float32)           # three equal corners: the distance to that point
        d2 = S.closest_on_triangle(pts, *point)[2]
        assert np.array_equal(d2, ((pts.astype(np.float64) - 1.0) ** 2).sum(axis=1))
        line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float32)   # collinear: the segment (0,0,0)-(2,0,0)
        d2 = S.closest_on_triangle(pts, *line)[2]
        q = np.clip(pts[:, 0].astype(np.float64), 0.0, 2.0)
        assert np.array_equal(d2, (pts[:, 0] - q) ** 2 + pts[:, 1].astype(np.float64) ** 2 + pts[:, 2].astype(np.float64) ** 2)
        two = np.array([[0, 0, 0], [0, 0, 0], [0, 2, 0]], dtype=np.float32)    # two equal corners
        assert np.all(np.isfinite(S.closest_on_triangle(pts, *two)[2]))
        assert S.face_support_spec(pts, np.concatenate([point, line, two]), np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]]), 0.3).tolist() == [True, True, False]


def test_bad_indices_and_non_finite_corners_are_unsupported():
    cloud = np.array([[1, 1, 0]], dtype=np.float32)
    verts = np.concatenate([TRI, np.array([[np.nan, 0, 0], [np.inf, 0, 0]], dtype=np.float32)])
    faces = np.array([[0, 1, 2], [-1, 1, 2], [0, 5, 2], [0, 1, 1 << 40], [0, 1, 3], [0, 4, 2], [2, 1, 0]], dtype=np.int64)
    assert S.face_support_spec(cloud, verts, faces, 1e6).tolist() == [True, False, False, False, False, False, True]
    assert S.face_support_spec(np.zeros((0, 3), dtype=np.float32), verts, faces, 1e6).tolist() == [False] * 7
    assert S.face_support_spec(cloud, verts, np.zeros((0, 3), dtype=np.int64), 1.0).shape == (0,)


def test_the_spacing_is_the_lower_median():
    line = lambda xs: np.stack([np.asarray(xs, dtype=np.float32), np.zeros(len(xs), dtype=np.float32), np.zeros(len(xs), dtype=np.float32)], axis=1)
    # nearest other point at 1, 1, 2, 4: squared 1, 1, 4, 16; rank (4 - 1) // 2 = 1 -> 1 (the upper median would give 2)
    assert S.spacing_spec(line([0, 1, 3, 7]), 1) == 1.0
    # second nearest at 3, 2, 3, 6: squared 4, 9, 9, 36 in order; rank 1 -> 9
    assert S.spacing_spec(line([0, 1, 3, 7]), 2) == 3.0
    # five points, rank 2: nearest at 1, 1, 2, 4, 8 -> 2
    assert S.spacing_spec(line([0, 1, 3, 7, 15]), 1) == 2.0
    assert S.spacing_spec(line([0, 0, 5]), 1) == 0.0                  # a duplicate is another point at distance 0
    for n, k in ((1, 1), (8, 8), (3, 5)):
        with pytest.raises(ValueError):
            S.spacing_spec(np.zeros((n, 3), dtype=np.float32), k)


def test_models_take_gen_trim_factor():
    from source.poco_model import PocoModel
    from source.ppsurf_model import PPSurfModel
    from ppsurf_amd import reconstruct
    kw = dict(output_names=['imp_surf_sign'], in_channels=3, out_channels=2, k=64, lambda_l1=0.0, debug=False,
              in_file='datasets/abc_minimal/testset.txt', results_dir='results', padding_factor=0.05, name='m', network_latent_size=32,
              gen_subsample_manifold_iter=10, gen_subsample_manifold=10000, gen_resolution_global=129, rec_batch_size=25000, gen_refine_iter=10,
              workers=0)
    pps = dict(kw, pointnet_latent_size=32, num_pts_local=50)
    assert PocoModel(**kw).gen_trim_factor is None and PPSurfModel(**pps).gen_trim_factor is None
    assert PocoModel(gen_trim_factor=2.5, **kw).gen_trim_factor == 2.5
    m = PPSurfModel(gen_trim_factor='3', gen_max_faces=100, gen_color_k=4, **pps)
    assert m.gen_trim_factor == 3.0 and type(m.gen_trim_factor) is float and m.gen_max_faces == 100 and m.gen_color_k == 4
    for bad in (0, 0.0, -1, -0.5, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='gen_trim_factor'):
            PocoModel(gen_trim_factor=bad, **kw)
        with pytest.raises(ValueError, match='gen_trim_factor'):
            PPSurfModel(gen_trim_factor=bad, **pps)
    params = inspect.signature(reconstruct.export_mesh_and_refine_vertices_region_growing_v3).parameters
    assert params['trim_factor'].default is None and list(params)[-1] == 'max_faces'


@pytest.mark.parametrize('argv', [['m.ply', 's.ply', 'o.ply'], ['m.ply', 's.ply', 'o.ply', '--factor', '2', '--dist', '0.1'],
                                  ['m.ply', 's.ply', 'o.ply', '--factor', '0'], ['m.ply', 's.ply', 'o.ply', '--dist', '-1'],
                                  ['m.ply', 's.ply', 'o.ply', '--dist', 'nan'], ['m.ply', 's.ply', 'o.ply', '--factor', 'inf'],
                                  ['m.ply', 's.ply', 'o.ply', '--factor', '2', '--spacing_k', '0'], ['m.ply', 's.ply', 'o.obj', '--dist', '1'],
                                  ['m.ply', 's.ply', '--dist', '1']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import trim
    with pytest.raises(SystemExit) as e:
        trim.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_host_side_argument_errors_need_no_device():
    import torch
    from ppsurf_amd import trim
    from ppsurf_amd._lib import PpsError
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for fn in (lambda: trim.face_support(v, v, f, 1.0), lambda: trim.trim_mesh(v, v, f, 1.0), lambda: trim.cloud_spacing(v, 1)):
        with pytest.raises(PpsError, match='no CPU'):
            fn()
    assert float(np.float32(0.7)) < 0.7 <= float(trim._f32_not_below(0.7)) == float(np.nextafter(np.float32(0.7), np.float32(1)))
    assert trim._f32_not_below(0.5) == np.float32(0.5) and trim._f32_not_below(0.1) == np.float32(0.1)


def test_the_trim_entries_are_declared_and_every_call_site_has_their_argument_count():
    from ppsurf_amd import _lib, build
    I, I64, P, F, D = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    assert _lib.EXT_SIGNATURES['ppsx_trim_cell_slots'] == (I, [P, I64, P, P, F, F, P, I64, P, P])
    assert _lib.EXT_SIGNATURES['ppsx_trim_face_support'] == (I, [P, I64, P, I64, P, I64, P, P, F, F, P, I64, P, P, D, P, P])
    assert _lib.EXT_PARAMS['ppsx_trim_face_support'] == ['verts', 'nv', 'faces', 'nf', 'pts', 'n', 'lo', 'hi', 'h', 'inv_h', 'table', 'capacity',
                                                         'order', 'offsets', 'r', 'support', 'stream']
    assert not any(n.startswith('pps_trim') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    text = open(os.path.join(REPO, 'ppsurf_amd', 'trim.py')).read()
    seen = {}
    for node in ast.walk(ast.parse(text)):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'call' and node.args
                and isinstance(node.args[0], ast.Constant) and str(node.args[0].value).startswith('ppsx_trim')):
            name = node.args[0].value
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            assert len(node.args) - 1 == len(_lib.EXT_PARAMS[name]) - 1, '{}:{}'.format(name, node.lineno)
            seen[name] = seen.get(name, 0) + 1
    assert seen == {'ppsx_trim_cell_slots': 1, 'ppsx_trim_face_support': 1}
    assert 'pps_trim.hip' in build.SOURCES and 'pps_tri.h' in build.HEADERS
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and {'ppsx_trim_cell_slots', 'ppsx_trim_face_support'} <= set(_lib._ext_entries)
