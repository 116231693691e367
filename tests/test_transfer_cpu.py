"""CPU tier of the colour transfer: the colour half of the readers on files written here from the published layouts,
the coloured PLY writer, properties of the numpy specification tests/transfer_spec.py, and the extension header of the C ABI."""
import ast
import ctypes
import glob
import os
import re
import struct

import numpy as np
import pytest

import transfer_spec as T
from golden_util import REPO


# ---- writers of the test files ---------------------------------------------------------------------------------------------------------------
LAS_REC = {0: 20, 1: 28, 2: 26, 3: 34, 7: 36}
LAS_RGB_AT = {2: 20, 3: 28, 7: 30}


def write_las_colored(path, ints, fmt, rgb=None, intensity=None, rec_len=None):
    """Uncompressed LAS 1.2 (formats 0-3) or 1.4 (format 7) from the ASPRS record layouts: int32 X Y Z, uint16 intensity at 12, three uint16
    RGB at 20 (format 2), 28 (format 3) or 30 (format 7); every other byte of a record is filler that is not zero."""
    n = ints.shape[0]
    rec_len = LAS_REC[fmt] if rec_len is None else rec_len
    minor = 4 if fmt >= 6 else 2
    header_size = 375 if minor == 4 else 227
    head = bytearray(header_size)
    head[0:4] = b'LASF'
    head[24], head[25] = 1, minor
    struct.pack_into('<HI', head, 94, header_size, header_size)
    struct.pack_into('<BHI', head, 104, fmt, rec_len, 0 if minor == 4 else n)
    struct.pack_into('<3d', head, 131, 0.001, 0.001, 0.001)
    struct.pack_into('<3d', head, 155, 512345.0, 5403210.0, 310.0)
    if minor == 4:
        struct.pack_into('<Q', head, 247, n)
    body = bytearray(n * rec_len)
    for i in range(n):
        at = i * rec_len
        for b in range(12, rec_len):
            body[at + b] = (41 * i + b) & 0xFF | 1
        struct.pack_into('<3i', body, at, *[int(v) for v in ints[i]])
        if rec_len >= 14:
            struct.pack_into('<H', body, at + 12, 0 if intensity is None else int(intensity[i]))
        if rgb is not None and fmt in LAS_RGB_AT and rec_len >= LAS_RGB_AT[fmt] + 6:
            struct.pack_into('<3H', body, at + LAS_RGB_AT[fmt], *[int(v) for v in rgb[i]])
    with open(path, 'wb') as f:
        f.write(bytes(head) + bytes(body))


def _ints(n, seed):
    return np.random.RandomState(seed).randint(-50000, 50000, size=(n, 3)).astype(np.int32)


def _xyz_of(ints):
    return ints.astype(np.float64) * 0.001 + np.array([512345.0, 5403210.0, 310.0])[None]


# ---- readers ---------------------------------------------------------------------------------------------------------------------------------
def test_las_format_2_sixteen_bit_colours_are_shifted(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(1)
    ints, rgb = _ints(40, 1), rng.randint(0, 65536, size=(40, 3))
    rgb[0] = (65535, 256, 255)
    path = str(tmp_path / 'a.las')
    write_las_colored(path, ints, 2, rgb=rgb, intensity=rng.randint(0, 65536, size=40))
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and got.shape == (40, 3) and np.array_equal(got, (rgb >> 8).astype(np.uint8))
    assert got[0].tolist() == [255, 1, 0]
    assert np.array_equal(meshio.load_pts(path), _xyz_of(ints))


def test_las_format_3_small_values_are_kept(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(2)
    ints, rgb = _ints(30, 2), rng.randint(0, 256, size=(30, 3))
    rgb[3] = (255, 0, 7)
    path = str(tmp_path / 'b.las')
    write_las_colored(path, ints, 3, rgb=rgb, intensity=rng.randint(0, 65536, size=30))
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb.astype(np.uint8))
    assert np.array_equal(meshio.load_pts(path), _xyz_of(ints))


def test_las_format_7(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(3)
    ints, rgb = _ints(25, 3), rng.randint(0, 65536, size=(25, 3))
    path = str(tmp_path / 'c.las')
    write_las_colored(path, ints, 7, rgb=rgb, intensity=rng.randint(0, 65536, size=25))
    assert np.array_equal(meshio.load_pts_colors(path), (rgb >> 8).astype(np.uint8))
    assert np.array_equal(meshio.load_pts(path), _xyz_of(ints))


def test_las_without_rgb_takes_a_grey_from_intensity(tmp_path):
    from ppsurf_amd import meshio
    inten = np.array([0, 1, 500, 999, 1000, 333], dtype=np.int64)
    ints = _ints(6, 4)
    path = str(tmp_path / 'd.las')
    write_las_colored(path, ints, 1, intensity=inten)
    want = ((inten * 255 + 500) // 1000).astype(np.uint8)
    assert want.tolist() == [0, 0, 128, 255, 255, 85]
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack([want] * 3, axis=1))
    assert meshio.load_pts(path).shape[0] == got.shape[0]
    # a format WITH RGB whose RGB is 0 everywhere falls back the same way
    path2 = str(tmp_path / 'd2.las')
    write_las_colored(path2, ints, 2, rgb=np.zeros((6, 3), dtype=np.int64), intensity=inten)
    assert np.array_equal(meshio.load_pts_colors(path2), got)


def test_las_without_colour_or_intensity_is_none(tmp_path):
    from ppsurf_amd import meshio
    path = str(tmp_path / 'e.las')
    write_las_colored(path, _ints(9, 5), 0, intensity=np.zeros(9, dtype=np.int64))
    assert meshio.load_pts_colors(path) is None
    assert meshio.load_pts(path).shape == (9, 3)


def test_las_record_too_short_for_its_colour_field(tmp_path):
    from ppsurf_amd import meshio
    path = str(tmp_path / 'short.las')
    write_las_colored(path, _ints(4, 6), 2, rec_len=24)
    with pytest.raises(ValueError, match='short.las'):
        meshio.load_pts_colors(path)


PCD_HEAD = ('# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z {0}\nSIZE 4 4 4 4\nTYPE F F F {1}\nCOUNT 1 1 1 1\n'
            'WIDTH {2}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {2}\nDATA {3}\n')


def test_pcd_binary_with_float_packed_rgb(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(7)
    xyz, rgb = rng.randn(12, 3).astype(np.float32), rng.randint(0, 256, size=(12, 3))
    rgb[0] = (255, 0, 128)
    packed = ((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]).astype(np.uint32)
    path = str(tmp_path / 'a.pcd')
    with open(path, 'wb') as f:
        f.write(PCD_HEAD.format('rgb', 'F', 12, 'binary').encode('ascii'))
        for p, c in zip(xyz, packed):
            f.write(struct.pack('<3fI', *[float(v) for v in p], int(c)))
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb.astype(np.uint8))
    assert np.array_equal(meshio.load_pts(path), xyz)


def test_pcd_ascii_with_unsigned_rgba_and_with_float_rgb(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(8)
    xyz, rgb = rng.randn(10, 3).astype(np.float32), rng.randint(0, 256, size=(10, 3))
    packed = ((0xFF << 24) | (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]).astype(np.uint32)
    path = str(tmp_path / 'u.pcd')
    with open(path, 'w') as f:
        f.write(PCD_HEAD.format('rgba', 'U', 10, 'ascii'))
        for p, c in zip(xyz, packed):
            f.write('{!r} {!r} {!r} {}\n'.format(*[float(v) for v in p], int(c)))
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb.astype(np.uint8))
    assert np.array_equal(meshio.load_pts(path), xyz)
    # TYPE F in an ascii file: the value is the float32 whose bits are the packed colour (PCL writes it with enough digits to round-trip)
    small = (packed & np.uint32(0x00FFFFFF)).astype(np.uint32)
    path = str(tmp_path / 'f.pcd')
    with open(path, 'w') as f:
        f.write(PCD_HEAD.format('rgb', 'F', 10, 'ascii'))
        for p, c in zip(xyz, small.view(np.float32)):
            f.write('{!r} {!r} {!r} {!r}\n'.format(*[float(v) for v in p], float(c)))
    assert np.array_equal(meshio.load_pts_colors(path), rgb.astype(np.uint8))
    # no colour field
    path = str(tmp_path / 'n.pcd')
    with open(path, 'w') as f:
        f.write(PCD_HEAD.format('intensity', 'F', 10, 'ascii'))
        for p in xyz:
            f.write('{!r} {!r} {!r} 0.5\n'.format(*[float(v) for v in p]))
    assert meshio.load_pts_colors(path) is None


def test_coff_with_integer_and_with_float_colours(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(9)
    v, rgb = rng.randn(9, 3), rng.randint(0, 256, size=(9, 3))
    path = str(tmp_path / 'i.off')
    with open(path, 'w') as f:
        f.write('COFF 9 1 0\n# colours follow the position\n' + ''.join('{!r} {!r} {!r} {} {} {} 255\n'.format(*map(float, p), *map(int, c))
                                                                          for p, c in zip(v, rgb)) + '3 0 1 2\n')
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb.astype(np.uint8))
    assert np.array_equal(meshio.load_pts(path), v)
    # float colours in [0, 1] (one beyond the range is clipped), after a normal: CNOFF
    frac = rng.rand(9, 3)
    frac[0] = (1.0, 0.0, 1.5)
    path = str(tmp_path / 'f.off')
    with open(path, 'w') as f:
        f.write('CNOFF\n9 0 0\n' + ''.join('{!r} {!r} {!r} 0 0 1 {!r} {!r} {!r} 0.5\n'.format(*map(float, p), *map(float, c)) for p, c in zip(v, frac)))
    got = meshio.load_pts_colors(path)
    assert np.array_equal(got, np.rint(np.clip(frac, 0.0, 1.0) * 255.0).astype(np.uint8)) and got[0].tolist() == [255, 0, 255]
    assert np.array_equal(meshio.load_pts(path), v)
    # a plain OFF has none
    path = str(tmp_path / 'p.off')
    with open(path, 'w') as f:
        f.write('OFF 9 0 0\n' + ''.join('{!r} {!r} {!r}\n'.format(*map(float, p)) for p in v))
    assert meshio.load_pts_colors(path) is None


def test_obj_with_complete_and_with_partial_colours(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(10)
    v, frac = rng.randn(7, 3), rng.rand(7, 3)
    want = np.rint(frac * 255.0).astype(np.uint8)
    path = str(tmp_path / 'c.obj')
    with open(path, 'w') as f:
        f.write('# obj\n' + ''.join('v {!r} {!r} {!r} {!r} {!r} {!r}\n'.format(*map(float, p), *map(float, c)) for p, c in zip(v, frac)) + 'f 1 2 3\n')
    got = meshio.load_pts_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(meshio.load_pts(path), v.astype(np.float32))
    mv, mf, mc = meshio.load_mesh_any(path)
    assert np.array_equal(mv, v.astype(np.float32)) and mf.tolist() == [[0, 1, 2]] and np.array_equal(mc, want)
    assert len(meshio.read_obj_mesh(path)) == 2                                     # the two-result form stays
    path = str(tmp_path / 'p.obj')
    with open(path, 'w') as f:
        lines = ['v {!r} {!r} {!r} {!r} {!r} {!r}\n'.format(*map(float, p), *map(float, c)) for p, c in zip(v, frac)]
        lines[4] = 'v {!r} {!r} {!r}\n'.format(*map(float, v[4]))
        f.write(''.join(lines))
    assert meshio.load_pts_colors(path) is None and meshio.load_mesh_any(path)[2] is None
    assert meshio.load_pts(path).shape == (7, 3)


def test_ply_colours_and_files_without_any(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(11)
    v, rgb = rng.randn(8, 3).astype(np.float32), rng.randint(0, 256, size=(8, 3)).astype(np.uint8)
    path = str(tmp_path / 'c.ply')
    meshio.write_ply_mesh_colored(path, v, np.zeros((0, 3), dtype=np.int32), rgb)
    assert np.array_equal(meshio.load_pts_colors(path), rgb)
    assert np.array_equal(meshio.load_pts(path)[:, :3].astype(np.float32), v)
    plain = str(tmp_path / 'p.ply')
    meshio.write_ply_points(plain, v)
    assert meshio.load_pts_colors(plain) is None
    stl = str(tmp_path / 'b.stl')
    with open(stl, 'wb') as f:
        f.write(b'binary'.ljust(80, b' ') + struct.pack('<I', 1) + struct.pack('<12fH', *([0.0] * 12), 0))
    assert meshio.load_pts(stl).shape == (3, 3) and meshio.load_pts_colors(stl) is None
    np.save(str(tmp_path / 'x.npy'), rng.rand(5, 6))                               # columns 3-5 of .npy / .xyz are normals, not colours
    assert meshio.load_pts_colors(str(tmp_path / 'x.npy')) is None


# ---- the coloured PLY writer -------------------------------------------------------------------------------------------------------------------
def test_colored_ply_writer_default_bytes_and_double_round_trip(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(12)
    v = rng.rand(6, 3) * 40.0 + np.array([512345.0, 5403210.0, 310.0])
    f = np.array([[0, 1, 2], [2, 3, 4], [3, 4, 5]], dtype=np.int64)
    rgb = rng.randint(0, 256, size=(6, 3)).astype(np.uint8)
    path = str(tmp_path / 's.ply')
    meshio.write_ply_mesh_colored(path, v, f, rgb)
    want = ('ply\nformat binary_little_endian 1.0\ncomment ppsurf_amd\nelement vertex 6\nproperty float x\nproperty float y\nproperty float z\n'
            'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face 3\n'
            'property list uchar int vertex_indices\nend_header\n').encode('ascii')
    for p, c in zip(v, rgb):
        want += struct.pack('<3f4B', *[float(x) for x in p.astype(np.float32)], int(c[0]), int(c[1]), int(c[2]), 255)
    for tri in f:
        want += struct.pack('<B3i', 3, *[int(x) for x in tri])
    assert open(path, 'rb').read() == want
    path = str(tmp_path / 'd.ply')
    rgba = np.concatenate([rgb, rng.randint(0, 256, size=(6, 1)).astype(np.uint8)], axis=1)
    meshio.write_ply_mesh_colored(path, v, f, rgba, double=True)
    assert b'property double x' in open(path, 'rb').read(200)
    got_v, got_f = meshio.read_ply_mesh(path, dtype=np.float64)
    assert np.array_equal(got_v, v) and np.array_equal(got_f, f)
    assert np.array_equal(meshio.read_ply_vertex_colors(path), rgb)
    assert np.array_equal(meshio._ply_vertex_columns(path)['alpha'], rgba[:, 3])


# ---- properties of the specification -----------------------------------------------------------------------------------------------------------
def _scene(n=20000, m=1500, hits=1000, seed=13):
    rng = np.random.RandomState(seed)
    cloud = rng.rand(n, 3).astype(np.float32)
    rgb = rng.randint(0, 256, size=(n, 3)).astype(np.uint8)
    verts = rng.rand(m, 3).astype(np.float32)
    verts[:hits] = cloud[rng.permutation(n)[:hits]]
    return cloud, rgb, verts


def test_spec_neighbours_against_float64_brute_force():
    cloud, _, verts = _scene(n=3000, m=200, hits=50)
    idx, d2 = T.knn(cloud, verts, 9)
    ref = ((verts[:, None, :].astype(np.float64) - cloud[None].astype(np.float64)) ** 2).sum(axis=2)
    assert np.all(np.diff(d2.astype(np.float64), axis=1) >= 0) and np.array_equal(d2[:50, 0], np.zeros(50, dtype=np.float32))
    assert np.allclose(np.sort(ref, axis=1)[:, :9], d2, rtol=1e-5, atol=1e-12)
    same = idx == np.argsort(ref, axis=1, kind='stable')[:, :9]
    assert same.mean() > 0.99                                                        # float32 rounding may swap near ties, nothing more


def test_spec_exact_hit_takes_the_hits_colour():
    """1000 vertices that ARE cloud points: eps = 1e-30 lets the hit outweigh every other neighbour by ~1e18 and nothing is infinite."""
    cloud, rgb, verts = _scene()
    idx, d2 = T.knn(cloud, verts[:1000], 8)
    assert np.all(d2[:, 0] == 0) and np.all(d2[:, 1] > 0)
    rgba = np.concatenate([rgb, np.full((rgb.shape[0], 1), 255, dtype=np.uint8)], axis=1)
    out = T.blend(idx, d2, rgba)
    assert np.array_equal(out, rgba[idx[:, 0]])
    assert np.all(np.isfinite(1.0 / (d2.astype(np.float64) + T.EPS)))


def test_spec_constant_cloud_and_neighbour_bounds():
    cloud, rgb, verts = _scene(n=5000, m=400, hits=100)
    const = np.tile(np.array([[17, 200, 255]], dtype=np.uint8), (cloud.shape[0], 1))
    out, near = T.transfer(cloud, const, verts, k=8)
    assert np.array_equal(out, np.tile(np.array([[17, 200, 255, 255]], dtype=np.uint8), (verts.shape[0], 1)))
    assert near.dtype == np.float32 and np.all(near[:100] == 0)
    idx, d2 = T.knn(cloud, verts, 8)
    out, _ = T.transfer(cloud, rgb, verts, k=8)
    nb = rgb[idx]                                                                   # [m, k, 3]
    assert np.all(out[:, :3] >= nb.min(axis=1)) and np.all(out[:, :3] <= nb.max(axis=1)) and np.all(out[:, 3] == 255)
    one, _ = T.transfer(cloud, rgb, verts, k=1)                                     # k = 1 is nearest-point transfer
    assert np.array_equal(one[:, :3], rgb[idx[:, 0]])


def test_spec_skips_bad_indices_and_rounds_half_up():
    rgba = np.array([[10, 20, 30, 255], [11, 21, 31, 255], [200, 100, 0, 255]], dtype=np.uint8)
    idx = np.array([[0, 1], [-1, 2], [3, 1 << 40], [1, 0]], dtype=np.int64)
    d2 = np.array([[0.25, 0.25], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]], dtype=np.float32)
    out = T.blend(idx, d2, rgba)
    assert out[0].tolist() == [11, 21, 31, 255]                                     # equal weights: 10.5 -> 11
    assert out[1].tolist() == [200, 100, 0, 255]                                    # the invalid entry is skipped although its d2 is 0
    assert out[2].tolist() == [0, 0, 0, 0]                                          # no valid neighbour
    assert out[3].tolist() == [11, 21, 31, 255]                                     # two exact hits: equal weights 1e30


# ---- the extension header of the C ABI ---------------------------------------------------------------------------------------------------------
def test_extension_header_library_and_table_agree():
    from ppsurf_amd import _lib
    from test_decoder_plan_cpu import _exported_symbols
    header = open(os.path.join(REPO, 'include', 'ppsurf_amd_ext.h')).read()
    exported = {n for n in _exported_symbols(_lib.LIB_PATH) if n.startswith('ppsx_')}
    assert exported, 'no extension entry in the dynamic symbol table'
    assert exported == set(re.findall(r'\b(ppsx_[a-z0-9_]+)\s*\(', header)) == set(_lib.EXT_SIGNATURES.keys())
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES) and not any(n.startswith('ppsx_') for n in _lib.SIGNATURES)
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.EXT_SIGNATURES['ppsx_blend_rgba_u8'] == (I, [P, P, I64, I, P, I64, ctypes.c_double, P, P])
    assert _lib.EXT_PARAMS['ppsx_blend_rgba_u8'] == ['idx', 'd2', 'm', 'k', 'rgba', 'n', 'eps', 'out', 'stream']
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2
    assert set(_lib._ext_entries) == exported and not set(_lib._entries) & exported  # bound by lib(), not by bind()
    # the one-argument form of the parser is what it was, and a prefix selects the other set
    text = 'int pps_a(int n);\nint ppsx_b(const uint8_t* p, double e, void* stream);'
    assert set(_lib.parse_header(text)[0]) == {'pps_a'}
    sig, names = _lib.parse_header(text, prefix='ppsx_')
    assert sig == {'ppsx_b': (I, [P, ctypes.c_double, P])} and names == {'ppsx_b': ['p', 'e', 'stream']}


def test_every_extension_call_site_names_a_declared_entry_with_its_argument_count():
    from ppsurf_amd import _lib
    checked = 0
    for path in sorted(glob.glob(os.path.join(REPO, 'ppsurf_amd', '*.py'))):
        text = open(path).read()
        for name in re.findall(r'\bcall\(\s*[\'"](ppsx_\w+)[\'"]', text):
            assert name in _lib.EXT_SIGNATURES, '{}: {} is not declared'.format(path, name)
            assert _lib.EXT_SIGNATURES[name][0] is ctypes.c_int, '{}: {} returns no status'.format(path, name)
        for node in ast.walk(ast.parse(text)):
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'call' and node.args
                    and isinstance(node.args[0], ast.Constant) and str(node.args[0].value).startswith('ppsx_')):
                name = node.args[0].value
                assert not any(isinstance(a, ast.Starred) for a in node.args)
                declared = len(_lib.EXT_PARAMS[name]) - (_lib.EXT_PARAMS[name][-1:] == ['stream'])
                assert len(node.args) - 1 == declared, '{}:{}: {} takes {} arguments besides the stream'.format(path, node.lineno, name, declared)
                checked += 1
    assert checked >= 1


def test_an_undeclared_extension_entry_is_refused():
    from ppsurf_amd import _lib
    with pytest.raises(_lib.PpsError, match=r'ppsx_blend_rgbx_u8 is not declared in .*ppsurf_amd_ext\.h'):
        _lib.call('ppsx_blend_rgbx_u8', 1)
    with pytest.raises(_lib.PpsError, match=r'pps_gather_maxx_f32 is not declared in .*ppsurf_amd\.h'):
        _lib.call('pps_gather_maxx_f32', 1)


def test_models_take_gen_color_k():
    from source.poco_model import PocoModel
    from source.ppsurf_model import PPSurfModel
    kw = dict(output_names=['imp_surf_sign'], in_channels=3, out_channels=2, k=64, lambda_l1=0.0, debug=False,
              in_file='datasets/abc_minimal/testset.txt', results_dir='results', padding_factor=0.05, name='m', network_latent_size=32,
              gen_subsample_manifold_iter=10, gen_subsample_manifold=10000, gen_resolution_global=129, rec_batch_size=25000, gen_refine_iter=10,
              workers=0)
    pps = dict(kw, pointnet_latent_size=32, num_pts_local=50)
    assert PocoModel(**kw).gen_color_k is None and PPSurfModel(**pps).gen_color_k is None
    assert PocoModel(gen_color_k=8, **kw).gen_color_k == 8 and PPSurfModel(gen_color_k=1, gen_max_faces=100, **pps).gen_color_k == 1
    for bad in (0, -1, 257):
        with pytest.raises(ValueError, match='gen_color_k'):
            PocoModel(gen_color_k=bad, **kw)
        with pytest.raises(ValueError, match='gen_color_k'):
            PPSurfModel(gen_color_k=bad, **pps)
