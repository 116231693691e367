"""Host tier of the cloud preparation: the readers of ppsurf_amd/meshio.py against files written here with `struct`
from the published layouts, and the numpy specification tests/cloud_spec.py against independent routes (np.unique on float64 cells, scipy's
kd-tree).  No GPU."""
import os
import struct

import numpy as np
import pytest

import cloud_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
ABC = os.path.join(HERE, 'golden', 'abc_minimal_testset', '04_pts_vis', '00010009_d97409455fa543b3a224250f_trimesh_000.xyz.ply')


# ---- writers of the test files ---------------------------------------------------------------------------------------------------------------
def write_las(path, ints, scale, offset, version=(1, 2), fmt=1):
    """Uncompressed LAS from the public header block of the ASPRS specification; ints int32 [n,3]."""
    n = ints.shape[0]
    rec_len = {0: 20, 1: 28, 2: 26, 3: 34, 6: 30, 7: 36}[fmt]
    header_size = {2: 227, 3: 235, 4: 375}[version[1]]
    vlr = b'\x5a' * 54 if version[1] < 4 else b''                 # something between header and points: the offset field must be honoured
    head = bytearray(header_size)
    head[0:4] = b'LASF'
    head[24], head[25] = version
    struct.pack_into('<HI', head, 94, header_size, header_size + len(vlr))
    struct.pack_into('<I', head, 100, 0)
    legacy = 0 if version[1] >= 4 else n
    struct.pack_into('<BHI', head, 104, fmt, rec_len, legacy)
    struct.pack_into('<3d', head, 131, *scale)
    struct.pack_into('<3d', head, 155, *offset)
    if version[1] >= 4:
        struct.pack_into('<Q', head, 247, n)
    body = bytearray(n * rec_len)
    for i in range(n):
        struct.pack_into('<3i', body, i * rec_len, *[int(v) for v in ints[i]])
        for b in range(12, rec_len):
            body[i * rec_len + b] = (37 * i + b) & 0xFF          # the rest of the record is not zero
    with open(path, 'wb') as f:
        f.write(bytes(head) + vlr + bytes(body))


def las_case(seed, n=500):
    rng = np.random.RandomState(seed)
    ints = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(n, 3)).astype(np.int32)
    ints[:, 2] = rng.randint(-50000, 50000, size=n)
    scale = (0.001, 0.0025, 0.01)
    offset = (512345.0, 5403210.0, 310.0)
    return ints, scale, offset


@pytest.mark.parametrize('version,fmt', [((1, 2), 1), ((1, 4), 6)])
def test_las_reader(tmp_path, version, fmt):
    from ppsurf_amd import meshio
    ints, scale, offset = las_case(fmt)
    path = str(tmp_path / 'scan.las')
    write_las(path, ints, scale, offset, version, fmt)
    got = meshio.load_pts(path)
    want = ints.astype(np.float64) * np.array(scale)[None] + np.array(offset)[None]
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want)


def test_compressed_las_is_refused(tmp_path):
    from ppsurf_amd import meshio
    for ext in ('.laz', '.copc', '.crs'):
        path = str(tmp_path / ('scan' + ext))
        open(path, 'wb').write(b'LASF')
        with pytest.raises(ValueError, match=r'compressed LAS is not supported.*\.las.*\.npy'):
            meshio.load_pts(path)


def test_stl_readers(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(3)
    tri = rng.randn(7, 3, 3).astype(np.float32)
    tri[3] = tri[2]                                              # duplicates are kept
    with open(tmp_path / 'b.stl', 'wb') as f:
        f.write(b'solid looks ascii but is binary'.ljust(80, b' ') + struct.pack('<I', tri.shape[0]))
        for t in tri:
            f.write(struct.pack('<3f', 0.0, 0.0, 1.0) + struct.pack('<9f', *t.reshape(-1)) + struct.pack('<H', 0))
    got = meshio.load_pts(str(tmp_path / 'b.stl'))
    assert got.shape == (21, 3) and np.array_equal(got, tri.reshape(-1, 3).astype(np.float64))
    with open(tmp_path / 'a.stl', 'w') as f:
        f.write('solid test\n')
        for t in tri:
            f.write(' facet normal 0 0 1\n  outer loop\n')
            for v in t:
                f.write('   vertex {!r} {!r} {!r}\n'.format(*[float(x) for x in v]))
            f.write('  endloop\n endfacet\n')
        f.write('endsolid test\n')
    got = meshio.load_pts(str(tmp_path / 'a.stl'))
    assert np.array_equal(got, tri.reshape(-1, 3).astype(np.float64))


def test_off_and_obj_readers(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(4)
    v = rng.randn(9, 3)
    with open(tmp_path / 'm.off', 'w') as f:
        f.write('OFF\n# a comment\n9 2 0\n' + ''.join('{!r} {!r} {!r}\n'.format(*map(float, p)) for p in v) + '3 0 1 2\n4 3 4 5 6\n')
    assert np.array_equal(meshio.load_pts(str(tmp_path / 'm.off')), v)
    with open(tmp_path / 'c.off', 'w') as f:
        f.write('COFF 9 1 0\n' + ''.join('{!r} {!r} {!r} 255 0 0 255\n'.format(*map(float, p)) for p in v) + '3 0 1 2\n')
    assert np.array_equal(meshio.load_pts(str(tmp_path / 'c.off')), v)
    with open(tmp_path / 'm.obj', 'w') as f:
        f.write('# obj\n' + ''.join('v {!r} {!r} {!r}\n'.format(*map(float, p)) for p in v) + 'vn 0 0 1\nf 1//1 2//1 3//1\n')
    got = meshio.load_pts(str(tmp_path / 'm.obj'))
    assert got.shape == (9, 3) and np.array_equal(got, v.astype(np.float32))          # read_obj_mesh stores float32


def test_pcd_readers(tmp_path):
    from ppsurf_amd import meshio
    rng = np.random.RandomState(5)
    xyz = rng.randn(11, 3).astype(np.float32)
    inten = rng.rand(11).astype(np.float32)
    head = ('# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS intensity x y z\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n'
            'WIDTH 11\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 11\nDATA {}\n')
    with open(tmp_path / 'a.pcd', 'w') as f:
        f.write(head.format('ascii') + ''.join('{!r} {!r} {!r} {!r}\n'.format(float(i), *map(float, p)) for i, p in zip(inten, xyz)))
    got = meshio.load_pts(str(tmp_path / 'a.pcd'))
    assert got.dtype == np.float32 and np.array_equal(got, xyz)
    with open(tmp_path / 'b.pcd', 'wb') as f:
        f.write(head.format('binary').encode('ascii'))
        for i, p in zip(inten, xyz):
            f.write(struct.pack('<4f', i, *p))
    assert np.array_equal(meshio.load_pts(str(tmp_path / 'b.pcd')), xyz)
    # 8-byte coordinates beside a 1-byte label and a 3-count field: float64 out
    xyz8 = rng.randn(6, 3) * 1e6
    head8 = 'VERSION 0.7\nFIELDS x y z label rgb3\nSIZE 8 8 8 1 2\nTYPE F F F U I\nCOUNT 1 1 1 1 3\nWIDTH 3\nHEIGHT 2\nDATA binary\n'
    with open(tmp_path / 'd.pcd', 'wb') as f:
        f.write(head8.encode('ascii'))
        for j, p in enumerate(xyz8):
            f.write(struct.pack('<3dB3h', *p, j, 1, 2, 3))
    got = meshio.load_pts(str(tmp_path / 'd.pcd'))
    assert got.dtype == np.float64 and np.array_equal(got, xyz8)


def test_unknown_type_still_raises(tmp_path):
    from ppsurf_amd import meshio
    with pytest.raises(ValueError, match='Unknown point cloud type'):
        meshio.load_pts(str(tmp_path / 'x.xlsx'))


def test_double_ply_mesh_round_trip(tmp_path):
    from ppsurf_amd import meshio
    v = np.random.RandomState(6).rand(8, 3) * 40.0 + np.array([512345.0, 5403210.0, 310.0])
    f = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int64)
    meshio.write_ply_mesh(str(tmp_path / 'd.ply'), v, f, double=True)
    assert b'property double x' in open(tmp_path / 'd.ply', 'rb').read(200)
    got_v, got_f = meshio.read_ply_mesh(str(tmp_path / 'd.ply'), dtype=np.float64)
    assert np.array_equal(got_v, v) and np.array_equal(got_f, f)
    v32, _ = meshio.read_ply_mesh(str(tmp_path / 'd.ply'))                           # evaluation and comparison read float32, as before
    assert v32.dtype == np.float32 and np.array_equal(v32, v.astype(np.float32))
    meshio.write_ply_mesh(str(tmp_path / 's.ply'), v, f)
    assert b'property float x' in open(tmp_path / 's.ply', 'rb').read(200)


# ---- the specification against independent routes --------------------------------------------------------------------------------------------
def clouds(n, seed):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 3)
    sphere = d / np.linalg.norm(d, axis=1, keepdims=True)
    u, v = rng.rand(n) * 2 * np.pi, rng.rand(n) * 2 * np.pi
    torus = np.stack([(1.0 + 0.3 * np.cos(v)) * np.cos(u), (1.0 + 0.3 * np.cos(v)) * np.sin(u), 0.3 * np.sin(v)], axis=1) + 0.01 * rng.randn(n, 3)
    cube = rng.rand(n, 3) * 2 - 1
    face = rng.randint(0, 6, size=n)
    cube[np.arange(n), face % 3] = np.where(face < 3, -1.0, 1.0)
    return {'sphere': sphere.astype(np.float32), 'torus': torus.astype(np.float32), 'cube': cube.astype(np.float32)}


def test_cells_against_float64_unique():
    rng = np.random.RandomState(7)
    pts = (rng.rand(20000, 3) * np.array([1.0, 0.7, 0.4])).astype(np.float32)
    lo, hi, ext = S.box(pts)
    for G in (5, 37, 300):
        h, inv_h = S.grid_step(ext, G)
        t = (pts.astype(np.float64) - lo.astype(np.float64)) / np.float64(h)
        margin = np.abs(t - np.rint(t))
        ok = (margin >= 1e-4).all(axis=1)                        # points at least 1e-4 h away from every cell wall: float32 and float64 agree
        sub = pts[ok]
        # box corners stay in, so that the grid of the subset is the grid of the cloud
        sub = np.concatenate([sub, lo[None], hi[None]])
        t = (sub[:-2].astype(np.float64) - lo.astype(np.float64)) / np.float64(h)
        assert (np.abs(t - np.rint(t)) >= 1e-4).all()
        c, dims, key = S.cells(sub, lo, hi, h, inv_h)
        c64 = np.floor(t).astype(np.int64)
        assert np.array_equal(c[:-2], c64)
        _, inv64 = np.unique(c64, axis=0, return_inverse=True)
        _, inv32 = np.unique(key[:-2], return_inverse=True)
        # the same partition into cells: equal pairs of labels
        assert np.unique(np.stack([inv64.reshape(-1), inv32.reshape(-1)], axis=1), axis=0).shape[0] == inv64.max() + 1 == inv32.max() + 1
        sel = S.voxel_select(sub, lo, hi, h, inv_h)
        assert np.all(np.diff(sel) > 0) and sel.shape[0] == S.voxel_count(sub, lo, hi, h, inv_h)
        # a kept point is one of its cell's own, and no point of the cell is nearer to the centre (float64 check with float32 slack)
        centre = lo.astype(np.float64) + (c.astype(np.float64) + 0.5) * np.float64(h)
        d = np.linalg.norm(sub.astype(np.float64) - centre, axis=1)
        best = np.full(key.max() + 1, np.inf) if key.max() < 10 ** 7 else None
        if best is not None:
            np.minimum.at(best, key, d)
            assert np.all(d[sel] <= best[key[sel]] + 1e-6 * float(h))
            assert np.array_equal(np.sort(key[sel]), np.unique(key))


def test_tie_and_duplicates_in_the_spec():
    h = np.float32(0.5)
    pts = np.array([[0.125, 0.25, 0.25], [0.375, 0.25, 0.25], [0.375, 0.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5]], dtype=np.float32)
    lo, hi, _ = S.box(pts)
    sel = S.voxel_select(pts, lo, hi, h, np.float32(1.0) / h)
    # cell 0 holds points 0..3: 0, 1 and 2 are equally far from the centre (0.25, 0.25, 0.25) -> the lowest index; a point on a wall belongs
    # to the cell above it; the point at the upper corner has a cell of its own (G = 3 per axis)
    assert sel.tolist() == [0, 4, 5]


def test_mean_distance_against_kdtree():
    from scipy.spatial import cKDTree
    pts = clouds(6000, 8)['torus']
    k = 16
    for d2 in (S.knn_d2(pts, k + 1), S.knn_d2(pts, k + 1, brute_max=0)):       # brute force and the candidate route agree with the tree
        m = S.mean_dist(d2)
        dist, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=k + 1)
        ref = dist[:, 1:].mean(axis=1)
        assert np.max(np.abs(m - ref) / ref) < 1e-6
    assert np.array_equal(S.knn_d2(pts, k + 1), S.knn_d2(pts, k + 1, brute_max=0))
    mu, sigma, thr = S.outlier_stats(m, 2.0)
    assert abs(mu - m.mean()) < 1e-12 * mu and abs(sigma - m.std()) < 1e-9 * sigma and thr == mu + 2.0 * sigma


@pytest.mark.parametrize('name', ['sphere', 'torus', 'cube'])
def test_budget_search(name):
    pts = clouds(400000, 9)[name]
    for budget in (2000, 20000, 100000):
        idx, G, h = S.subsample(pts, budget)
        print('{} budget {}: G {} h {:.6g} kept {} ({:.3f})'.format(name, budget, G, float(h), idx.shape[0], idx.shape[0] / budget))
        assert idx.shape[0] <= budget
        assert idx.shape[0] >= 0.9 * budget


def planted(seed=10):
    rng = np.random.RandomState(seed)
    d = rng.randn(200000, 3)
    sphere = 0.4 * d / np.linalg.norm(d, axis=1, keepdims=True)
    far = rng.rand(200, 3) * 20.0 - 10.0
    return np.concatenate([sphere, far]).astype(np.float32), 200000


def test_planted_outliers_in_the_spec():
    pts, ns = planted()
    keep, m, stats = S.outlier_keep(pts, 16, 2.0)
    kept = np.zeros(pts.shape[0], dtype=bool)
    kept[keep] = True
    far = np.abs(np.linalg.norm(pts[ns:].astype(np.float64), axis=1) - 0.4) > 1.0
    print('threshold {:.4f}; far planted {} removed {}; sphere removed {}'.format(stats[2], far.sum(), (~kept[ns:][far]).sum(), (~kept[:ns]).sum()))
    assert far.sum() > 150 and not kept[ns:][far].any()
    assert (~kept[:ns]).sum() <= 0.01 * ns
    keep, m, stats = S.outlier_keep(pts[:ns], 16, 2.0)
    print('clean sphere: removed {:.3%}'.format(1 - keep.shape[0] / ns))
    assert ns - keep.shape[0] <= 0.05 * ns


# ---- the library refuses what it cannot do ---------------------------------------------------------------------------------------------------
def test_prepare_cloud_has_no_cpu_path():
    import torch
    from ppsurf_amd import cloud
    from ppsurf_amd._lib import PpsError
    with pytest.raises(PpsError):
        cloud.prepare_cloud(torch.zeros(10, 3), max_points=5)
    with pytest.raises(PpsError):
        cloud.prepare_cloud(np.zeros((10, 3)), max_points=5, device='cpu')
    with pytest.raises(ValueError):
        cloud.prepare_cloud(np.zeros((10, 3)), max_points=5, voxel_size=0.1)


def test_data_modules_reject_preparation_of_a_dataset(tmp_path):
    from ppsurf_amd.data import PocoDataModule, PPSurfDataModule
    args = dict(workers=0, use_ddp=False, padding_factor=0.05, seed=42, manifold_points=1000, patches_per_shape=-1, do_data_augmentation=False,
                batch_size=1)
    txt = str(tmp_path / 'testset.txt')
    for kw in ({'max_points': 1000}, {'voxel_size': 0.01}, {'outlier_k': 16}):
        with pytest.raises(ValueError, match='single-file'):
            PocoDataModule(in_file=txt, **args, **kw)
        with pytest.raises(ValueError, match='single-file'):
            PPSurfDataModule(num_pts_local=50, in_file=txt, **args, **kw)
    PPSurfDataModule(num_pts_local=50, in_file=txt, **args)                         # defaults: nothing changes
    dm = PocoDataModule(in_file=str(tmp_path / 'scan.las'), **args, max_points=1000)
    assert dm.prepare == {'max_points': 1000, 'voxel_size': None, 'outlier_k': 0, 'outlier_ratio': 2.0}
    for loader in (dm.test_dataloader, dm.train_dataloader, dm.val_dataloader):
        with pytest.raises(ValueError, match='predict only'):
            loader()
