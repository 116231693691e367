"""Host tier of the mesh simplification: the numpy specification tests/simplify_spec.py against independent formulations
(np.unique on the fp64 cell triples, np.linalg.solve, a brute-force leader search), the geometric conditions that follow from the construction, the
budget bound, and the argument handling of ppsurf_amd.simplify and of the models."""
import os

import numpy as np
import pytest
import torch

import simplify_spec as S
import vis_spec
from golden_util import GOLDEN

ABC_MESH = os.path.join(GOLDEN, 'abc_minimal_gt', '03_meshes', '00010009_d97409455fa543b3a224250f_trimesh_000.ply')
CUBE_FACES = {8: 768, 16: 3072, 24: 6912}
SQRT3 = np.sqrt(3.0)


def abc_mesh(subdivisions=1):
    from ppsurf_amd import meshio, visualization
    v, f = meshio.read_ply_mesh(ABC_MESH)
    v, f = torch.from_numpy(v.astype(np.float64)), torch.from_numpy(f.astype(np.int64))
    for _ in range(subdivisions):
        v, f = visualization.subdivide(v, f)
    return v.numpy(), f.numpy()


def sphere_volume(R):
    """The analytic sphere of DESIGN section 9 (radius 0.35 in the box [-0.5, 0.5]^3, inside > 0) on an R^3 grid."""
    g = np.linspace(-0.5, 0.5, R)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    return 0.35 - np.sqrt(x * x + y * y + z * z)


def sphere_mesh(R=33):
    """Its Marching Cubes mesh (host path of marching_cubes_torch) in the box's coordinates."""
    from ppsurf_amd import mcubes
    v, f = mcubes.marching_cubes(sphere_volume(R), 0.0)
    return v.astype(np.float64) * (1.0 / (R - 1)) - 0.5, f.astype(np.int64)


def awkward_mesh():
    """Exact duplicate vertices, degenerate faces (a repeated index, three equal positions), duplicate faces, an unreferenced vertex, and
    vertices exactly on the walls of the h = 0.25 grid (multiples of 1/4 are exact)."""
    rng = np.random.RandomState(31)
    base = (rng.randint(0, 9, size=(300, 3)) / 8.0)
    verts = np.concatenate([base, base[:60], [[2.0, 2.0, 2.0]]])
    faces = rng.randint(0, 360, size=(900, 3))
    faces = np.concatenate([faces, faces[:50], faces[50:80][:, [1, 2, 0]], [[5, 5, 9], [7, 7, 7], [3, 303, 40]]])
    return verts.astype(np.float64), faces.astype(np.int64)


def on_wall_mesh():
    """A strip whose middle row of vertices lies exactly on a cell wall of the G = 4 grid (x = 0.5 with lo = 0, ext = 1)."""
    xs = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    ys = np.linspace(0.0, 0.5, 7)
    verts = np.array([[x, y, 0.1 * x * y] for x in xs for y in ys])
    idx = lambda i, j: i * 7 + j
    faces = [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(4) for j in range(6)] + \
            [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(4) for j in range(6)]
    return verts, np.array(faces, dtype=np.int64)


def check_geometry(verts, faces, out, closest):
    """Conditions 1 and 2 of DESIGN section 13 on a specification / device result `out` (dict with h, verts, cid, used).  `closest(queries)` ->
    distances to the INPUT surface."""
    h = out['h']
    d = np.asarray(closest(out['verts']), dtype=np.float64)
    print('output vertex to input surface: max {:.4f} h (bound {:.4f} h)'.format(d.max() / h, SQRT3))
    assert d.max() <= SQRT3 * h
    remap = np.cumsum(out['used']) - 1
    kept = out['used'][out['cid']]
    target = out['verts'][remap[out['cid'][kept]]]
    d2 = np.sqrt(((np.asarray(verts, dtype=np.float64)[kept] - target) ** 2).sum(axis=1))
    print('input vertex to its output vertex: max {:.4f} h, rms {:.4f} h'.format(d2.max() / h, np.sqrt((d2 * d2).mean()) / h))
    assert d2.max() <= SQRT3 * h


@pytest.mark.parametrize('name', ['cube', 'abc', 'awkward', 'wall'])
def test_cells_and_leaders_against_unique(name):
    verts, faces = {'cube': lambda: S.cube_mesh(31), 'abc': lambda: abc_mesh(0), 'awkward': awkward_mesh, 'wall': on_wall_mesh}[name]()
    lo, hi, ext = S.box(verts)
    for G in (1, 4, 7, 32, 1000):
        h, inv_h = S.grid_step(ext, G)
        c, dims, key = S.cells(verts, lo, hi, inv_h)
        assert (c >= 0).all() and (c < dims[None]).all()
        triples, inv = np.unique(np.minimum(np.floor((verts - lo) * inv_h), dims - 1.0), axis=0, return_inverse=True)
        leader = S.leaders(key)
        cid, ncell = S.cluster_ids(leader)
        assert ncell == triples.shape[0]
        inv = inv.reshape(-1)
        brute = np.full(ncell, verts.shape[0], dtype=np.int64)
        np.minimum.at(brute, inv, np.arange(verts.shape[0]))
        assert np.array_equal(leader, brute[inv])
        assert np.array_equal(cid, np.argsort(np.argsort(brute))[inv])               # clusters are numbered by ascending leader
        fl = leader[faces]
        want = int(((fl[:, 0] != fl[:, 1]) & (fl[:, 1] != fl[:, 2]) & (fl[:, 0] != fl[:, 2])).sum())
        assert S.count(verts, faces, G) == want
    if name == 'wall':
        c, _, _ = S.cells(verts, lo, hi, S.grid_step(ext, 4)[1])
        assert set(c[np.asarray(verts)[:, 0] == 0.5, 0]) == {2}                       # a vertex on a wall belongs to the cell above it


def test_segment_sums_are_sequential():
    rng = np.random.RandomState(5)
    ids = rng.randint(0, 40, size=3000)
    vals = rng.randn(3000, 2) * 10.0 ** rng.randint(-8, 8, size=(3000, 1))
    order, off = S.segments(ids, 40)
    got = S.segment_sums(vals, order, off)
    for r in range(40):
        acc = np.zeros(2)
        for e in np.nonzero(ids == r)[0]:
            acc = acc + vals[e]
        assert np.array_equal(got[r], acc)


@pytest.mark.parametrize('name,G', [('cube', 16), ('abc', 24), ('sphere', 12), ('awkward', 4)])
def test_placement_against_linalg_solve(name, G):
    verts, faces = {'cube': lambda: S.cube_mesh(48), 'abc': lambda: abc_mesh(1), 'sphere': sphere_mesh, 'awkward': awkward_mesh}[name]()
    out = S.simplify(verts, faces, G)
    A6, b, xhat = out['A'], out['b'], out['xhat']
    A = A6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    trace = A6[:, 0] + A6[:, 3] + A6[:, 5]
    live = trace > 0
    lam = 1e-3 * trace[live]
    M = A[live] + lam[:, None, None] * np.eye(3)[None]
    ref = np.linalg.solve(M, (b[live] + lam[:, None] * xhat[live])[:, :, None])[:, :, 0]
    got, fell = S.place(A6, b, xhat, out['h'])
    # the system's condition is at most (trace + lambda) / lambda ~ 1e3: an fp64 solve loses three of sixteen digits
    inside = ~fell[live]
    err = np.linalg.norm(got[live][inside] - ref[inside], axis=1) / np.linalg.norm(ref[inside], axis=1)
    print('{} G={}: {} cells, {} fall back, largest relative deviation from np.linalg.solve {:.3g}'.format(name, G, A.shape[0], int(fell.sum()), err.max()))
    assert err.max() <= 1e-9
    # fall-backs: exactly the cells whose optimum lies outside the cell, wherever np.linalg.solve is not within its own error of a wall
    wall = 0.5 * out['h'] * (1 + 2.0 ** -30)
    reach = np.abs(ref).max(axis=1)
    clear = np.abs(reach - wall) > 1e-9 * out['h']
    assert np.array_equal(fell[live][clear], (reach > wall)[clear])
    assert fell[~live].all() and np.array_equal(got[fell], xhat[fell])
    mean, none = S.place(A6, b, xhat, out['h'], 'mean')
    assert np.array_equal(mean, xhat) and not none.any()
    # the quadrics themselves against a plain float64 accumulation in another order
    fc = out['cid'][faces]
    for c in np.random.RandomState(1).choice(A.shape[0], size=min(40, A.shape[0]), replace=False):
        touching = np.nonzero((fc == c).any(axis=1))[0]
        q = verts[faces[touching]] - out['centre'][c]
        n = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        m = (n * q[:, 0]).sum(axis=1)
        np.testing.assert_allclose(A[c], (n[:, :, None] * n[:, None, :]).sum(axis=0), rtol=0, atol=1e-12 * trace[c])
        np.testing.assert_allclose(b[c], (m[:, None] * n).sum(axis=0), rtol=0, atol=1e-12 * max(np.abs(m[:, None] * n).sum(), 1e-300))
        np.testing.assert_allclose(xhat[c], (verts[out['cid'] == c] - out['centre'][c]).mean(axis=0), rtol=1e-9, atol=1e-13 * out['h'])


def test_faces_are_remapped_deduplicated_and_compacted():
    verts, faces = awkward_mesh()
    out = S.simplify(verts, faces, h=0.25)
    new = out['cid'][faces]
    alive = (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 0] != new[:, 2])
    assert out['survivors'] == int(alive.sum()) > out['faces_out'] > 0
    seen, want = set(), []
    for row in new[alive]:
        key = tuple(sorted(row.tolist()))
        if key not in seen:
            seen.add(key)
            want.append(row)
    ids = np.nonzero(out['used'])[0]
    assert np.array_equal(ids[out['faces']], np.array(want))                          # first of every unordered triple, order kept
    assert np.array_equal(np.unique(out['faces']), np.arange(out['verts_out']))        # no unreferenced vertex
    assert np.array_equal(out['verts'], out['pos'][ids])


@pytest.mark.parametrize('G', [8, 16, 24])
def test_cube_fixture(G):
    """Condition 3 of DESIGN section 13."""
    verts, faces = S.cube_mesh(97)
    assert verts.shape == (56456, 3) and faces.shape == (112908, 3)
    quadric, mean = S.simplify(verts, faces, G), S.simplify(verts, faces, G, 'mean')
    h = quadric['h']
    dq, dm = S.cube_surface_distance(quadric['verts']).max(), S.cube_surface_distance(mean['verts']).max()
    print('cube G={}: quadric {:.5f} h, mean {:.5f} h from the surface; fallback {}, flipped {}'.format(G, dq / h, dm / h, quadric['fallback'],
                                                                                                 quadric['flipped']))
    assert quadric['fallback'] == 0 and quadric['flipped'] == 0
    assert quadric['faces_out'] == mean['faces_out'] == CUBE_FACES[G]
    assert dq <= dm / 100.0


@pytest.mark.parametrize('name,G', [('cube', 16), ('abc', 20), ('sphere', 10)])
@pytest.mark.parametrize('placement', ['quadric', 'mean'])
def test_geometric_conditions_on_the_spec(name, G, placement):
    verts, faces = {'cube': lambda: S.cube_mesh(40), 'abc': lambda: abc_mesh(0), 'sphere': sphere_mesh}[name]()
    out = S.simplify(verts, faces, G, placement)
    assert out['faces_out'] > 0
    check_geometry(verts, faces, out, lambda q: vis_spec.closest_point_spec(verts, faces, q, chunk=64)[0])


@pytest.mark.parametrize('budget', [500, 5000, 50000])
def test_budget_bound(budget):
    verts, faces = S.cube_mesh(97)
    counted = {}

    def count(G):
        counted[G] = S.count(verts, faces, G)
        return counted[G]

    G = S.budget_search(verts, faces, budget, count)
    assert len(counted) == 20 and counted[G] <= budget < counted[G + 1]
    out = S.simplify(verts, faces, G)
    print('budget {}: G = {}, count {}, faces_out {}'.format(budget, G, counted[G], out['faces_out']))
    assert out['survivors'] == counted[G] and out['faces_out'] <= counted[G] <= budget
    assert S.simplify_budget(verts, faces, faces.shape[0]) is None                    # within the budget: unchanged


def test_degenerate_inputs():
    one = np.tile(np.array([[1.0, 2.0, 3.0]]), (5, 1))
    out = S.simplify(one, np.array([[0, 1, 2]]), 4)
    assert out['faces_out'] == 0 and out['verts'].shape == (0, 3) and S.count(one, np.array([[0, 1, 2]]), 4) == 0
    verts, faces = sphere_mesh(17)
    out = S.simplify(verts, faces, 1)                # the top layers hold the three poles only: no face has corners in three cells
    assert out['cells'] <= 4 and out['survivors'] == 0 and out['faces'].shape == (0, 3)
    lo, hi, ext = S.box(verts)
    assert S.grid_dims(lo, hi, 1.0 / (ext / (1 << 21))) is None


def test_simplify_mesh_arguments():
    from ppsurf_amd import simplify
    from ppsurf_amd._lib import PpsError
    v, f = np.zeros((10, 3)), np.zeros((4, 3), dtype=np.int64)
    with pytest.raises(PpsError, match='no CPU'):
        simplify.simplify_mesh(torch.zeros(10, 3), torch.zeros(4, 3, dtype=torch.int64), max_faces=2)
    with pytest.raises(PpsError, match='no CPU'):
        simplify.simplify_mesh(v, f, max_faces=2, device='cpu')
    with pytest.raises(PpsError):
        simplify.ClusterGrid(torch.zeros(10, 3), torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match='exclude'):
        simplify.simplify_mesh(v, f, max_faces=2, voxel_size=0.1)
    with pytest.raises(ValueError, match='exclude'):
        simplify.simplify_mesh(v, f)
    with pytest.raises(ValueError):
        simplify.simplify_mesh(v, f, voxel_size=0.0)
    with pytest.raises(ValueError):
        simplify.simplify_mesh(v, f, max_faces=-1)
    with pytest.raises(ValueError, match='placement'):
        simplify.simplify_mesh(v, f, max_faces=2, placement='median')


@pytest.mark.parametrize('argv', [['in.ply', 'out.ply'], ['in.ply', 'out.ply', '--max_faces', '10', '--voxel_size', '0.1'],
                                  ['in.ply', 'out.ply', '--max_faces', '-3'], ['in.ply', 'out.ply', '--voxel_size', '0'],
                                  ['in.ply', 'out.ply', '--max_faces', '10', '--placement', 'median'], ['in.stl', 'out.ply', '--max_faces', '10'],
                                  ['in.ply', 'out.obj', '--max_faces', '10'], ['in.ply']])
def test_cli_argument_errors(argv, capsys):
    from ppsurf_amd import simplify
    with pytest.raises(SystemExit) as e:
        simplify.main(argv)
    assert e.value.code == 2
    assert 'usage' in capsys.readouterr().err


def test_models_take_gen_max_faces():
    from source.poco_model import PocoModel
    from source.ppsurf_model import PPSurfModel
    kw = dict(output_names=['imp_surf_sign'], in_channels=3, out_channels=2, k=64, lambda_l1=0.0, debug=False,
              in_file='datasets/abc_minimal/testset.txt', results_dir='results', padding_factor=0.05, name='m', network_latent_size=32,
              gen_subsample_manifold_iter=10, gen_subsample_manifold=10000, gen_resolution_global=129, rec_batch_size=25000, gen_refine_iter=10,
              workers=0)
    pps = dict(kw, pointnet_latent_size=32, num_pts_local=50)
    assert PocoModel(**kw).gen_max_faces is None and PPSurfModel(**pps).gen_max_faces is None
    assert PocoModel(gen_max_faces=100000, **kw).gen_max_faces == 100000 and PPSurfModel(gen_max_faces=4, **pps).gen_max_faces == 4
    for bad in (3, 0, -1):
        with pytest.raises(ValueError, match='gen_max_faces'):
            PocoModel(gen_max_faces=bad, **kw)
        with pytest.raises(ValueError, match='gen_max_faces'):
            PPSurfModel(gen_max_faces=bad, **pps)
    import inspect
    from ppsurf_amd import reconstruct
    params = list(inspect.signature(reconstruct.export_mesh_and_refine_vertices_region_growing_v3).parameters)
    assert params[-1] == 'max_faces'


def test_abi_declares_the_simplify_entries():
    from ppsurf_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'ppsurf_amd.h')).read()
    for name in ('pps_simplify_leaders', 'pps_simplify_count', 'pps_simplify_place'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().pps_abi_version() == 2
