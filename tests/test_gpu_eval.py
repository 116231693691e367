"""Mesh evaluation on the GPU (csrc/pps_eval.hip, ppsurf_amd/evaluation.py): the kernels against numpy restatements (tests/eval_spec.py),
the metrics against analytic answers, determinism, and the end-to-end predict -> tables flow of the reference (poco_model.py:275-300)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_spec as E
from golden_util import REPO, filled_sd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLDEN = os.path.join(REPO, 'tests', 'golden')
GT_DIR = os.path.join(GOLDEN, 'abc_minimal_gt', '03_meshes')


def _dev(verts, faces):
    return (torch.as_tensor(np.asarray(verts, dtype=np.float32)).to(DEV).contiguous(),
            torch.as_tensor(np.asarray(faces, dtype=np.int32)).to(DEV).contiguous())


def _fixture(name_index=1):
    from ppsurf_amd import meshio
    names = sorted(os.listdir(GT_DIR))
    return meshio.read_ply_mesh(os.path.join(GT_DIR, names[name_index]))


def test_face_stats_against_numpy():
    from ppsurf_amd import geometry
    verts, faces = _fixture(0)
    faces = np.concatenate([faces, np.array([[0, 0, 1], [5, 5, 5]], np.int32)])             # two degenerate faces at the end
    area, normal, corners = geometry.face_stats(*_dev(verts, faces))
    a_np, n_np, c_np = E.face_stats_spec(verts, faces)
    assert np.array_equal(corners.cpu().numpy(), c_np.astype(np.float32))
    np.testing.assert_allclose(area.cpu().numpy(), a_np, rtol=1e-5, atol=1e-6 * a_np.max())   # fp32 cancellation on slivers
    v = np.asarray(verts, np.float64)[faces]
    sin = 2 * a_np / np.maximum(np.linalg.norm(v[:, 1] - v[:, 0], axis=1) * np.linalg.norm(v[:, 2] - v[:, 0], axis=1), 1e-300)
    well = sin > 1e-2                                          # the normal of a sliver is ill-conditioned in fp32
    assert well.mean() > 0.95
    np.testing.assert_allclose(normal.cpu().numpy()[well], n_np[well], atol=2e-5)
    np.testing.assert_allclose(np.linalg.norm(normal.cpu().numpy()[a_np > 0], axis=1), 1.0, atol=1e-5)
    assert area[-2:].tolist() == [0.0, 0.0] and normal[-2:].abs().sum().item() == 0.0


def test_sampling_matches_the_generator_and_is_a_prefix():
    from ppsurf_amd import geometry
    verts, faces = _fixture(0)
    area, _, corners = geometry.face_stats(*_dev(verts, faces))
    prefix = geometry.area_prefix(area)
    pts, face = geometry.sample_surface(corners, prefix, 50000, seed=7, stream_id=3)
    p_np, f_np = E.sample_spec(corners.cpu().numpy(), prefix.cpu().numpy(), 50000, 7, 3)
    assert np.array_equal(face.cpu().numpy().astype(np.int64), f_np)
    np.testing.assert_allclose(pts.cpu().numpy(), p_np, rtol=0, atol=1e-6)
    pk, fk = geometry.sample_surface(corners, prefix, 1234, seed=7, stream_id=3)
    assert torch.equal(pk, pts[:1234]) and torch.equal(fk, face[:1234])
    p2, _ = geometry.sample_surface(corners, prefix, 1234, seed=7, stream_id=4)
    assert not torch.equal(p2, pk)                                                             # streams are independent draws


def test_sampling_never_draws_zero_area_faces():
    from ppsurf_amd import geometry
    v, f = E.icosphere(2, 0.3)
    nf = f.shape[0]
    degenerate = np.array([[0, 0, 1], [2, 3, 2], [4, 4, 4]])
    faces = np.concatenate([degenerate, f[:nf // 2], degenerate, f[nf // 2:], degenerate])      # first, inside and last
    area, _, corners = geometry.face_stats(*_dev(v, faces))
    zero = (area == 0).cpu().numpy()
    assert zero.sum() == 9
    _, face = geometry.sample_surface(corners, geometry.area_prefix(area), 200000, seed=1)
    assert not zero[face.cpu().numpy()].any()


def test_sampling_face_counts_follow_the_areas():
    """Chi-square of the face counts of 200k samples over 20 faces of very different areas (df = 19, p = 0.001: 43.82)."""
    from ppsurf_amd import geometry
    rng = np.random.default_rng(5)
    scale = np.repeat(np.geomspace(0.05, 1.0, 20), 3)[:, None]
    verts = (rng.standard_normal((60, 3)) * scale).astype(np.float32)
    faces = np.arange(60, dtype=np.int32).reshape(20, 3)
    area, _, corners = geometry.face_stats(*_dev(verts, faces))
    n = 200000
    _, face = geometry.sample_surface(corners, geometry.area_prefix(area), n, seed=11)
    counts = np.bincount(face.cpu().numpy(), minlength=20)
    a = area.double().cpu().numpy()
    expected = n * a / a.sum()
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    assert chi2 < 43.82, chi2


def _winding_case(verts, faces, pts):
    from ppsurf_amd import geometry
    _, _, corners = geometry.face_stats(*_dev(verts, faces))
    w = geometry.winding_number(corners, torch.from_numpy(pts.astype(np.float32)).to(DEV)).cpu().numpy()
    w_np = E.winding_spec(verts.astype(np.float32), faces, pts.astype(np.float32))
    band = (np.abs(w_np) > 0.499) & (np.abs(w_np) < 0.501)
    assert np.array_equal((np.abs(w) > 0.5)[~band], (np.abs(w_np) > 0.5)[~band])
    assert np.median(np.abs(w - w_np)) < 1e-5
    # a small mesh is held to the derived bound on every query as well.  The 1280-face icosphere and the full fixture keep the assertions
    # above only: atan2_fast's own error is counted once per face, so there the bound exceeds E.WINDING_CAP and says nothing.
    # Measured max(err / bound) on an MI355X for the 320-face icosphere: 0.021.
    if faces.shape[0] <= 320:
        w_ref, bound = E.winding_spec_bounded(verts, faces, pts)
        case = dict(faces=faces, w=w_ref, bound=bound, planted=np.zeros(pts.shape[0], dtype=bool))
        print('{} faces: max err / bound {:.4f}'.format(faces.shape[0], E.check_winding(case, w)))
    return w, w_np


def _gpu_winding(verts, faces, pts):
    from ppsurf_amd import geometry
    _, _, corners = geometry.face_stats(*_dev(verts, faces))
    return geometry.winding_number(corners, torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(DEV)).cpu().numpy()


@pytest.mark.parametrize('name', E.WINDING_CASES)
def test_winding_within_the_derived_bound(name):
    """Every query of the case within winding_spec_bounded's bound of the fp64 winding number (E.check_winding: the reference first, then the
    kernel, then the inside mask), for the mesh and for its face-flipped copy; the planted degenerate queries finite, bounded by nf / 2 and
    the same bits in a second call.  Measured max(err / bound) on an MI355X: one_face 0.128, two_faces 0.082, corner3 0.080, ico63 0.052,
    ico64 0.049, ico65 0.040, ico320 0.014, ico313 0.015, abc500 0.036 (the numpy fp32 twin: 0.112 ... 0.036, test_eval_spec_cpu.py)."""
    case = E.winding_case(name)
    v, f, pts = case['verts'], case['faces'], case['pts']
    w = _gpu_winding(v, f, pts)
    ratio = E.check_winding(case, w)
    print('{}: {} faces, {} queries, max err / bound {:.4f}'.format(name, f.shape[0], pts.shape[0], ratio))
    assert np.array_equal(_gpu_winding(v, f, pts).view(np.uint64), w.view(np.uint64))
    held = case['bound'] < E.WINDING_CAP
    if name == 'ico320':                                      # closed: an integer
        assert (np.abs(w - np.round(w)) <= case['bound'])[held].all()
    w_flip = _gpu_winding(v, f[:, ::-1].copy(), pts)          # (the bound is symmetric in b <-> c)
    assert np.isfinite(w_flip).all()
    assert (np.abs(w + w_flip) <= 2 * case['bound'])[held].all()


def test_winding_tile_tails_against_the_prefix_of_a_longer_run():
    """m = 1, 255, 1023, 1024, 1025, 2049, 3000 queries (SWEEP_TILE = 1024, SWEEP_IPL = 4 rows of 256 lanes) on the open 313-face mesh: the
    first m queries alone give what they give inside the longer run, to the bound -- not bit for bit, the planner may cut elsewhere.
    Measured max(err / bound) on an MI355X: 0.015."""
    case = E.winding_case('ico313')
    v, f = case['verts'], case['faces']
    free = ~case['planted']
    pts, w_ref, bound = case['pts'][free], case['w'][free], case['bound'][free]
    assert (bound < E.WINDING_CAP).mean() >= 0.99
    w_long = _gpu_winding(v, f, pts)
    worst = 0.0
    for m in (1, 255, 1023, 1024, 1025, 2049, 3000):
        w = _gpu_winding(v, f, pts[:m])
        assert w.shape == (m,)
        held = bound[:m] < E.WINDING_CAP
        err = np.abs(w - w_ref[:m])
        assert (err <= bound[:m])[held].all(), m
        assert (np.abs(w - w_long[:m]) <= 2 * bound[:m])[held].all(), m
        worst = max(worst, float((err / bound[:m])[held].max())) if held.any() else worst
    print('max err / bound over the query counts {:.4f}'.format(worst))


def test_winding_number_against_numpy():
    rng = np.random.default_rng(2)
    v, f = E.icosphere(3, 0.3)
    pts = rng.random((5000, 3)) - 0.5
    pts[:1000] = pts[:1000] / np.linalg.norm(pts[:1000], axis=1, keepdims=True) * rng.uniform(0.28, 0.32, (1000, 1))   # near the surface
    w, w_np = _winding_case(v, f, pts)
    inside = np.linalg.norm(pts, axis=1) < 0.29
    assert (np.abs(w[inside] - 1.0) < 1e-4).all()
    _winding_case(*E.icosphere(2, 0.3), pts)                              # 320 faces: the derived bound too
    verts, faces = _fixture(1)
    w, w_np = _winding_case(verts, faces, rng.random((5000, 3)) - 0.5)
    assert 0.01 < (np.abs(w) > 0.5).mean() < 0.5                          # the part fills ~3 % of the query cube
    # a face-flipped mesh: w -> -w
    from ppsurf_amd import geometry
    q = torch.from_numpy((rng.random((5000, 3)) - 0.5).astype(np.float32)).to(DEV)
    _, _, c = geometry.face_stats(*_dev(verts, faces))
    _, _, c_flip = geometry.face_stats(*_dev(verts, faces[:, ::-1].copy()))
    w1, w2 = geometry.winding_number(c, q), geometry.winding_number(c_flip, q)
    w1, w2 = w1.cpu().numpy(), w2.cpu().numpy()
    # not bitwise: the rounding order of det and D changes with b <-> c, and a query next to a face plane sees that face's fp32 error
    assert np.median(np.abs(w2 + w1)) < 1e-6 and (np.abs(w2 + w1) < 1e-5).mean() > 0.99
    clear = np.abs(np.abs(w1) - 0.5) > 1e-3
    assert np.array_equal((np.abs(w1) > 0.5)[clear], (np.abs(w2) > 0.5)[clear])


def test_chamfer_nn_step_against_brute_force():
    from ppsurf_amd import evaluation, geometry
    verts, faces = _fixture(0)
    vg, fg = _fixture(2)
    a1, _, c1 = geometry.face_stats(*_dev(verts, faces))
    a2, _, c2 = geometry.face_stats(*_dev(vg, fg))
    s1, _ = geometry.sample_surface(c1, geometry.area_prefix(a1), 10000, seed=0, stream_id=0)
    s2, _ = geometry.sample_surface(c2, geometry.area_prefix(a2), 10000, seed=0, stream_id=1)
    idx, d2 = evaluation.nearest(s2, s1)
    p1, p2 = s1.cpu().numpy().astype(np.float64), s2.cpu().numpy().astype(np.float64)
    ref = np.empty(p1.shape[0])
    for s in range(0, p1.shape[0], 500):
        ref[s:s + 500] = ((p1[s:s + 500, None, :] - p2[None]) ** 2).sum(axis=2).min(axis=1)
    np.testing.assert_allclose(np.sqrt(d2.cpu().numpy().astype(np.float64)), np.sqrt(ref), rtol=0, atol=1e-6)
    got = ((p1 - p2[idx.cpu().numpy()]) ** 2).sum(axis=1)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)


def test_concentric_spheres_and_self_comparison():
    from ppsurf_amd import evaluation
    n = 100000
    vo, fo = E.icosphere(5, 0.30)
    vi, fi = E.icosphere(5, 0.25)
    m = evaluation.mesh_metrics(*_dev(vi, fi), *_dev(vo, fo), num_samples=n)
    ratio = E.mesh_volume(vi, fi) / E.mesh_volume(vo, fo)
    n_union = n * E.mesh_volume(vo, fo)                       # query points inside the outer sphere (unit cube of queries)
    sigma = (ratio * (1 - ratio) / n_union) ** 0.5
    assert abs(m['iou'] - ratio) < 4 * sigma, (m['iou'], ratio, sigma)
    assert abs(m['chamfer'] - 0.05) < 0.03 * 0.05, m['chamfer']
    assert m['normal_error'] < 0.05
    # a mesh against itself
    s = evaluation.mesh_metrics(*_dev(vo, fo), *_dev(vo, fo), num_samples=n)
    area = 4 * np.pi * 0.3 ** 2
    assert s['iou'] == 1.0 and s['f1'] == 1.0
    assert 0.0 < s['chamfer'] < 3 * (area / n) ** 0.5
    assert s['normal_error'] < 0.05
    flipped = evaluation.mesh_metrics(*_dev(vo, fo[:, ::-1].copy()), *_dev(vo, fo), num_samples=n)
    assert flipped['normal_error'] > 3.0 and flipped['iou'] == 1.0


def test_marching_cubes_sphere_against_an_icosphere():
    """The repo's Marching Cubes of an analytic sphere (inside > level) at R = 65 against an icosphere of the same radius: pins the MC
    orientation convention (normals towards lower values = outwards) against the evaluator's."""
    from ppsurf_amd import evaluation, ops
    R, r = 65, 0.35
    x = np.linspace(-0.5, 0.5, R)
    step = x[1] - x[0]
    g = np.stack(np.meshgrid(x, x, x, indexing='ij'), axis=-1)
    vol = torch.from_numpy(r - np.linalg.norm(g, axis=-1)).to(DEV).contiguous()
    verts, faces = ops.marching_cubes(vol, 0.0)
    verts = verts * step - 0.5
    vo, fo = E.icosphere(5, r)
    m = evaluation.mesh_metrics(verts.float(), faces, *_dev(vo, fo), num_samples=100000)
    assert m['iou'] > 0.97 and m['normal_error'] < 0.1 and 0 < m['chamfer'] < 2.0 / R, m


def test_mesh_metrics_is_deterministic():
    from ppsurf_amd import evaluation
    verts, faces = _fixture(0)
    vg, fg = _fixture(0)
    vg = vg * np.float32(0.97) + np.float32(0.01)
    a = evaluation.mesh_metrics(*_dev(verts, faces), *_dev(vg, fg), num_samples=30000)
    b = evaluation.mesh_metrics(*_dev(verts, faces), *_dev(vg, fg), num_samples=30000)
    assert a == b and all(np.isfinite(v) for v in a.values())
    assert 0.5 < a['iou'] < 1.0 and 0.0 < a['chamfer'] < 0.05


def _reduce_on_device(d):
    from ppsurf_amd import evaluation
    t = {k: (None if v is None else torch.as_tensor(v).to(DEV).contiguous()) for k, v in d.items()}
    return evaluation.reduce_sums(t['d2_rg'], t['d2_gr'], t['nn_rg'], t['face_rec'], t['face_gt'], t['normal_rec'], t['normal_gt'],
                                  t['w_rec'], t['w_gt']).cpu().numpy()


def _check_reduce(out, d):
    """The eight sums against reduce_spec: the counts equal as integers, the three fp64 sums within its bound.  Returns max(err / bound)."""
    ref, bound = E.reduce_spec(**d)
    assert np.array_equal(out[[2, 3, 4, 5, 7]], ref[[2, 3, 4, 5, 7]]), (out, ref)
    ratio = 0.0
    for k in (0, 1, 6):
        err = abs(out[k] - ref[k])
        assert err <= bound[k], (k, out[k], ref[k], bound[k])
        ratio = max(ratio, err / bound[k]) if bound[k] > 0 else ratio
    return ratio


@pytest.mark.parametrize('n_rec', [1, 511, 512, 513, 1537])
def test_reduce_against_plain_sums(n_rec):
    """reduce_kernel (one workgroup of 512, strided) against plain numpy sums on crafted inputs (E.reduce_inputs): n_rec around the
    workgroup size with another n_gt, mq = 0, 1, 777, zero / over-long / NaN normals, winding numbers at +-0.5 and on all four cells, and
    the None groups of a mesh without area.  Measured max(err / bound) on an MI355X: 0.22 (n_rec 512), 0.14, 0.13, 0.02, 0 (n_rec 1)."""
    worst = 0.0
    for mq in (0, 1, 777):
        d = E.reduce_inputs(n_rec, 700, mq, seed=n_rec + mq)
        out = _reduce_on_device(d)
        worst = max(worst, _check_reduce(out, d))
        assert np.array_equal(_reduce_on_device(d).view(np.uint64), out.view(np.uint64))
        bare = dict(d, d2_rg=None, d2_gr=None, nn_rg=None, face_rec=None, face_gt=None, normal_rec=None, normal_gt=None)
        out = _reduce_on_device(bare)
        assert out[[0, 1, 6, 7]].tolist() == [0.0] * 4
        _check_reduce(out, bare)
        # the two directions exchanged: the Chamfer sums and FP / FN change places bit for bit, nothing else moves
        plain = dict(d, nn_rg=None, face_rec=None, face_gt=None, normal_rec=None, normal_gt=None)
        a = _reduce_on_device(plain)
        b = _reduce_on_device(dict(plain, d2_rg=d['d2_gr'], d2_gr=d['d2_rg'], w_rec=d['w_gt'], w_gt=d['w_rec']))
        assert np.array_equal(b.view(np.uint64), a[[1, 0, 2, 4, 3, 5, 6, 7]].view(np.uint64))
    print('n_rec {}: max err / bound {:.4f}'.format(n_rec, worst))


def _metrics_from_stages(v_rec, f_rec, v_gt, f_gt, n):
    """mesh_metrics rebuilt in numpy fp64: Chamfer and the normal error from the outputs of the stages (each pinned on its own), IoU and
    F1 from the fp64 winding numbers -> (metrics, normal-error bound)."""
    from ppsurf_amd import evaluation, geometry
    ar, nr, cr = geometry.face_stats(*_dev(v_rec, f_rec))
    ag, ng, cg = geometry.face_stats(*_dev(v_gt, f_gt))
    s_rec, face_rec = geometry.sample_surface(cr, geometry.area_prefix(ar), n, 0, 0)
    s_gt, face_gt = geometry.sample_surface(cg, geometry.area_prefix(ag), n, 0, 1)
    nn_rg, d2_rg = evaluation.nearest(s_gt, s_rec)
    _, d2_gr = evaluation.nearest(s_rec, s_gt)
    query = evaluation.iou_query_points(n).astype(np.float32)
    w_rec, b_rec = E.winding_spec_bounded(v_rec, f_rec, query)
    w_gt, b_gt = E.winding_spec_bounded(v_gt, f_gt, query)
    # by the reference alone no query is near |w| = 0.5, so the kernel's inside masks must be the reference's: IoU and F1 exactly
    assert (np.abs(np.abs(w_rec) - 0.5) > 0.4999).all() and (np.abs(np.abs(w_gt) - 0.5) > 0.4999).all() and max(b_rec.max(), b_gt.max()) < E.WINDING_CAP
    host = lambda t: t.cpu().numpy()
    sums, bound = E.reduce_spec(host(d2_rg), host(d2_gr), host(nn_rg), host(face_rec), host(face_gt), host(nr), host(ng), w_rec, w_gt)
    tp, fp, fn = sums[2], sums[3], sums[4]
    precision, recall = tp / (tp + fp), tp / (tp + fn)
    ref = {'chamfer': (sums[0] + sums[1]) / (2 * n), 'f1': 2.0 * (precision * recall) / (precision + recall), 'iou': tp / (tp + fp + fn),
           'normal_error': sums[6] / sums[7]}
    assert sums[7] == n and tp > 0 and fp + fn > 0
    return ref, bound[6] / sums[7]


def test_mesh_metrics_against_the_stages():
    """mesh_metrics of two small spheres against a numpy fp64 rebuild: IoU and F1 equal, Chamfer to 1e-12 relative, the normal error to
    reduce_spec's bound over the count.  Exchanging reconstruction and ground truth keeps IoU and F1; its Chamfer is held to its own
    rebuild, not to the first call's: the surface samples are drawn per role (stream 0 the reconstruction, 1 the ground truth), so the
    two calls see other samples and agree to Monte-Carlo precision only (printed: 1.7e-3 relative).  What is symmetric bit for bit, the sums, is checked in
    test_reduce_against_plain_sums.  A reconstruction without area: Chamfer -1, normal error NaN, IoU 0."""
    from ppsurf_amd import evaluation
    n = 3000
    va, fa = E.icosphere(2, 0.30)
    vb, fb = E.icosphere(2, 0.25)
    vb = vb + np.array([0.03, -0.02, 0.01])
    got, ref = {}, {}
    for key, (v1, f1, v2, f2) in {'ab': (va, fa, vb, fb), 'ba': (vb, fb, va, fa)}.items():
        got[key] = evaluation.mesh_metrics(*_dev(v1, f1), *_dev(v2, f2), num_samples=n)
        ref[key], ne_bound = _metrics_from_stages(v1, f1, v2, f2, n)
        print(key, got[key], 'normal-error bound {:.2e}, err {:.2e}'.format(ne_bound, abs(got[key]['normal_error'] - ref[key]['normal_error'])))
        assert got[key]['iou'] == ref[key]['iou'] and got[key]['f1'] == ref[key]['f1']
        assert abs(got[key]['chamfer'] - ref[key]['chamfer']) <= 1e-12 * ref[key]['chamfer']
        assert abs(got[key]['normal_error'] - ref[key]['normal_error']) <= ne_bound
    assert 0.3 < got['ab']['iou'] < 0.7 and got['ab']['chamfer'] > 0.02
    assert got['ba']['iou'] == got['ab']['iou'] and got['ba']['f1'] == got['ab']['f1']
    print('Chamfer ab / ba - 1 = {:.2e}'.format(got['ab']['chamfer'] / got['ba']['chamfer'] - 1.0))
    flat = evaluation.mesh_metrics(*_dev(np.zeros((3, 3)), np.array([[0, 1, 2]])), *_dev(va, fa), num_samples=n)
    assert flat['chamfer'] == -1.0 and np.isnan(flat['normal_error']) and flat['iou'] == 0.0 and flat['f1'] == 0.0


def _read_tables(res_dir):
    out = {}
    for stem in ('chamfer_distance', 'f1', 'iou', 'normal_error'):
        out[stem] = [r.split(',') for r in open(os.path.join(res_dir, stem + '.csv')).read().strip().split('\n')]
    return out


def test_predict_evaluates_against_ground_truth(tmp_path, capsys):
    from test_gpu_cli import _configs
    from ppsurf_amd import evaluation, runner
    ds = tmp_path / 'ds'
    shutil.copytree(os.path.join(GOLDEN, 'abc_minimal_testset'), str(ds))
    shutil.copytree(GT_DIR, str(ds / '03_meshes'))
    in_file = str(ds / 'testset.txt')
    names = [s.strip() for s in open(in_file) if s.strip()]
    ckpt = str(tmp_path / 'last.ckpt')
    torch.save({'state_dict': {'network.' + k: v for k, v in filled_sd('', key='ppsurf').items()}}, ckpt)
    res = tmp_path / 'res'
    runner.main(['pps.py', 'predict'] + _configs(tmp_path, in_file) + ['--ckpt_path', ckpt, '--model.init_args.gen_resolution_global', '33',
                                                                       '--model.init_args.results_dir', str(res), '--trainer.devices', '1'])
    out = capsys.readouterr().out
    assert 'Evaluating ppsurf_mini' in out and 'Evaluating ppsurf_mini finished' in out
    res_dir = res / 'ppsurf_mini' / 'ds'
    tables = _read_tables(str(res_dir))
    missing = {n for n in names if not (res_dir / 'meshes' / (n + '.xyz.ply')).exists()}
    for stem, rows in tables.items():
        assert rows[0] == ['Shape', 'ppsurf_mini']
        assert [r[0] for r in rows[1:]] == names + ['AVERAGE', 'MEDIAN', 'STDEV']
        for r in rows[1:4]:
            assert (r[1] == 'nan') == (r[0] in missing), (stem, r)
    assert out.count('No reconstruction for') == len(missing)
    for r in tables['iou'][1:4]:
        assert r[0] in missing or 0.0 <= float(r[1]) <= 1.0
    # the ground truth as its own reconstruction
    gt = [os.path.join(str(ds / '03_meshes'), n + '.ply') for n in names]
    own = evaluation.make_quantitative_comparison(names, gt, ['gt'], [os.path.join(str(ds / '03_meshes'), '{}.ply')], str(tmp_path / 'own'),
                                                  num_samples=100000)
    assert own['iou'][0].tolist() == [1.0] * 3 and own['f1'][0].tolist() == [1.0] * 3
    assert (own['chamfer'][0] > 0).all() and (own['chamfer'][0] < 0.01).all() and (own['normals'][0] < 0.2).all()
    # the stand-alone command in a child process gives the same tables
    env = dict(os.environ)
    subprocess.check_call([sys.executable, '-m', 'ppsurf_amd.evaluation', '--name', 'ppsurf_mini', '--results_dir', str(res), '--data_dir', str(ds),
                           '--testset', 'testset.txt', '--num_samples', '100000', '--workers', '4'], cwd=REPO, env=env, timeout=300)
    assert _read_tables(str(res_dir)) == tables
