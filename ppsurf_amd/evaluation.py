"""Evaluation of reconstructions against ground-truth meshes on the GPU: Chamfer distance, F1, IoU and normal error.

    python -m ppsurf_amd.evaluation --name ppsurf --results_dir results --data_dir datasets/abc_minimal --testset testset.txt \\
        --num_samples 100000

Replaces source/base/evaluation.py:32-59 (`make_quantitative_comparison`) and source/base/metrics.py:120-323, which need trimesh,
pysdf, pykdtree and openpyxl.  Per mesh pair, one upload and one set of samples serve all four metrics (the mesh queries are
geometry.py's, the reduction is csrc/pps_eval.hip):
  * face statistics (areas, unit normals, face-major corners) of both meshes;
  * `num_samples` area-weighted surface samples of each mesh (counter-based generator, stream 0 = reconstruction, 1 = ground truth);
  * the two 1-NN searches between the sample sets (ops.KnnBlocks, k = 1): Chamfer = (sum d(gt->rec) + sum d(rec->gt)) / (N_rec + N_gt)
    with Euclidean distances (metrics.py:120-139); normal error = mean arccos(clip(n_rec . n_gt[nn], -1, 1)) over the rec->gt neighbours
    (`normal_error_approx`, metrics.py:246-269);
  * inside masks of both meshes over the reference's query points `default_rng(42).random((num_samples, 3)) - 0.5` by the generalised
    winding number (|w| > 0.5), which give IoU and F1 (metrics.py:157-219);
  * the fp64 sums of all of it in one deterministic reduction.
The estimators and the IoU/F1 query points are the reference's; the surface samples come from this generator, not trimesh's, so
Chamfer and normal error agree with the reference to Monte-Carlo precision.  The tables are CSV (openpyxl is not available).

`--data_dir` is the dataset root here (the ground truth is `<data_dir>/03_meshes`, the shape list `<data_dir>/<testset>`).  The
reference's defaults (`--data_dir datasets/abc_minimal/03_meshes`, `--testset datasets/abc_minimal/testset.txt`) do not resolve
together, since it joins the two; its own driver passes `--data_dir datasets/<name> --testset testset.txt`.
"""
import argparse
import math
import os
import typing
import warnings

import numpy as np
import torch

from . import _lib, meshio, ops
from .geometry import _device, area_prefix, face_stats, sample_surface, winding_number
from .lightning_api import calc_f1, calc_precision, calc_recall

METRIC_FILES = {'chamfer': 'chamfer_distance', 'f1': 'f1', 'iou': 'iou', 'normals': 'normal_error'}
_KEYS = {'chamfer': 'chamfer', 'f1': 'f1', 'iou': 'iou', 'normals': 'normal_error'}


def iou_query_points(num_samples: int, num_dims: int = 3) -> np.ndarray:
    """The reference's IoU / F1 query points, bit for bit (metrics.py:162-163, 187-188)."""
    rng = np.random.default_rng(seed=42)
    return rng.random(size=(num_samples, num_dims)) - 0.5


def reduce_sums(d2_rg, d2_gr, nn_rg, face_rec, face_gt, normal_rec, normal_gt, w_rec, w_gt) -> torch.Tensor:
    """f64 [8] on the device: sum sqrt(d2_rg), sum sqrt(d2_gr), TP, FP, FN, TN, sum arccos(...), number of non-NaN cosines.
    d2_rg / d2_gr (and the normal group) may be None."""
    dev = w_rec.device
    out = torch.empty(8, dtype=torch.float64, device=dev)
    n_rec = d2_rg.shape[0] if d2_rg is not None else 0
    n_gt = d2_gr.shape[0] if d2_gr is not None else 0
    _lib.call('pps_eval_reduce', d2_rg, n_rec, d2_gr, n_gt, nn_rg, face_rec, face_gt, normal_rec, normal_gt, w_rec, w_gt, w_rec.shape[0], out)
    return out


def nearest(pts: torch.Tensor, query: torch.Tensor):
    """1-NN of every query among pts -> (index int64 [m], squared distance f32 [m]) through the block-culling kNN search."""
    idx, d2 = ops.KnnBlocks(pts).query(query, 1, return_d2=True)
    return idx[:, 0].contiguous(), d2[:, 0].contiguous()


def _upload(verts, faces, device):
    v = torch.as_tensor(verts).to(device=device, dtype=torch.float32).contiguous()
    f = torch.as_tensor(faces).to(device=device, dtype=torch.int32).contiguous()
    return v, f


def mesh_metrics(verts_rec: torch.Tensor, faces_rec: torch.Tensor, verts_gt: torch.Tensor, faces_gt: torch.Tensor, num_samples: int,
                 seed: int = 0) -> dict:
    """{'chamfer', 'f1', 'iou', 'normal_error'} of a reconstruction against its ground truth, all device tensors (verts [nv,3],
    faces [nf,3] integer).  Chamfer is -1.0 and the normal error NaN when either mesh has no samplable area (metrics.py:127-128)."""
    _lib.need_device('evaluation', verts_rec, faces_rec, verts_gt, faces_gt)
    dev = verts_rec.device
    vr, fr = _upload(verts_rec, faces_rec, dev)
    vg, fg = _upload(verts_gt, faces_gt, dev)
    ar, nr, cr = face_stats(vr, fr)
    ag, ng, cg = face_stats(vg, fg)
    pr, pg = area_prefix(ar), area_prefix(ag)
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    tot_r, tot_g = torch.cat([zero, pr[-1:]]).max(), torch.cat([zero, pg[-1:]]).max()
    query = torch.from_numpy(iou_query_points(num_samples)).to(device=dev, dtype=torch.float32)
    w_rec, w_gt = winding_number(cr, query), winding_number(cg, query)
    tot_r, tot_g = [float(x) for x in torch.stack([tot_r, tot_g]).tolist()]
    n = int(num_samples)
    if tot_r > 0.0 and tot_g > 0.0 and n > 0:
        s_rec, f_rec = sample_surface(cr, pr, n, seed, 0)
        s_gt, f_gt = sample_surface(cg, pg, n, seed, 1)
        nn_rg, d2_rg = nearest(s_gt, s_rec)
        _, d2_gr = nearest(s_rec, s_gt)
        sums = reduce_sums(d2_rg, d2_gr, nn_rg, f_rec, f_gt, nr, ng, w_rec, w_gt).tolist()
        chamfer = (sums[0] + sums[1]) / (2 * n)
        normal_error = sums[6] / sums[7] if sums[7] > 0 else float('nan')
    else:
        sums = reduce_sums(None, None, None, None, None, None, None, w_rec, w_gt).tolist()
        chamfer, normal_error = -1.0, float('nan')
    tp, fp, fn = sums[2], sums[3], sums[4]
    union = tp + fp + fn
    iou = 0.0 if union == 0.0 else tp / union
    f1 = calc_f1(calc_precision(tp, fp), calc_recall(tp, fn))
    if math.isnan(f1):
        f1 = 0.0
    return {'chamfer': chamfer, 'f1': f1, 'iou': iou, 'normal_error': normal_error}


# ---- the reference's file-level API (metrics.py:120-323) ---------------------------------------------------------------------------------------
def load_mesh(path: str):
    """(verts f32 [nv,3], faces int32 [nf,3]) of a mesh file (PLY; the reference loads through trimesh)."""
    if os.path.splitext(path)[1].lower() != '.ply':
        raise ValueError('only PLY meshes are supported: {}'.format(path))
    return meshio.read_ply_mesh(path)


def file_metrics(file_in: str, file_ref: str, num_samples: int) -> dict:
    """mesh_metrics of two mesh files; every metric NaN when either file cannot be read."""
    try:
        v_in, f_in = load_mesh(file_in)
        v_ref, f_ref = load_mesh(file_ref)
    except (OSError, ValueError, KeyError, IndexError):
        return {k: float('nan') for k in ('chamfer', 'f1', 'iou', 'normal_error')}
    dev = _device()
    vi, fi = _upload(v_in, f_in, dev)
    vr, fr = _upload(v_ref, f_ref, dev)
    return mesh_metrics(vi, fi, vr, fr, num_samples)


def chamfer_distance(file_in, file_ref, samples_per_model, num_processes=1):
    return file_in, file_ref, file_metrics(file_in, file_ref, samples_per_model)['chamfer']


def intersection_over_union(file_in, file_ref, num_samples, num_dims=3):
    assert num_dims == 3
    return file_in, file_ref, file_metrics(file_in, file_ref, num_samples)['iou']


def f1_approx(file_in, file_ref, num_samples, num_dims=3):
    assert num_dims == 3
    return file_in, file_ref, file_metrics(file_in, file_ref, num_samples)['f1']


def normal_error_approx(file_in, file_ref, num_samples=100000, num_processes=1):
    return file_in, file_ref, file_metrics(file_in, file_ref, num_samples)['normal_error']


def get_metrics_mesh_single_file(gt_mesh_file: str, mesh_file: str, num_samples: int) -> dict:
    """All four metrics of one pair with the guards of get_metric_mesh_single_file (metrics.py:289-303)."""
    if os.path.isfile(mesh_file) and os.path.isfile(gt_mesh_file):
        return file_metrics(mesh_file, gt_mesh_file, num_samples)
    if not os.path.isfile(mesh_file):
        print('WARNING: mesh missing: {}'.format(mesh_file))
        return {k: float('nan') for k in ('chamfer', 'f1', 'iou', 'normal_error')}
    raise FileExistsError()


def get_metric_mesh_single_file(gt_mesh_file: str, mesh_file: str, num_samples: int,
                                metric: typing.Literal['chamfer', 'iou', 'normals', 'f1'] = 'chamfer') -> float:
    if metric not in _KEYS:
        raise ValueError()
    return get_metrics_mesh_single_file(gt_mesh_file, mesh_file, num_samples)[_KEYS[metric]]


def _all_metrics(result_file_template, shape_list, gt_mesh_files, num_samples):
    """{metric: [np.ndarray over shapes, one per template]}, every mesh pair loaded and evaluated once."""
    out = {m: [] for m in _KEYS}
    for template in result_file_template:
        rows = [get_metrics_mesh_single_file(gt_mesh_files[i], template.format(s), num_samples) for i, s in enumerate(shape_list)]
        for m, key in _KEYS.items():
            out[m].append(np.array([r[key] for r in rows], dtype=np.float64))
    return out


def get_metric_meshes(result_file_template: typing.Sequence[str], shape_list: typing.Sequence[str], gt_mesh_files: typing.Sequence[str],
                      num_samples=10000, metric: typing.Literal['chamfer', 'iou', 'normals', 'f1'] = 'chamfer', num_processes=1):
    """metrics.py:306-323 (one process: the work is on the GPU)."""
    if metric not in _KEYS:
        raise ValueError()
    return _all_metrics(result_file_template, shape_list, gt_mesh_files, num_samples)[metric]


def write_metric_table(path: str, shape_names, headers, columns):
    """CSV of one metric: `Shape,<header>...`, one row per shape, then the AVERAGE / MEDIAN / STDEV rows of evaluation.py:286-297
    (NaN ignored, STDEV = sample standard deviation)."""
    data = np.array(columns, dtype=np.float64).reshape(len(headers), len(shape_names)).T
    fmt = lambda v: repr(float(v))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=RuntimeWarning)      # all-NaN columns, fewer than two values for STDEV
        stats = [('AVERAGE', np.nanmean(data, axis=0)), ('MEDIAN', np.nanmedian(data, axis=0)), ('STDEV', np.nanstd(data, axis=0, ddof=1))]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(','.join(['Shape'] + list(headers)) + '\n')
        for name, row in zip(shape_names, data):
            f.write(','.join([name] + [fmt(v) for v in row]) + '\n')
        for name, row in stats:
            f.write(','.join([name] + [fmt(v) for v in row]) + '\n')


def make_quantitative_comparison(shape_names: typing.Sequence[str], gt_mesh_files: typing.Sequence[str], result_headers: typing.Sequence[str],
                                 result_file_templates: typing.Sequence[str], comp_output_dir: str, num_samples=10000, num_processes=0):
    """evaluation.py:32-59: chamfer_distance.csv, f1.csv, iou.csv and normal_error.csv in comp_output_dir.  Returns
    {metric: [np.ndarray over shapes, one per template]}."""
    results = _all_metrics(result_file_templates, shape_names, gt_mesh_files, num_samples)
    for metric, stem in METRIC_FILES.items():
        write_metric_table(os.path.join(comp_output_dir, stem + '.csv'), shape_names, result_headers, results[metric])
    return results


# ---- stand-alone command (source/make_evaluation.py) ---------------------------------------------------------------------------------------------
def parse_arguments(args=None):
    parser = argparse.ArgumentParser(description='Evaluate reconstructions against the ground-truth meshes of a dataset (on the GPU).')
    parser.add_argument('--name', type=str, default='ppsurf', help='name')
    parser.add_argument('--workers', type=int, default=8, help='accepted for compatibility and ignored (the work runs on the GPU)')
    parser.add_argument('--results_dir', type=str, default='results', help='output folder (reconstructions)')
    parser.add_argument('--data_dir', type=str, default='datasets/abc_minimal', help='dataset root (holds 03_meshes and the test set file)')
    parser.add_argument('--testset', type=str, default='testset.txt', help='test set file name, relative to --data_dir')
    parser.add_argument('--num_samples', type=int, default=10000, help='number of samples for metrics')
    return parser.parse_args(args=args)


def make_evaluation(args):
    from .data import read_shape_list
    data_dir = os.path.normpath(args.data_dir)
    model_results_rec_dir = os.path.join(args.results_dir, args.name, os.path.basename(data_dir))
    shape_names = read_shape_list(os.path.join(data_dir, args.testset))
    gt_meshes_dir = os.path.join(data_dir, '03_meshes')
    if not os.path.exists(gt_meshes_dir):
        print('Warning: {} not found. Skipping evaluation.'.format(gt_meshes_dir))
        return None
    gt_meshes = [os.path.join(gt_meshes_dir, '{}.ply'.format(vs)) for vs in shape_names]
    os.makedirs(model_results_rec_dir, exist_ok=True)
    return make_quantitative_comparison(shape_names=shape_names, gt_mesh_files=gt_meshes, result_headers=[args.name],
                                        result_file_templates=[os.path.join(model_results_rec_dir, 'meshes/{}.xyz.ply')],
                                        comp_output_dir=model_results_rec_dir, num_processes=args.workers, num_samples=args.num_samples)


def main(argv=None):
    make_evaluation(parse_arguments(argv))


if __name__ == '__main__':
    main()
