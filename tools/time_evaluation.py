"""Stages of the mesh evaluation (ppsurf_amd/evaluation.py, csrc/pps_eval.hip) at the reference's setting (100k samples) on one R = 257 case:
the repo's Marching Cubes of an analytic sphere (radius 0.35, inside > 0) against a 20480-face icosphere of the same radius.
    python tools/time_evaluation.py [--reps 10]
-> device-event ms per stage (face stats, sampling, 1-NN, winding, reduce) and of the whole mesh_metrics, and the winding kernel's rate in
point x triangle pairs per second (both meshes' winding passes over the 100k IoU query points)."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import evaluation as ev, geometry as geo, ops  # noqa: E402
from eval_spec import icosphere  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--num_samples', type=int, default=100000)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R, r, n = args.res, 0.35, args.num_samples
    x = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(x, x, x, indexing='ij')
    vol = (r - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous()
    v_rec, f_rec = ops.marching_cubes(vol, 0.0)
    v_rec = (v_rec * (1.0 / (R - 1)) - 0.5).float().contiguous()
    f_rec = f_rec.to(torch.int32).contiguous()
    vg, fg = icosphere(5, r)
    v_gt = torch.from_numpy(vg.astype(np.float32)).to(dev)
    f_gt = torch.from_numpy(fg.astype(np.int32)).to(dev)
    query = torch.from_numpy(ev.iou_query_points(n)).to(device=dev, dtype=torch.float32)

    stages = ['face stats', 'sampling', '1-NN', 'winding', 'reduce', 'mesh_metrics']
    times = {s: [] for s in stages}
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        e[0].record()
        ar, nr, cr = geo.face_stats(v_rec, f_rec)
        ag, ng, cg = geo.face_stats(v_gt, f_gt)
        e[1].record()
        pr, pg = geo.area_prefix(ar), geo.area_prefix(ag)
        s_rec, fi_rec = geo.sample_surface(cr, pr, n, 0, 0)
        s_gt, fi_gt = geo.sample_surface(cg, pg, n, 0, 1)
        e[2].record()
        nn_rg, d2_rg = ev.nearest(s_gt, s_rec)
        _, d2_gr = ev.nearest(s_rec, s_gt)
        e[3].record()
        w_rec, w_gt = geo.winding_number(cr, query), geo.winding_number(cg, query)
        e[4].record()
        ev.reduce_sums(d2_rg, d2_gr, nn_rg, fi_rec, fi_gt, nr, ng, w_rec, w_gt)
        e[5].record()
        m = ev.mesh_metrics(v_rec, f_rec, v_gt, f_gt, n)
        e[6].record()
        torch.cuda.synchronize()
        if rep > 0:                                   # the first round warms up (code objects, allocator)
            for i, s in enumerate(stages):
                times[s].append(e[i].elapsed_time(e[i + 1]))
    pairs = n * (f_rec.shape[0] + f_gt.shape[0])
    print('R = {}: reconstruction {} faces, ground truth {} faces, {} samples / query points, {} reps'.format(
        R, f_rec.shape[0], f_gt.shape[0], n, args.reps))
    for s in stages:
        t = np.array(times[s])
        print('  {:<13s} median {:8.3f} ms   min {:8.3f} ms'.format(s, float(np.median(t)), float(t.min())))
    t_w = float(np.median(times['winding'])) * 1e-3
    print('  winding: {:.3e} point x triangle pairs in {:.3f} ms = {:.3e} pairs/s'.format(pairs, t_w * 1e3, pairs / t_w))
    print('  metrics: ' + ', '.join('{} {:.6g}'.format(k, v) for k, v in m.items()))


if __name__ == '__main__':
    main()
