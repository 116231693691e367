"""Stages of the qualitative comparison (ppsurf_amd/visualization.py, csrc/pps_vis.hip) on one R = 257 case: the repo's Marching Cubes of an
analytic sphere (radius 0.35) as the reconstruction against a 20480-face icosphere of the same radius as the ground truth.
    python tools/time_comparison.py [--reps 10]
-> device-event ms of the closest point of every reconstruction vertex on the ground truth (and its rate in point x triangle pairs per
second), of one midpoint subdivision of the reconstruction, of rasterisation and shading of the reconstruction at 1024^2, and the wall
time of one shape of the comparison: visualize_chamfer_distance plus the four renders (reconstruction, ground truth, distance mesh,
point cloud), files included."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import geometry as geo, meshio, ops, visualization as vis  # noqa: E402
from eval_spec import icosphere  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--size', type=int, default=1024)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R, r, size = args.res, 0.35, args.size
    x = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(x, x, x, indexing='ij')
    vol = (r - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous()
    v_rec, f_rec = ops.marching_cubes(vol, 0.0)
    v_rec = (v_rec * (1.0 / (R - 1)) - 0.5).float().contiguous()
    f_rec = f_rec.to(torch.int32).contiguous()
    vg, fg = icosphere(5, r)
    v_gt = torch.from_numpy(vg.astype(np.float32)).to(dev)
    f_gt = torch.from_numpy(fg.astype(np.int32)).to(dev)
    _, _, c_gt = geo.face_stats(v_gt, f_gt)
    cam = vis.camera_array(*vis.camera(v_rec.cpu().numpy(), size))

    stages = ['closest point', 'subdivide', 'raster', 'shade']
    times = {s: [] for s in stages}
    for rep in range(args.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        _, d, _ = geo.closest_point_on_corners(c_gt, v_rec)
        e[1].record()
        vis.subdivide(v_rec, f_rec)
        e[2].record()
        keys = vis.raster_faces(v_rec, f_rec, cam, size, size)
        e[3].record()
        vis.shade(keys, v_rec, f_rec, cam)
        e[4].record()
        torch.cuda.synchronize()
        if rep > 0:                                   # the first round warms up (code objects, allocator)
            for i, s in enumerate(stages):
                times[s].append(e[i].elapsed_time(e[i + 1]))
    pairs = v_rec.shape[0] * f_gt.shape[0]
    print('R = {}: reconstruction {} vertices / {} faces, ground truth {} faces, {}^2 pixels, {} reps'.format(
        R, v_rec.shape[0], f_rec.shape[0], f_gt.shape[0], size, args.reps))
    for s in stages:
        t = np.array(times[s])
        print('  {:<14s} median {:8.3f} ms   min {:8.3f} ms'.format(s, float(np.median(t)), float(t.min())))
    t_c = float(np.median(times['closest point'])) * 1e-3
    print('  closest point: {:.3e} point x triangle pairs in {:.3f} ms = {:.3e} pairs/s; max |d| = {:.3e}'.format(
        pairs, t_c * 1e3, pairs / t_c, float(d.abs().max())))
    print('  raster + shade: {:.3f} ms'.format(float(np.median(np.array(times['raster']) + np.array(times['shade'])))))

    with tempfile.TemporaryDirectory() as tmp:
        rec, gt, pc = os.path.join(tmp, 'rec.ply'), os.path.join(tmp, 'gt.ply'), os.path.join(tmp, 'pc.ply')
        meshio.write_ply_mesh(rec, v_rec.cpu().numpy(), f_rec.cpu().numpy())
        meshio.write_ply_mesh(gt, vg, fg)
        pts, _ = geo.sample_surface(c_gt, geo.area_prefix(geo.face_stats(v_gt, f_gt)[0]), 50000)
        meshio.write_ply_points(pc, pts.cpu().numpy())
        walls = []
        for rep in range(3):
            out = os.path.join(tmp, 'out{}'.format(rep))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cd = os.path.join(out, 'cd.ply')
            vis.visualize_chamfer_distance(rec, gt, cd, 10000, 0.05)
            vis.render_meshes([rec, gt, cd, pc], [os.path.join(out, n + '.png') for n in ('rec', 'gt', 'cd', 'pc')])
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        print('  one shape (distance mesh + 4 renders, files included): {:.3f} s (runs: {})'.format(
            float(np.median(walls[1:])), ', '.join('{:.3f}'.format(w) for w in walls)))


if __name__ == '__main__':
    main()
