"""Rates of the dataset generator (ppsurf_amd/make_dataset.py, csrc/pps_scan.hip).
    python tools/time_make_dataset.py [--reps 10]
-> device-event ms and ray x triangle pairs per second of the first-hit kernel for the rays of 30 scans at 64^2 (122880 rays) against
the repo's Marching Cubes of an analytic sphere at R = 257 (radius 0.35, ~3 x 10^5 faces) and against a 20480-face icosphere; then the wall
time and point count per shape of a whole default build (`make_dataset`, files included) of tests/golden/abc_minimal_gt/03_meshes."""
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
from ppsurf_amd import geometry as geo, make_dataset as md, meshio, ops  # noqa: E402
from eval_spec import icosphere  # noqa: E402


def time_first_hit(name, verts, faces, reps):
    _, _, corners = geo.face_stats(verts, faces)
    s = md.resolve_settings(None, num_scans_per_mesh_min=30, num_scans_per_mesh_max=30)
    v = verts.cpu().numpy()
    cams = md.scan_cameras(v.min(0), v.max(0), s, md.shape_rng(0, name))
    orig, dirs = md.scan_rays(torch.from_numpy(cams).to(verts.device), s['scan_resolution'])
    times = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t, face = geo.first_hit(corners, orig, dirs)
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:                                   # the first round warms up (code objects, allocator)
            times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    pairs = orig.shape[0] * faces.shape[0]
    print('  {:<10s} {:>7d} faces x {} rays: median {:8.3f} ms  min {:8.3f} ms = {:.3e} pairs/s; {:.1f} % of rays hit'.format(
        name, faces.shape[0], orig.shape[0], ms, float(np.min(times)), pairs / (ms * 1e-3), 100.0 * float((face >= 0).float().mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--res', type=int, default=257)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R, r = args.res, 0.35
    x = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(x, x, x, indexing='ij')
    vol = (r - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous()
    v_mc, f_mc = ops.marching_cubes(vol, 0.0)
    v_mc = (v_mc * (1.0 / (R - 1)) - 0.5).float().contiguous()
    f_mc = f_mc.to(torch.int32).contiguous()
    vi, fi = icosphere(5, r)
    print('first hit (30 scans x 64^2 rays, {} reps):'.format(args.reps))
    time_first_hit('sphere R={}'.format(R), v_mc, f_mc, args.reps)
    time_first_hit('icosphere', torch.from_numpy(vi.astype(np.float32)).to(dev), torch.from_numpy(fi.astype(np.int32)).to(dev), args.reps)

    gt = os.path.join(REPO, 'tests', 'golden', 'abc_minimal_gt', '03_meshes')
    names = sorted(md.mesh_files(gt))
    print('whole default build of {} ({} shapes):'.format(os.path.relpath(gt, REPO), len(names)))
    with tempfile.TemporaryDirectory() as tmp:
        md.make_dataset(gt, os.path.join(tmp, 'warm'), verbose=False)
        for name in names:
            one = os.path.join(tmp, 'in_' + name)
            os.makedirs(one)
            os.symlink(os.path.join(gt, name + '.ply'), os.path.join(one, name + '.ply'))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            md.make_dataset(one, os.path.join(tmp, 'out_' + name), verbose=False)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            n = meshio.read_ply_vertices(os.path.join(tmp, 'out_' + name, '04_pts_vis', name + '.xyz.ply')).shape[0]
            nf = meshio.read_ply_mesh(os.path.join(gt, name + '.ply'))[1].shape[0]
            print('  {}: {} faces, {} points, {:.3f} s'.format(name, nf, n, wall))


if __name__ == '__main__':
    main()
