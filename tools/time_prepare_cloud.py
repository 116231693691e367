"""Rates of the cloud preparation (ppsurf_amd/cloud.py, csrc/pps_cloud.hip).
    python tools/time_prepare_cloud.py [--points 5000000] [--budget 250000] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) on a synthetic noisy-torus scan of `--points` points: one counting pass at the chosen grid, the whole
20-pass budget search, the selection pass, 17-NN search + outlier kernels on the kept cloud, and `prepare_cloud` end to end from the host
array (upload included).  Kernel stages are timed with device events, stages with a host loop by wall clock around a synchronise.  Beside
them the same stages of the numpy specification tests/cloud_spec.py and of scipy's kd-tree on this machine's CPU (one run each), the only
baseline there is for a new capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import cloud, ops  # noqa: E402
import cloud_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402


def torus_scan(n, seed=1):
    rng = np.random.RandomState(seed)
    u, v = rng.rand(n) * 2 * np.pi, rng.rand(n) * 2 * np.pi
    p = np.stack([(1.0 + 0.3 * np.cos(v)) * np.cos(u), (1.0 + 0.3 * np.cos(v)) * np.sin(u), 0.3 * np.sin(v)], axis=1)
    return (p + 0.002 * rng.randn(n, 3)) * 20.0 + np.array([512345.0, 5403210.0, 310.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=5000000)
    ap.add_argument('--budget', type=int, default=250000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    host = torus_scan(args.points)
    centred = (host - (host.min(axis=0) + host.max(axis=0)) * 0.5).astype(np.float32)
    pts = torch.from_numpy(centred).to(dev)
    grid = cloud.VoxelGrid(pts)
    G = grid.search(args.budget)
    h, inv_h = grid.step(G)
    sel = grid.select(h, inv_h)
    kept = pts[sel].contiguous()
    print('{} points, budget {}: G {} h {:.6g} kept {}; table of {} slots'.format(args.points, args.budget, G, float(h), sel.shape[0], grid.capacity))
    lib, st = cloud._lib.lib(), torch.cuda.current_stream().cuda_stream
    lo, hi = grid._vec3(grid.lo), grid._vec3(grid.hi)
    grid._scratch(best=True)
    keep = torch.empty(grid.n, dtype=torch.uint8, device=dev)

    def count_pass():
        lib.pps_cloud_voxel_count(pts.data_ptr(), grid.n, lo, hi, float(h), float(inv_h), grid._table.data_ptr(), grid.capacity, grid._count.data_ptr(), st)

    def select_pass():
        lib.pps_cloud_voxel_select(pts.data_ptr(), grid.n, lo, hi, float(h), float(inv_h), grid._table.data_ptr(), grid._best.data_ptr(), grid.capacity,
                                   grid._count.data_ptr(), keep.data_ptr(), st)

    def knn_outliers():
        cloud.remove_outliers(kept, 16, 2.0)

    rows = [('one counting pass (kernel + table reset)', device_ms(count_pass, args.reps)),
            ('selection pass (kernels + resets, without the compaction)', device_ms(select_pass, args.reps)),
            ('selection pass with torch.nonzero', wall_ms(lambda: grid.select(h, inv_h), args.reps)),
            ('budget search, 20 counting passes (host loop)', wall_ms(lambda: grid.search(args.budget), args.reps)),
            ('17-NN search + outlier kernels on the kept cloud', wall_ms(knn_outliers, args.reps)),
            ('prepare_cloud end to end from the host array', wall_ms(lambda: cloud.prepare_cloud(host, max_points=args.budget, outlier_k=16, device=dev),
                                                                     args.reps))]
    print('GPU ({} reps after warm-up):'.format(args.reps))
    for name, (med, lo_) in rows:
        print('  {:<60s} median {:10.3f} ms  min {:10.3f} ms'.format(name, med, lo_))
    if args.no_cpu:
        return
    print('CPU (numpy specification / scipy kd-tree, one run each, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    blo, bhi, ext = S.box(centred)

    def cpu(name, fn):
        t0 = time.perf_counter()
        out = fn()
        print('  {:<60s} {:10.1f} ms'.format(name, (time.perf_counter() - t0) * 1e3))
        return out
    cpu('one counting pass (np.unique of the keys)', lambda: S.voxel_count(centred, blo, bhi, h, inv_h))
    g_cpu = cpu('budget search, 20 counting passes', lambda: S.budget_search(centred, args.budget))
    s_cpu = cpu('selection pass (lexsort)', lambda: S.voxel_select(centred, blo, bhi, h, inv_h))
    assert g_cpu == G and np.array_equal(s_cpu, sel.cpu().numpy())
    from scipy.spatial import cKDTree
    kc = centred[s_cpu].astype(np.float64)

    def tree():
        dist, _ = cKDTree(kc).query(kc, k=17, workers=-1)
        m = dist[:, 1:].mean(axis=1)
        return np.nonzero(m <= m.mean() + 2.0 * m.std())[0]
    cpu('kd-tree 17-NN (all cores) + statistics on the kept cloud', tree)


if __name__ == '__main__':
    main()
