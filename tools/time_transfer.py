"""Rates of the colour transfer (ppsurf_amd/transfer.py, csrc/pps_transfer.hip).
    python tools/time_transfer.py [--res 257] [--points 250000] [--k 8] [--reps 10] [--spec_rows 2048] [--no_cpu]
-> median ms (after one warm-up round) for the vertices of the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` against a
coloured cloud of `--points` noisy points of that sphere: the block structure of the search (built once per cloud), the search alone, the blend
kernel alone and `transfer_colors` end to end.  Beside them the numpy specification tests/transfer_spec.py on this machine's CPU: its blend on
the whole input (checked against the kernel, bit for bit) and its brute-force search on the first `--spec_rows` vertices, scaled to all of them
(the whole search takes some ten minutes in numpy) -- the only baseline there is for a new capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import ops, transfer  # noqa: E402
import transfer_spec as T  # noqa: E402
from timing import wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--points', type=int, default=250000)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--spec_rows', type=int, default=2048)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    x = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(x, x, x, indexing='ij')
    verts, _ = ops.marching_cubes((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    rng = np.random.RandomState(41)
    d = rng.randn(args.points, 3)
    cloud_h = (0.35 * d / np.linalg.norm(d, axis=1, keepdims=True) + 0.001 * rng.randn(args.points, 3)).astype(np.float32)
    rgba_h = np.concatenate([rng.randint(0, 256, size=(args.points, 3)), np.full((args.points, 1), 255)], axis=1).astype(np.uint8)
    cloud, rgba = torch.from_numpy(cloud_h).to(dev), torch.from_numpy(rgba_h).to(dev)
    m, k = int(verts.shape[0]), args.k
    print('sphere R={}: {} vertices against {} coloured points, k = {}'.format(R, m, args.points, k))
    blocks = ops.KnnBlocks(cloud)
    idx, d2 = blocks.query(verts, k, return_d2=True)
    rows = [('block structure of the cloud (KnnBlocks, once per cloud)', wall_ms(lambda: ops.KnnBlocks(cloud), args.reps)),
            ('search: {} nearest of {} points for {} vertices'.format(k, args.points, m), wall_ms(lambda: blocks.query(verts, k, return_d2=True), args.reps)),
            ('blend kernel (ppsx_blend_rgba_u8)', wall_ms(lambda: transfer.blend_rgba(idx, d2, rgba), args.reps)),
            ('transfer_colors end to end (blocks + search + blend)', wall_ms(lambda: transfer.transfer_colors(cloud, rgba, verts, k=k), args.reps))]
    print('GPU ({} reps after warm-up):'.format(args.reps))
    for name, (med, lo_) in rows:
        print('  {:<72s} median {:10.3f} ms  min {:10.3f} ms'.format(name, med, lo_))
    moved = m * k * 12 + m * k * 4 + m * 4
    print('  blend: {:.1f} MB of indices, distances, gathered colours and results -> {:.0f} GB/s at the median'.format(moved / 1e6, moved / rows[2][1][0] / 1e6))
    if args.no_cpu:
        return
    print('CPU (numpy specification, one run each, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    hidx, hd2 = idx.cpu().numpy(), d2.cpu().numpy()
    t0 = time.perf_counter()
    want = T.blend(hidx, hd2, rgba_h)
    print('  {:<72s} {:10.1f} ms'.format('blend of all {} vertices'.format(m), (time.perf_counter() - t0) * 1e3))
    assert np.array_equal(transfer.blend_rgba(idx, d2, rgba).cpu().numpy(), want), 'the kernel differs from the specification'
    rows_ = min(args.spec_rows, m)
    hv = verts[:rows_].cpu().numpy()
    t0 = time.perf_counter()
    sidx, sd2 = T.knn(cloud_h, hv, k)
    dt = (time.perf_counter() - t0) * 1e3
    print('  {:<72s} {:10.1f} ms  (x {:.1f} = {:.0f} s for all vertices)'.format('brute-force search of the first {} vertices'.format(rows_), dt, m / rows_,
                                                                                 dt * m / rows_ / 1e3))
    assert np.array_equal(sidx, hidx[:rows_]) and np.array_equal(sd2.view(np.uint32), hd2[:rows_].view(np.uint32)), 'the search differs from the specification'


if __name__ == '__main__':
    main()
