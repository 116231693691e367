"""Rates of the Taubin smoothing (ppsurf_amd/smooth.py, csrc/pps_smooth.hip).
    python tools/time_smooth.py [--res 257] [--iters 10] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) for the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`: the adjacency build
(half-edge kernel, sort, distinct keys, row offsets), one pass (device events around 100 passes back to back) and `smooth_mesh(iters)` end to end.
Beside them the numpy specification tests/smooth_spec.py on this machine's CPU on the same mesh (checked against the device, bit for bit) --
the only baseline there is for a new capability."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, mcubes, smooth, topology  # noqa: E402
import smooth_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402


BATCH = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    faces = faces.contiguous()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    offsets, nbr, mult = topology.mesh_adjacency(faces, nv)
    ne = int(nbr.shape[0])
    deg = offsets[1:] - offsets[:-1]
    print('sphere R={}: {} faces, {} vertices, {} half-edges after merging, valence max {} mean {:.2f}'.format(
        R, nf, nv, ne, int(deg.max().item()), ne / nv))
    x, y = verts.double(), torch.empty(nv, 3, dtype=torch.float64, device=dev)

    def passes():                                     # BATCH passes between two events: one launch alone is too short to time
        for _ in range(BATCH // 2):
            _lib.call('ppsx_smooth_pass', x, nv, offsets, nbr, mult, ne, 0.5, y)
            _lib.call('ppsx_smooth_pass', y, nv, offsets, nbr, mult, ne, -0.53, x)

    rows = [('adjacency (ppsx_smooth_half_edges + sort + unique_consecutive + bincount + cumsum), wall', wall_ms(lambda: topology.mesh_adjacency(faces, nv), args.reps)),
            ('{} passes back to back (ppsx_smooth_pass), device events'.format(BATCH), device_ms(passes, args.reps)),
            ('smooth_mesh(iters={}) end to end, wall'.format(args.iters), wall_ms(lambda: smooth.smooth_mesh(verts, faces, args.iters), args.reps))]
    print('GPU ({} reps after warm-up):'.format(args.reps))
    for name, (med, lo_) in rows:
        print('  {:<92s} median {:10.3f} ms  min {:10.3f} ms'.format(name, med, lo_))
    # bytes one pass asks for: x and out (24 B each) and an offset (8 B) per vertex; mult (4 B), then nbr + mult (8 B) and 24 B of x per entry
    moved = nv * (24 + 24 + 8) + ne * (4 + 8 + 24)
    per_pass = rows[1][1][0] / BATCH
    print('  one pass: {:.4f} ms; it asks for {:.1f} MB -> {:.0f} GB/s (the adjacency and both states stay in the caches between passes)'.format(
        per_pass, moved / 1e6, moved / per_pass / 1e6))
    out_v, _, info = smooth.smooth_mesh(verts, faces, args.iters)
    print('  smooth_mesh: {}'.format(info))
    if args.no_cpu:
        return
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    t0 = time.perf_counter()
    want = S.smooth_spec(hv, hf, args.iters)
    dt = (time.perf_counter() - t0) * 1e3
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    print('  {:<92s} {:10.1f} ms'.format('smooth_spec(iters={}) on the same mesh'.format(args.iters), dt))
    assert out_v.cpu().numpy().tobytes() == want.tobytes(), 'the device differs from the specification'
    print('  the device equals the specification on all {} vertices'.format(nv))


if __name__ == '__main__':
    main()
