"""Rates of the hole filling (ppsurf_amd/fill.py, csrc/pps_fill.hip).
    python tools/time_fill.py [--res 257] [--max_edges 16] [--fans 2000] [--drop 0.01] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) for the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` with the vertex fans of
`--fans` random vertices and the fraction `--drop` of random faces removed: `fill_holes(max_edges)` end to end and the adjacency build (wall
clock), and the rim keys kernel, the sort of its keys, the loop kernel and the emit kernel (device events around BATCH launches back to back).
Beside them the numpy specification tests/fill_spec.py on this machine's CPU on the same mesh (checked against the device, bit for bit) --
the only baseline there is for a new capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, fill, mcubes, topology  # noqa: E402
import fill_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402

BATCH = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--max_edges', type=int, default=16)
    ap.add_argument('--fans', type=int, default=2000)
    ap.add_argument('--drop', type=float, default=0.01)
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
    whole = int(faces.shape[0])
    rng = np.random.default_rng(0)
    hf = faces.cpu().numpy()
    hf = S.without_fans(hf[rng.random(whole) >= args.drop], rng.choice(int(verts.shape[0]), size=args.fans, replace=False))
    faces = torch.from_numpy(hf).to(dev).contiguous()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    offsets, nbr, mult, _ = topology.adjacency_rows(faces, nv)
    ne = int(nbr.shape[0])
    succ, cand, rim_edges, _, _ = topology.rim_rows(faces, nv, offsets, nbr, mult)
    nc = int(cand.shape[0])
    out_v, out_f, info = fill.fill_holes(verts, faces, args.max_edges)
    print('sphere R={}: {} of {} faces, {} vertices, {} rim half-edges, {} candidates'.format(R, nf, whole, nv, rim_edges, nc))
    print('  fill_holes: {}'.format(info))
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    found = torch.zeros(nc, dtype=torch.int32, device=dev)
    _lib.call('ppsx_fill_rim_keys', faces, nf, nv, offsets, nbr, mult, ne, keys)
    _lib.call('ppsx_fill_loops', cand, nc, succ, nv, args.max_edges, found)
    keep = found > 0
    leader, length = cand[keep].contiguous(), found[keep].contiguous()
    nl = int(leader.shape[0])
    fan = (length > 3).to(torch.int64)
    rows = torch.where(length > 3, length.to(torch.int64), torch.ones_like(fan))
    vslot, foff = torch.cumsum(fan, 0) - fan, torch.cumsum(rows, 0) - rows
    nnew, nfnew = int(fan.sum().item()), int(rows.sum().item())
    new_v, new_f = torch.zeros(nnew, 3, dtype=torch.float32, device=dev), torch.full((nfnew, 3), -1, dtype=torch.int64, device=dev)

    def batch(fn):
        def run():
            for _ in range(BATCH):
                fn()
        return run

    timed = [('fill_holes(max_edges={}) end to end, wall'.format(args.max_edges), 1, wall_ms(lambda: fill.fill_holes(verts, faces, args.max_edges), args.reps)),
             ('adjacency (ppsx_smooth_half_edges + sort + unique_consecutive + bincount + cumsum), wall', 1,
              wall_ms(lambda: topology.adjacency_rows(faces, nv), args.reps)),
             ('rim rows (ppsx_fill_rim_keys + sort + bincounts + succ), wall', 1, wall_ms(lambda: topology.rim_rows(faces, nv, offsets, nbr, mult), args.reps)),
             ('ppsx_fill_rim_keys, device events', BATCH,
              device_ms(batch(lambda: _lib.call('ppsx_fill_rim_keys', faces, nf, nv, offsets, nbr, mult, ne, keys)), args.reps)),
             ('torch.sort of the {} rim keys, device events'.format(3 * nf), BATCH, device_ms(batch(lambda: torch.sort(keys)), args.reps)),
             ('ppsx_fill_loops, device events', BATCH,
              device_ms(batch(lambda: _lib.call('ppsx_fill_loops', cand, nc, succ, nv, args.max_edges, found)), args.reps)),
             ('ppsx_fill_emit ({} loops), device events'.format(nl), BATCH,
              device_ms(batch(lambda: _lib.call('ppsx_fill_emit', verts, nv, succ, leader, length, vslot, foff, nl, new_v, nnew, new_f, nfnew)), args.reps))]
    print('GPU ({} reps after warm-up; device-event rows are one launch of {} back to back):'.format(args.reps, BATCH))
    for name, per, (med, lo_) in timed:
        print('  {:<92s} median {:10.4f} ms  min {:10.4f} ms'.format(name, med / per, lo_ / per))
    kernels = sum(t[2][0] / t[1] for t in timed[3:] if t[0].startswith('ppsx_'))
    print('  the three kernels together {:.4f} ms; one adjacency build {:.4f} ms'.format(kernels, timed[1][2][0]))
    if args.no_cpu:
        return
    hv = verts.cpu().numpy()
    t0 = time.perf_counter()
    want_v, want_f, want_info = S.fill_spec(hv, hf, args.max_edges)
    dt = (time.perf_counter() - t0) * 1e3
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    print('  {:<92s} {:10.1f} ms'.format('fill_spec(max_edges={}) on the same mesh'.format(args.max_edges), dt))
    assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes() and info == want_info, \
        'the device differs from the specification'
    print('  the device equals the specification on all {} vertices and {} faces'.format(want_v.shape[0], want_f.shape[0]))


if __name__ == '__main__':
    main()
