"""Rates of the removal of isolated pieces (ppsurf_amd/pieces.py, csrc/pps_pieces.hip).
    python tools/time_pieces.py [--res 257] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) for the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` plus fragments: a quarter-size
copy of it beside it with half of its faces removed at random (the pattern of tests/pieces_spec.py `debris`).  `remove_pieces(keep_largest=1)`
end to end, and its parts: the pairs (key kernel, sort, runs of two), the labelling with its number of rounds, the statistics and the
selection (device events around BATCH launches back to back).  The statistics also run on the sphere's faces alone as ONE component, as one
component per wave and as 4096 components interleaved lane by lane: if the first is far above the second, the combine before the atomics is
not working.  For comparison only: `ops.mesh_small_components(k = 6)`, which makes the same pass over the edges, on the same mesh, and the
numpy specification tests/pieces_spec.py on this machine's CPU (checked against the device, byte for byte)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, mcubes, ops, pieces, topology  # noqa: E402
import pieces_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402

BATCH = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    sphere_v = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    sphere_f = faces.contiguous()
    snv, snf = int(sphere_v.shape[0]), int(sphere_f.shape[0])
    some = torch.from_numpy(np.random.default_rng(5).random(snf) < 0.5).to(dev)
    shift = torch.tensor([1.0, 0.0, 0.0], device=dev)
    verts = torch.cat([sphere_v, sphere_v * 0.25 + shift]).contiguous()
    faces = torch.cat([sphere_f, sphere_f[some] + snv]).contiguous()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])

    out_v, out_f, info = pieces.remove_pieces(verts, faces, keep_largest=1)
    table = pieces._table(verts, faces)
    nc = int(table['leader'].shape[0])
    fa, fb, _ = topology.manifold_pairs(faces, nv)
    print('sphere R={} ({} faces) plus fragments: {} faces, {} vertices, {} pairs, {} components, {} labelling rounds'.format(
        R, snf, nf, nv, int(fa.shape[0]), nc, table['rounds']))
    print('  remove_pieces(keep_largest=1): {}'.format(info))
    rank = pieces._rank(table['faces'])
    keep = torch.empty(nc, dtype=torch.uint8, device=dev)
    count, lo, hi = torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(nc, 3, device=dev), torch.empty(nc, 3, device=dev)

    def batch(fn):
        def run():
            for _ in range(BATCH):
                fn()
        return run

    def stats_ms(f, label, cid, n):
        c, l, h = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
        return device_ms(batch(lambda: _lib.call('ppsx_pieces_stats', verts, nv, f, int(f.shape[0]), label, cid, n, c, l, h)), args.reps)

    own = torch.arange(snf, dtype=torch.int32, device=dev)
    zero = torch.zeros_like(own)
    per_wave, mixed = (own // 64).contiguous(), (own % 4096).contiguous()
    timed = [('remove_pieces(keep_largest=1) end to end, wall', 1, wall_ms(lambda: pieces.remove_pieces(verts, faces, keep_largest=1), args.reps)),
             ('pairs (ppsx_pieces_edge_keys + sort with indices + runs of two), wall', 1, wall_ms(lambda: topology.manifold_pairs(faces, nv), args.reps)),
             ('pairs + labelling ({} rounds of hook, compress and one flag read), wall'.format(table['rounds']), 1,
              wall_ms(lambda: pieces._labels(faces, nv), args.reps)),
             ('ppsx_pieces_stats, the mesh ({} components), device events'.format(nc), BATCH,
              device_ms(batch(lambda: _lib.call('ppsx_pieces_stats', verts, nv, faces, nf, table['label'], table['cid'], nc, count, lo, hi)), args.reps)),
             ('ppsx_pieces_stats, the sphere as ONE component, device events', BATCH, stats_ms(sphere_f, zero, zero, 1)),
             ('ppsx_pieces_stats, the sphere as one component per wave ({}), device events'.format((snf + 63) // 64), BATCH,
              stats_ms(sphere_f, zero, per_wave, (snf + 63) // 64)),
             ('ppsx_pieces_stats, the sphere as 4096 components lane by lane, device events', BATCH, stats_ms(sphere_f, zero, mixed, 4096)),
             ('ppsx_pieces_select ({} components, three rules), device events'.format(nc), BATCH,
              device_ms(batch(lambda: _lib.call('ppsx_pieces_select', table['faces'], table['lo'], table['hi'], rank, nc, 1, 500, 1, 0.1, 1, 1,
                                                table['box_diag2'], keep)), args.reps)),
             ('for comparison: ops.mesh_small_components(k = 6) on the same mesh, wall', 1,
              wall_ms(lambda: ops.mesh_small_components(faces, nv, 6), args.reps))]
    print('GPU ({} reps after warm-up; device-event rows are one launch of {} back to back):'.format(args.reps, BATCH))
    for name, per, (med, lo_) in timed:
        print('  {:<92s} median {:10.4f} ms  min {:10.4f} ms'.format(name, med / per, lo_ / per))
    if args.no_cpu:
        return
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    t0 = time.perf_counter()
    want_v, want_f, want_info, _ = S.remove_spec(hv, hf, None, None, 1)
    dt = (time.perf_counter() - t0) * 1e3
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    print('  {:<92s} {:10.1f} ms'.format('remove_spec(keep_largest=1) on the same mesh', dt))
    assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes() and info == want_info, \
        'the device differs from the specification'
    print('  the device equals the specification on all {} vertices and {} faces'.format(want_v.shape[0], want_f.shape[0]))


if __name__ == '__main__':
    main()
