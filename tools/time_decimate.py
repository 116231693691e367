"""Rates and quality of the edge-collapse decimation (ppsurf_amd/decimate.py, csrc/pps_decimate.hip) beside the vertex clustering
(ppsurf_amd/simplify.py) on the same mesh and budgets.
    python tools/time_decimate.py [--res 257] [--reps 10] [--budgets 100000 20000] [--no_cpu]
-> on the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`: `decimate_mesh` end to end (median ms after one warm-up
round, wall clock around a synchronise), its rounds, the time per round, and where a run spends its time -- the rebuilds of the adjacency
and incidence rows against the four kernels, the choice of the winners (flags to a list, one host read) and the apply -- from one run with a
synchronise between the parts.  `simplify_mesh` at the same budgets beside it.  For both outputs: faces whose normal points into the
sphere (flipped), edges that do not have exactly two owners (non-manifold or border), and the RMS and maximum distance of 20 000 input
vertices from the output surface, in units of the Marching Cubes cell.  With the CPU part: the numpy specification tests/decimate_spec.py on a
small sphere (`--cpu_res`), checked against the device byte for byte."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
from ppsurf_amd import decimate, geometry, simplify, topology  # noqa: E402
from timing import parts_of, sphere, wall_ms  # noqa: E402


def quality(verts, faces, query, cell):
    """flipped faces, edges without exactly two owners, RMS and maximum distance of the query points from the surface in cells."""
    p = verts.double()[faces]
    n = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
    flipped = int(((n * p.mean(dim=1)).sum(dim=1) <= 0).sum().item())
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    keys = (e.min(dim=1)[0] << 32) | e.max(dim=1)[0]
    owners = torch.unique(keys, return_counts=True)[1]
    d = geometry.closest_point_on_mesh(verts, faces, query)[1].double()
    return {'flipped': flipped, 'edges_not_2': int((owners != 2).sum().item()), 'rms_cells': float(torch.sqrt((d * d).mean()).item() / cell),
            'max_cells': float(d.max().item() / cell)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--budgets', type=int, nargs='+', default=[100000, 20000])
    ap.add_argument('--cpu_res', type=int, default=33)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    verts, faces = sphere(args.res, dev)
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    cell = 1.0 / (args.res - 1)
    query = verts[torch.from_numpy(np.random.default_rng(0).choice(nv, size=min(20000, nv), replace=False)).to(dev)]
    print('sphere R={}: {} vertices, {} faces; the input itself: {}'.format(args.res, nv, nf, quality(verts, faces, query, cell)))
    for budget in args.budgets:
        out_v, out_f, info = decimate.decimate_mesh(verts, faces, budget)
        print('budget {}:'.format(budget))
        print('  decimate_mesh  {}'.format(info))
        print('                 {}'.format(quality(out_v, out_f, query, cell)))
        med, low = wall_ms(lambda: decimate.decimate_mesh(verts, faces, budget), args.reps)
        rounds = max(info['rounds'], 1)
        print('                 end to end median {:.2f} ms  min {:.2f} ms; {} rounds, {:.3f} ms per round'.format(med, low, info['rounds'], med / rounds))
        v, f = topology.checked_mesh('time_decimate', verts, faces, limit=True)
        parts = parts_of(lambda timer: decimate._decimate_rows(v, f, budget, 1000, timer=timer))
        total = sum(parts.values())
        print('                 one run with a synchronise between the parts, {:.2f} ms: '.format(total) +
              ', '.join('{} {:.2f} ms ({:.0f} %)'.format(k, parts[k], 100.0 * parts[k] / total) for k in ('rows', 'kernels', 'select', 'apply', 'output')))
        s_v, s_f, report = simplify.simplify_mesh(verts, faces, max_faces=budget)
        med, low = wall_ms(lambda: simplify.simplify_mesh(verts, faces, max_faces=budget), args.reps)
        print('  simplify_mesh  {}'.format(report))
        print('                 {}'.format(quality(s_v.float(), s_f, query, cell)))
        print('                 end to end median {:.2f} ms  min {:.2f} ms'.format(med, low))
    if args.no_cpu:
        return
    import decimate_spec as S
    small_v, small_f = sphere(args.cpu_res, dev)
    budget = int(small_f.shape[0]) // 3
    out_v, out_f, info = decimate.decimate_mesh(small_v, small_f, budget)
    t0 = time.perf_counter()
    want_v, want_f, want_info = S.decimate_spec(small_v.cpu().numpy(), small_f.cpu().numpy(), budget)
    dt = (time.perf_counter() - t0) * 1e3
    med, _ = wall_ms(lambda: decimate.decimate_mesh(small_v, small_f, budget), args.reps)
    print('CPU (numpy specification, one run): sphere R={}, {} faces -> {}: {:.0f} ms against {:.2f} ms on the device, {} rounds'.format(
        args.cpu_res, int(small_f.shape[0]), budget, dt, med, info['rounds']))
    assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes() and info == want_info, \
        'the device differs from the specification'
    print('  the device equals the specification on all {} vertices and {} faces'.format(want_v.shape[0], want_f.shape[0]))


if __name__ == '__main__':
    main()
