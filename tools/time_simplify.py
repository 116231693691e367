"""Rates of the mesh simplification (ppsurf_amd/simplify.py, csrc/pps_simplify.hip).
    python tools/time_simplify.py [--res 257] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) on the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`: one counting pass (leaders +
survivor count) at the grid a 100 000-face budget chooses, the whole 20-pass budget search with its host round trips, the simplification at that
grid (cluster ids, two CSRs, placement, face remap and compaction), and `simplify_mesh` end to end at budgets 100 000 and 20 000.  Beside them the
same stages of the numpy specification tests/simplify_spec.py on this machine's CPU (one run each), the only baseline there is for a new
capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import ops, simplify  # noqa: E402
import simplify_spec as S  # noqa: E402
from timing import wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--budgets', type=int, nargs='+', default=[100000, 20000])
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    x = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(x, x, x, indexing='ij')
    verts, faces = ops.marching_cubes((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts = (verts * (1.0 / (R - 1)) - 0.5).contiguous()
    grid = simplify.ClusterGrid(verts, faces)
    print('sphere R={}: {} vertices, {} faces; table of {} slots'.format(R, grid.nv, grid.nf, grid.capacity))
    rows, chosen = [], {}
    for budget in args.budgets:
        G = grid.search(budget)
        _, _, rep = grid.run(G=G)
        chosen[budget] = G
        print('budget {}: {}'.format(budget, rep))
        if budget == args.budgets[0]:
            rows.append(('one counting pass at G = {} (leaders + survivor count, one host read)'.format(G), wall_ms(lambda: grid.count(G), args.reps)))
            rows.append(('budget search, 20 counting passes (host loop)', wall_ms(lambda: grid.search(budget), args.reps)))
        rows.append(('simplification at G = {} (ids, CSRs, placement, faces)'.format(G), wall_ms(lambda: grid.run(G=G), args.reps)))
        rows.append(('simplify_mesh end to end, budget {}'.format(budget), wall_ms(lambda: simplify.simplify_mesh(verts, faces, max_faces=budget), args.reps)))
    print('GPU ({} reps after warm-up):'.format(args.reps))
    for name, (med, lo_) in rows:
        print('  {:<72s} median {:10.3f} ms  min {:10.3f} ms'.format(name, med, lo_))
    if args.no_cpu:
        return
    print('CPU (numpy specification, one run each, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()

    def cpu(name, fn):
        t0 = time.perf_counter()
        out = fn()
        print('  {:<72s} {:10.1f} ms'.format(name, (time.perf_counter() - t0) * 1e3))
        return out
    budget = args.budgets[0]
    cpu('one counting pass at G = {}'.format(chosen[budget]), lambda: S.count(hv, hf, chosen[budget]))
    assert cpu('budget search, 20 counting passes', lambda: S.budget_search(hv, hf, budget)) == chosen[budget]
    for budget in args.budgets:
        want = cpu('simplification at G = {}'.format(chosen[budget]), lambda: S.simplify(hv, hf, chosen[budget]))
        got_v, got_f, _ = grid.run(G=chosen[budget])
        assert np.array_equal(got_f.cpu().numpy(), want['faces']) and np.array_equal(got_v.cpu().numpy(), want['verts'])


if __name__ == '__main__':
    main()
