"""Rates of the weld stage (ppsurf_amd/weld.py, csrc/pps_weld.hip).
    python tools/time_weld.py [--res 257] [--reps 10] [--spec_faces 4096] [--no_cpu]
-> median ms (after one warm-up round) for the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`, exploded into a
soup: every face gets private copies of its corners and the rows are shuffled (seeded).  At eps = 0 and at a small positive eps, a
hundredth of the shortest edge: `weld_mesh` end to end, and its parts: the cell lists (trim.SupportGrid: slot kernel, sort, counts), the
labelling on those lists (the rounds of hook and compress with one flag read each) with its number of rounds, and the face kernel (device
events around BATCH launches back to back).  The welded soup must be the indexed mesh again, in the numbering of the first copies.  The
numpy specification tests/weld_spec.py is brute force over all pairs, quadratic in the rows, so it runs on the soup of the first
`--spec_faces` faces on this machine's CPU and is checked there against the device, byte for byte."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, mcubes, trim, weld  # noqa: E402
import weld_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402

BATCH = 20


def lists(v, eps):
    grid = trim.SupportGrid(v)
    return grid.build(grid.edge_for(max(min(eps, float(grid.ext)), weld.H_FLOOR)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--spec_faces', type=int, default=4096)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    nv, nf = hv.shape[0], hf.shape[0]
    assert np.unique(hv, axis=0).shape[0] == nv and np.unique(hf).shape[0] == nv
    sv, sf, first = S.soup(hv, hf, 7)
    want_v, want_f = S.welded_soup(hv, hf, first)
    edges = hv[hf].astype(np.float64)
    shortest = float(np.sqrt(((edges - edges[:, [1, 2, 0]]) ** 2).sum(axis=2).min()))
    v, f = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    print('sphere R={}: {} faces, {} vertices; the soup has {} rows; shortest edge {:.3e}'.format(R, nf, nv, sv.shape[0], shortest))
    for eps in (0.0, 0.01 * shortest):
        out_v, out_f, info = weld.weld_mesh(v, f, eps)
        assert info['vertices_out'] == nv and info['faces_out'] == nf, info
        assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes(), 'the welded soup is not the indexed mesh'
        grid = lists(v, eps)
        leader, rounds = weld._clusters(v, eps)
        newrow = (torch.cumsum(leader == torch.arange(sv.shape[0], dtype=torch.int32, device=dev), 0) - 1)[leader.long()].contiguous()
        out, code = torch.empty_like(f), torch.empty(nf, dtype=torch.uint8, device=dev)
        cells = int((grid.offsets[1:] > grid.offsets[:-1]).sum().item())
        print('eps = {:.3e}: {}; cell edge {:.3e}, {} occupied cells, {} labelling rounds'.format(eps, info, float(grid.h), cells, rounds))

        def batch():
            for _ in range(BATCH):
                _lib.call('ppsx_weld_faces', f, nf, sv.shape[0], newrow, out, code)

        lists_ms = wall_ms(lambda: lists(v, eps), args.reps)
        both_ms = wall_ms(lambda: weld._clusters(v, eps), args.reps)
        timed = [('weld_mesh end to end, wall', 1, wall_ms(lambda: weld.weld_mesh(v, f, eps), args.reps)),
                 ('cell lists (box, ppsx_trim_cell_slots, stable sort, counts), wall', 1, lists_ms),
                 ('cell lists and labelling: {} rounds of hook, compress and one flag read, wall'.format(rounds), 1, both_ms),
                 ('the labelling alone (the row above minus the cell lists)', 1, (both_ms[0] - lists_ms[0], both_ms[1] - lists_ms[1])),
                 ('ppsx_weld_faces, device events', BATCH, device_ms(batch, args.reps))]
        print('  GPU ({} reps after warm-up; device-event rows are one launch of {} back to back):'.format(args.reps, BATCH))
        for name, per, (med, lo_) in timed:
            print('    {:<90s} median {:10.4f} ms  min {:10.4f} ms'.format(name, med / per, lo_ / per))
        if args.no_cpu:
            continue
        k = min(args.spec_faces, nf)
        pv, pf, _ = S.soup(hv, hf[:k], 8)
        t0 = time.perf_counter()
        spec_v, spec_f, spec_info, _ = S.weld_spec(pv, pf, eps)
        dt = (time.perf_counter() - t0) * 1e3
        got_v, got_f, got_info = weld.weld_mesh(torch.from_numpy(pv).to(dev), torch.from_numpy(pf).to(dev), eps)
        assert got_v.cpu().numpy().tobytes() == spec_v.tobytes() and got_f.cpu().numpy().tobytes() == spec_f.tobytes() and got_info == spec_info, \
            'the device differs from the specification'
        print('  CPU (numpy specification, one run, {} threads visible): weld_spec on the soup of the first {} faces ({} rows) {:10.1f} ms;'
              ' quadratic in the rows, so about {:.0f} s for all {}; the device equals it on those rows, byte for byte'.format(
                  os.environ.get('OMP_NUM_THREADS', '?'), k, pv.shape[0], dt, dt * 1e-3 * (sv.shape[0] / pv.shape[0]) ** 2, sv.shape[0]))


if __name__ == '__main__':
    main()
