"""Rates of the self-intersection stage (ppsurf_amd/intersect.py, csrc/pps_intersect.hip).
    python tools/time_intersect.py [--res 257] [--reps 10] [--no_stages] [--no_cpu]
-> on the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`, alone and with a shifted copy of itself:
`self_intersections(return_pairs=True)` end to end (median ms after one warm-up round, wall clock around a synchronise), the pairs and the
flagged faces, the split of the broad phase (cell edge, small and large faces, boxed pairs) and where a run spends its time -- boxes, cell
lists, count with its host read, emit with the prefix sum and the sort -- as medians over runs with a synchronise between the parts.  Then
the yardstick of DESIGN.md section 29: the faces that cross another one after `smooth`, `denoise`, `simplify`, `decimate` and `fill` after a
trim on that sphere.  With the CPU part: the numpy specification tests/intersect_spec.py on the two 320-face icospheres, checked against
the device byte for byte."""
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
from ppsurf_amd import decimate, denoise, fill, intersect, simplify, smooth, trim  # noqa: E402
from timing import parts_of, sphere, wall_ms  # noqa: E402

PARTS = ('boxes', 'lists', 'count', 'emit', 'output')
SHIFT = (0.25, 0.04, 0.02)


def parts_ms(verts, faces, reps):
    """{part: median ms} over `reps` runs (after one warm-up) of one walk with a synchronise between the parts."""
    rows = []
    for rep in range(reps + 1):
        parts = parts_of(lambda timer: intersect._walk(verts, faces, intersect.MAX_PAIRS, True, timer=timer))
        if rep > 0:
            rows.append(parts)
    return {p: float(np.median([r.get(p, 0.0) for r in rows])) for p in PARTS}


def run_case(name, verts, faces, reps):
    flags, pairs, info = intersect.self_intersections(verts, faces, return_pairs=True)
    lo, hi, ext, live = intersect.face_boxes(verts, faces)
    edge = intersect.cell_edge(ext, live)
    lists = intersect._Lists(lo, ext, live, edge, None, None)
    print('{}: {} vertices, {} faces'.format(name, int(verts.shape[0]), int(faces.shape[0])))
    print('  self_intersections  {}'.format(info))
    print('              broad phase: cell edge {:.6g} (large above {:.6g}), {} small faces in the cells, {} large faces in the list'.format(
        lists.h, edge, int(lists.small.shape[0]), int(lists.large.shape[0])))
    med, low = wall_ms(lambda: intersect.self_intersections(verts, faces, return_pairs=True), reps)
    print('              end to end median {:.2f} ms  min {:.2f} ms'.format(med, low))
    parts = parts_ms(verts, faces, reps)
    total = sum(parts.values())
    print('              with a synchronise between the parts, {:.2f} ms: '.format(total) +
          ', '.join('{} {:.2f} ms ({:.0f} %)'.format(p, parts[p], 100.0 * parts[p] / total) for p in PARTS))
    return info


def stages(verts, faces):
    """faces_intersecting after the stages that move or replace faces: the yardstick."""
    def crossing(v, f):
        info = intersect.self_intersections(v.contiguous(), f.contiguous())[1]
        return '{} of {} faces cross another one ({} pairs)'.format(info['faces_intersecting'], info['faces_in'], info['pairs'])
    print('the yardstick: faces that cross another face after a stage, on the sphere of {} faces'.format(int(faces.shape[0])))
    print('  as given                      {}'.format(crossing(verts, faces)))
    print('  smooth --iters 10             {}'.format(crossing(*smooth.smooth_mesh(verts, faces, 10)[:2])))
    print('  denoise                       {}'.format(crossing(*denoise.denoise_mesh(verts, faces)[:2])))
    out = simplify.simplify_mesh(verts, faces, max_faces=20000)
    print('  simplify --max_faces 20000    {}'.format(crossing(out[0].float(), out[1])))
    print('  decimate --max_faces 20000    {}'.format(crossing(*decimate.decimate_mesh(verts, faces, 20000)[:2])))
    rng = np.random.RandomState(43)
    d = rng.randn(100000, 3)
    cloud = torch.from_numpy((0.35 * d / np.linalg.norm(d, axis=1, keepdims=True) + 0.001 * rng.randn(100000, 3)).astype(np.float32)).to(verts.device)
    cut_v, cut_f, cut = trim.trim_mesh(cloud, verts, faces, 0.5 * trim.cloud_spacing(cloud))
    fill_v, fill_f, filled = fill.fill_holes(cut_v.contiguous(), cut_f.contiguous(), 64)
    print('  trim --factor 0.5 (100 000 points): {} of {} faces left; {}'.format(cut['faces_out'], cut['faces_in'], crossing(cut_v, cut_f)))
    print('  fill --max_edges 64 after it  {}; fill: {}'.format(crossing(fill_v, fill_f), filled))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_stages', action='store_true')
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    verts, faces = sphere(args.res, dev)
    run_case('sphere R={}'.format(args.res), verts, faces, args.reps)
    moved = (verts.double() + torch.tensor(SHIFT, dtype=torch.float64, device=dev)).float()
    run_case('sphere R={} and a copy moved by {}'.format(args.res, SHIFT), torch.cat([verts, moved]).contiguous(),
             torch.cat([faces, faces + verts.shape[0]]).contiguous(), args.reps)
    if not args.no_stages:
        stages(verts, faces)
    if args.no_cpu:
        return
    import intersect_spec as S
    small_v, small_f = S.clean('two icospheres')
    dv, df = torch.from_numpy(small_v).to(dev), torch.from_numpy(small_f).to(dev)
    flags, pairs, info = intersect.self_intersections(dv, df, return_pairs=True)
    t0 = time.perf_counter()
    want_flags, want_pairs, want_info = S.intersect_spec(small_v, small_f)
    dt = (time.perf_counter() - t0) * 1e3
    med, _ = wall_ms(lambda: intersect.self_intersections(dv, df, return_pairs=True), args.reps)
    print('CPU (numpy specification, one run): two icospheres, {} faces, {} pairs: {:.1f} ms against {:.2f} ms on the device'.format(
        int(small_f.shape[0]), want_info['pairs'], dt, med))
    assert flags.cpu().numpy().tobytes() == want_flags.tobytes() and pairs.cpu().numpy().tobytes() == want_pairs.tobytes(), 'the device differs from the specification'
    assert info == want_info, 'the device differs from the specification'
    print('  the device equals the specification on all {} faces and {} pairs'.format(want_flags.shape[0], want_pairs.shape[0]))


if __name__ == '__main__':
    main()
