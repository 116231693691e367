"""Rates of the longest-edge bisection (ppsurf_amd/subdivide.py, csrc/pps_subdivide.hip).
    python tools/time_subdivide.py [--res 257] [--reps 10] [--budget 100000] [--no_cpu]
-> on the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` after `decimate_mesh` to `--budget` faces, at
`--factor 0.5` and `1.0`: `split_long_edges` end to end (median ms after one warm-up round, wall clock around a synchronise), its rounds and
splits, the faces and the longest edge before and after, the time per evaluation, and where a run spends its time -- the edge sort with
the run table against the four kernels with their host read and the emit with its prefix sums -- from one run with a synchronise between the
parts.  With the CPU part: the numpy specification tests/subdivide_spec.py on a small sphere (`--cpu_res`), checked against the device byte
for byte."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
from ppsurf_amd import decimate, subdivide, topology  # noqa: E402
from timing import parts_of, sphere, wall_ms  # noqa: E402

FACTORS = (0.5, 1.0)


def shape(verts, faces):
    """The longest and the median edge, the smallest corner angle in degrees, the edges without exactly two owners."""
    p = verts.double()[faces]
    corners = []
    for i in range(3):
        u, w = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        corners.append(torch.rad2deg(torch.atan2(torch.cross(u, w, dim=1).norm(dim=1), (u * w).sum(dim=1))))
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    keys, owners = torch.unique((e.min(dim=1)[0] << 32) | e.max(dim=1)[0], return_counts=True)
    length = (verts.double()[keys >> 32] - verts.double()[keys & 0xFFFFFFFF]).norm(dim=1)
    return {'max_edge': round(float(length.max().item()), 6), 'median_edge': round(float(length.median().item()), 6),
            'min_angle': round(float(torch.stack(corners).min().item()), 3), 'edges_not_2': int((owners != 2).sum().item())}


def run_case(name, verts, faces, factor, reps):
    out_v, out_f, info = subdivide.split_long_edges(verts, faces, factor=factor)
    print('{} at factor {}: {} vertices, {} faces'.format(name, factor, int(verts.shape[0]), int(faces.shape[0])))
    print('  split_long_edges  {}'.format(info))
    print('              before {}'.format(shape(verts, faces)))
    print('              after  {}'.format(shape(out_v, out_f)))
    med, low = wall_ms(lambda: subdivide.split_long_edges(verts, faces, factor=factor), reps)
    evaluations = info['rounds'] + 1
    print('              end to end median {:.2f} ms  min {:.2f} ms; {} rounds and one last evaluation, {:.3f} ms per evaluation'.format(
        med, low, info['rounds'], med / evaluations))
    v, f = topology.checked_mesh('time_subdivide', verts, faces, limit=True)
    parts = parts_of(lambda timer: subdivide._subdivided(v, f, None, factor, 100, subdivide.MAX_FACES, timer=timer))
    total = sum(parts.values())
    print('              one run with a synchronise between the parts, {:.2f} ms (the sort of the given faces under sort, the median under kernels): '.format(total) +
          ', '.join('{} {:.2f} ms ({:.0f} %)'.format(k, parts.get(k, 0.0), 100.0 * parts.get(k, 0.0) / total) for k in ('sort', 'kernels', 'emit', 'output')))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--budget', type=int, default=100000)
    ap.add_argument('--cpu_res', type=int, default=33)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    verts, faces = sphere(args.res, dev)
    dec_v, dec_f, dec_info = decimate.decimate_mesh(verts, faces, args.budget)
    dec_v, dec_f = dec_v.contiguous(), dec_f.contiguous()
    for factor in FACTORS:
        run_case('sphere R={} after decimate_mesh to {} faces'.format(args.res, dec_info['faces_out']), dec_v, dec_f, factor, args.reps)
    if args.no_cpu:
        return
    import subdivide_spec as S
    small_v, small_f = sphere(args.cpu_res, dev)
    out_v, out_f, ends, info = subdivide.split_long_edges(small_v, small_f, factor=0.5, return_ends=True)
    t0 = time.perf_counter()
    want_v, want_f, want_ends, want_info = S.subdivide_spec(small_v.cpu().numpy(), small_f.cpu().numpy(), factor=0.5)
    dt = (time.perf_counter() - t0) * 1e3
    med, _ = wall_ms(lambda: subdivide.split_long_edges(small_v, small_f, factor=0.5), args.reps)
    print('CPU (numpy specification, one run): sphere R={}, {} -> {} faces: {:.0f} ms against {:.2f} ms on the device, {} rounds, {} splits'.format(
        args.cpu_res, int(small_f.shape[0]), info['faces_out'], dt, med, info['rounds'], info['splits']))
    assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes(), 'the device differs from the specification'
    assert ends.cpu().numpy().tobytes() == want_ends.tobytes() and info == want_info, 'the device differs from the specification'
    print('  the device equals the specification on all {} faces and {} vertices'.format(want_f.shape[0], want_v.shape[0]))


if __name__ == '__main__':
    main()
