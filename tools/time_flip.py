"""Rates and quality of the Delaunay edge flips (ppsurf_amd/flip.py, csrc/pps_flip.hip).
    python tools/time_flip.py [--res 257] [--reps 10] [--budget 100000] [--no_cpu]
-> on the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` as written, and on the same sphere after `decimate_mesh`
to `--budget` faces: `flip_edges` end to end (median ms after one warm-up round, wall clock around a synchronise), its rounds and flips, the
time per round, and where a run spends its time -- the edge sort with keys, owners and pairs against the two kernels with their host read
and the apply -- from one run with a synchronise between the parts.  Before and after: the smallest corner angle, the share of corners below
5, 10, 20 and 30 degrees, and the edges that do not have exactly two owners.  With the CPU part: the numpy specification tests/flip_spec.py
on a small sphere (`--cpu_res`), checked against the device byte for byte."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
from ppsurf_amd import decimate, flip, topology  # noqa: E402
from timing import parts_of, sphere, wall_ms  # noqa: E402

BINS = (5.0, 10.0, 20.0, 30.0)


def shape(verts, faces):
    """The smallest corner angle in degrees, the share of the corners below every bound of BINS, the edges without exactly two owners."""
    p = verts.double()[faces]
    corners = []
    for i in range(3):
        u, w = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        corners.append(torch.rad2deg(torch.atan2(torch.cross(u, w, dim=1).norm(dim=1), (u * w).sum(dim=1))))
    a = torch.stack(corners, dim=1).reshape(-1)
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    owners = torch.unique((e.min(dim=1)[0] << 32) | e.max(dim=1)[0], return_counts=True)[1]
    out = {'min_angle': round(float(a.min().item()), 3), 'edges_not_2': int((owners != 2).sum().item())}
    out.update({'below_{:.0f}'.format(b): round(float((a < b).double().mean().item()), 5) for b in BINS})
    return out


def run_case(name, verts, faces, reps):
    out_v, out_f, info = flip.flip_edges(verts, faces)
    print('{}: {} vertices, {} faces'.format(name, int(verts.shape[0]), int(faces.shape[0])))
    print('  flip_edges  {}'.format(info))
    print('              before {}'.format(shape(verts, faces)))
    print('              after  {}'.format(shape(out_v, out_f)))
    med, low = wall_ms(lambda: flip.flip_edges(verts, faces), reps)
    evaluations = info['rounds'] + 1
    print('              end to end median {:.2f} ms  min {:.2f} ms; {} rounds and one last evaluation, {:.3f} ms per evaluation'.format(
        med, low, info['rounds'], med / evaluations))
    v, f = topology.checked_mesh('time_flip', verts, faces, limit=True)
    parts = parts_of(lambda timer: flip._flipped(v, f, 10.0, 1e-6, 100, timer=timer))
    total = sum(parts.values())
    print('              one run with a synchronise between the parts, {:.2f} ms: '.format(total) +
          ', '.join('{} {:.2f} ms ({:.0f} %)'.format(k, parts.get(k, 0.0), 100.0 * parts.get(k, 0.0) / total) for k in ('sort', 'kernels', 'apply', 'output')))


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
    run_case('sphere R={} as written'.format(args.res), verts, faces, args.reps)
    dec_v, dec_f, dec_info = decimate.decimate_mesh(verts, faces, args.budget)
    run_case('the same after decimate_mesh to {} faces'.format(dec_info['faces_out']), dec_v.contiguous(), dec_f.contiguous(), args.reps)
    if args.no_cpu:
        return
    import flip_spec as S
    small_v, small_f = sphere(args.cpu_res, dev)
    out_v, out_f, info = flip.flip_edges(small_v, small_f)
    t0 = time.perf_counter()
    _, want_f, want_info = S.flip_spec(small_v.cpu().numpy(), small_f.cpu().numpy())
    dt = (time.perf_counter() - t0) * 1e3
    med, _ = wall_ms(lambda: flip.flip_edges(small_v, small_f), args.reps)
    print('CPU (numpy specification, one run): sphere R={}, {} faces: {:.0f} ms against {:.2f} ms on the device, {} rounds, {} flips'.format(
        args.cpu_res, int(small_f.shape[0]), dt, med, info['rounds'], info['flips']))
    assert out_f.cpu().numpy().tobytes() == want_f.tobytes() and info == want_info, 'the device differs from the specification'
    print('  the device equals the specification on all {} faces'.format(want_f.shape[0]))


if __name__ == '__main__':
    main()
