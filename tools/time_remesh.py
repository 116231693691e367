"""Rates and quality of the isotropic remeshing (ppsurf_amd/remesh.py, csrc/pps_remesh.hip) on a Marching Cubes sphere.
    python tools/time_remesh.py [--res 257] [--reps 10] [--factor 1.0] [--iters 5] [--no_cpu]
-> on the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`: `remesh_isotropic` end to end (median ms after one
warm-up run, wall clock around a synchronise) and where a run spends its time -- the median, the splits, the collapses, the flips and the
relaxation -- from one run with a synchronise between the parts; `collapse_short_edges` alone with its own parts (the rebuilds of the rows
against the kernels with their host read and the apply) and its time per round beside a round of `decimate_mesh`; one relaxation pass beside
two passes of `smooth_mesh`.  For the input and the output: the faces, the histogram of the corner angles, the smallest angle, the spread of
the edge lengths and the crossing faces that `intersect` finds.  With the CPU part: the numpy specification tests/remesh_spec.py on a small
sphere (`--cpu_res`), checked against the device byte for byte."""
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
from ppsurf_amd import decimate, intersect, remesh, smooth, subdivide, topology  # noqa: E402
from timing import parts_of, sphere, wall_ms  # noqa: E402

BINS = (0, 10, 20, 30, 40, 50, 60, 90, 120, 180.0001)


def quality(verts, faces):
    """faces, the corner-angle histogram over BINS, the smallest angle, the edge lengths' coefficient of variation and min / median / max in
    units of the median, and the crossing pairs of `intersect`."""
    import remesh_spec as R
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    import flip_spec
    a = flip_spec.angles(v, f[R.valid_faces(f, v.shape[0])])
    e = R.edge_lengths(v, f)
    med = float(np.median(e))
    return {'faces': int(f.shape[0]), 'vertices': int(v.shape[0]), 'corner_histogram': np.histogram(a, bins=np.array(BINS))[0].tolist(),
            'smallest_angle': float(a.min()), 'corners_below_30': float((a < 30.0).mean()), 'edge_cv': float(e.std() / e.mean()),
            'edge_min_med_max': [float(e.min() / med), med, float(e.max() / med)],
            'crossing_pairs': intersect.self_intersections(verts, faces)[1]['pairs']}


def shown(parts):
    total = sum(parts.values())
    return '{:.2f} ms: '.format(total) + ', '.join('{} {:.2f} ms ({:.0f} %)'.format(k, ms, 100.0 * ms / total) for k, ms in parts.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--factor', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--cpu_res', type=int, default=25)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    verts, faces = sphere(args.res, dev)
    print('sphere R={}, bins {}'.format(args.res, BINS))
    print('  input   {}'.format(quality(verts, faces)))
    out_v, out_f, info = remesh.remesh_isotropic(verts, faces, factor=args.factor, iters=args.iters)
    print('  remesh_isotropic(factor={}, iters={})  {}'.format(args.factor, args.iters, info))
    print('  output  {}'.format(quality(out_v, out_f)))
    med, low = wall_ms(lambda: remesh.remesh_isotropic(verts, faces, factor=args.factor, iters=args.iters), args.reps)
    print('  end to end median {:.2f} ms  min {:.2f} ms'.format(med, low))
    v, f = topology.checked_mesh('time_remesh', verts, faces, limit=True)
    params = remesh._checked_remesh(None, args.factor, args.iters, 0.5, 10.0, None)
    print('  one run with a synchronise between the parts, ' + shown(parts_of(lambda timer: remesh._remeshed(v, f, *params, timer=timer))))
    low_edge, high_edge = info['low'], info['high']
    c_v, c_f, c_info = remesh.collapse_short_edges(verts, faces, low_edge, high_edge)
    med, _ = wall_ms(lambda: remesh.collapse_short_edges(verts, faces, low_edge, high_edge), args.reps)
    rounds = max(c_info['rounds'], 1)
    print('  collapse_short_edges alone  {}'.format(c_info))
    print('                 median {:.2f} ms, {} rounds and one last evaluation, {:.3f} ms per evaluation'.format(med, c_info['rounds'], med / (rounds + 1)))
    print('                 ' + shown(parts_of(lambda timer: remesh._collapsed(v, f, low_edge, high_edge, 1000, timer=timer))))
    budget = int(faces.shape[0]) - 2 * max(c_info['collapses'], 1)
    d_info = decimate.decimate_mesh(verts, faces, budget)[2]
    med, _ = wall_ms(lambda: decimate.decimate_mesh(verts, faces, budget), args.reps)
    print('  decimate_mesh to the same face count: median {:.2f} ms, {} rounds, {:.3f} ms per round'.format(med, d_info['rounds'], med / max(d_info['rounds'], 1)))
    one, _ = wall_ms(lambda: remesh.relax_tangential(verts, faces, 1, 0.5), args.reps)
    eleven, _ = wall_ms(lambda: remesh.relax_tangential(verts, faces, 11, 0.5), args.reps)
    s_one, _ = wall_ms(lambda: smooth.smooth_mesh(verts, faces, 1, 0.5, -0.53), args.reps)
    s_eleven, _ = wall_ms(lambda: smooth.smooth_mesh(verts, faces, 11, 0.5, -0.53), args.reps)
    print('  relax_tangential: 1 pass {:.2f} ms, 11 passes {:.2f} ms: {:.3f} ms per pass; smooth_mesh: 1 iteration {:.2f} ms, 11 {:.2f} ms: '
          '{:.3f} ms per two passes'.format(one, eleven, (eleven - one) / 10.0, s_one, s_eleven, (s_eleven - s_one) / 10.0))
    if args.no_cpu:
        return
    import remesh_spec as R
    small_v, small_f = sphere(args.cpu_res, dev)
    hv, hf = small_v.cpu().numpy(), small_f.cpu().numpy()
    low, high = 0.8 * subdivide.median_edge(small_v, small_f), 4.0 / 3.0 * subdivide.median_edge(small_v, small_f)
    for name, device, spec in (('remesh_isotropic', lambda: remesh.remesh_isotropic(small_v, small_f, factor=args.factor, iters=args.iters),
                                lambda: R.remesh_spec(hv, hf, factor=args.factor, iters=args.iters)),
                               ('collapse_short_edges', lambda: remesh.collapse_short_edges(small_v, small_f, low, high),
                                lambda: R.collapse_spec(hv, hf, low, high)),
                               ('relax_tangential', lambda: remesh.relax_tangential(small_v, small_f, 3, 0.5), lambda: R.relax_spec(hv, hf, 3, 0.5))):
        out_v, out_f, info = device()
        t0 = time.perf_counter()
        want_v, want_f, want_info = spec()
        dt = (time.perf_counter() - t0) * 1e3
        med, _ = wall_ms(device, args.reps)
        assert out_v.cpu().numpy().tobytes() == want_v.tobytes() and out_f.cpu().numpy().tobytes() == want_f.tobytes() and info == want_info, \
            '{}: the device differs from the specification'.format(name)
        print('CPU (numpy specification, one run) {}: sphere R={}, {} faces -> {}: {:.0f} ms against {:.2f} ms on the device; the bytes are equal'.format(
            name, args.cpu_res, int(small_f.shape[0]), int(want_f.shape[0]), dt, med))


if __name__ == '__main__':
    main()
