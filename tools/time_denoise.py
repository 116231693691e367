"""Rates of the feature-preserving denoising (ppsurf_amd/denoise.py, csrc/pps_denoise.hip).
    python tools/time_denoise.py [--res 257] [--threshold 0.5] [--normal_iters 5] [--vertex_iters 10] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) for the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`: the incidence build
(corner-key kernel, sort, row offsets), the face normals, one filter pass and one vertex pass (device events around 100 launches back to
back) and `denoise_mesh` end to end.  Beside them the numpy specification tests/denoise_spec.py on this machine's CPU on the same mesh
(checked against the device, bit for bit) -- the only baseline there is for a new capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, denoise, mcubes, topology  # noqa: E402
import denoise_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402

BATCH = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--threshold', type=float, default=0.5)
    ap.add_argument('--normal_iters', type=int, default=5)
    ap.add_argument('--vertex_iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R, T = args.res, args.threshold
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    faces = faces.contiguous()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    offsets, inc = topology.vertex_incidence(faces, nv)
    ni = int(inc.shape[0])
    deg = offsets[1:] - offsets[:-1]
    print('sphere R={}: {} faces, {} vertices, {} corners, faces per vertex max {} mean {:.2f}'.format(R, nf, nv, ni, int(deg.max().item()), ni / nv))
    n, m = denoise.filtered_face_normals(verts, faces, T, 0), torch.empty(nf, 3, dtype=torch.float64, device=dev)
    x, y = verts.double(), torch.empty(nv, 3, dtype=torch.float64, device=dev)

    def batch(fn):                                    # BATCH launches between two events: one launch alone is too short to time
        def run():
            for _ in range(BATCH):
                fn()
        return run

    def filter_passes():
        for _ in range(BATCH // 2):
            _lib.call('ppsx_denoise_filter_pass', faces, nf, nv, offsets, inc, ni, n, T, m)
            _lib.call('ppsx_denoise_filter_pass', faces, nf, nv, offsets, inc, ni, m, T, n)

    def vertex_passes():
        for _ in range(BATCH // 2):
            _lib.call('ppsx_denoise_vertex_pass', x, nv, faces, nf, n, offsets, inc, ni, y)
            _lib.call('ppsx_denoise_vertex_pass', y, nv, faces, nf, n, offsets, inc, ni, x)

    rows = [('incidence (ppsx_normals_corner_keys + sort + bincount + cumsum), wall', 1, wall_ms(lambda: topology.vertex_incidence(faces, nv), args.reps)),
            ('ppsx_denoise_face_normals, device events', BATCH,
             device_ms(batch(lambda: _lib.call('ppsx_denoise_face_normals', verts, nv, faces, nf, m)), args.reps)),
            ('ppsx_denoise_filter_pass, device events', BATCH, device_ms(filter_passes, args.reps)),
            ('ppsx_denoise_vertex_pass, device events', BATCH, device_ms(vertex_passes, args.reps)),
            ('denoise_mesh({}, {}, {}) end to end, wall'.format(T, args.normal_iters, args.vertex_iters), 1,
             wall_ms(lambda: denoise.denoise_mesh(verts, faces, T, args.normal_iters, args.vertex_iters), args.reps))]
    print('GPU ({} reps after warm-up; the kernels {} launches back to back, per launch):'.format(args.reps, BATCH))
    for name, per, (med, lo_) in rows:
        print('  {:<80s} median {:10.4f} ms  min {:10.4f} ms'.format(name, med / per, lo_ / per))
    out_v, _, info = denoise.denoise_mesh(verts, faces, T, args.normal_iters, args.vertex_iters)
    print('  denoise_mesh: {}'.format(info))
    if args.no_cpu:
        return
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    t0 = time.perf_counter()
    want = S.denoise_spec(hv, hf, T, args.normal_iters, args.vertex_iters)
    dt = (time.perf_counter() - t0) * 1e3
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    print('  {:<80s} {:10.1f} ms'.format('denoise_spec({}, {}, {}) on the same mesh'.format(T, args.normal_iters, args.vertex_iters), dt))
    assert out_v.cpu().numpy().tobytes() == want.tobytes(), 'the device differs from the specification'
    print('  the device equals the specification on all {} vertices'.format(nv))


if __name__ == '__main__':
    main()
