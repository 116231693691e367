"""Rates of the trim by support (ppsurf_amd/trim.py, csrc/pps_trim.hip).
    python tools/time_trim.py [--res 257] [--points 250000] [--factor 2.0] [--reps 10] [--spec_faces 256] [--no_cpu]
-> median ms (after one warm-up round) for the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` against a cloud of
`--points` noisy points of its UPPER half (the lower half is what a trim removes): the spacing of the cloud, the cell lists (slot kernel,
sort, counts), the support kernel alone, and `trim_mesh` end to end.  Beside them the numpy specification tests/trim_spec.py on this machine's
CPU on the first `--spec_faces` faces spread over the mesh (checked against the kernel, bit for bit) and scaled to all of them -- the only
baseline there is for a new capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import mcubes, trim  # noqa: E402
import trim_spec as S  # noqa: E402
from timing import wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--points', type=int, default=250000)
    ap.add_argument('--factor', type=float, default=2.0)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--spec_faces', type=int, default=256)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    x = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(x, x, x, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    faces = faces.contiguous()
    rng = np.random.RandomState(43)
    d = rng.randn(args.points, 3)
    d[:, 2] = np.abs(d[:, 2])
    cloud_h = (0.35 * d / np.linalg.norm(d, axis=1, keepdims=True) + 0.001 * rng.randn(args.points, 3)).astype(np.float32)
    cloud = torch.from_numpy(cloud_h).to(dev)
    spacing = trim.cloud_spacing(cloud)
    r = float(np.float64(args.factor) * np.float64(spacing))
    nf = int(faces.shape[0])
    print('sphere R={}: {} faces, {} vertices against {} points of the upper half; spacing {:.6g}, factor {} -> r = {:.6g}'.format(
        R, nf, verts.shape[0], args.points, spacing, args.factor, r))
    grid = trim.SupportGrid(cloud)
    h = grid.edge_for(r)
    grid.build(h)
    keep = grid.support(verts, faces, r)
    occupied = int((grid.offsets[1:] > grid.offsets[:-1]).sum().item())
    print('cell edge {:.6g}: grid {} x {} x {}, {} occupied cells, {:.1f} points per occupied cell; {} of {} faces supported'.format(
        float(h), *[int(np.floor((grid.hi[a] - grid.lo[a]) * grid.inv_h)) + 1 for a in range(3)], occupied, args.points / occupied,
        int(keep.sum().item()), nf))
    rows = [('cloud_spacing (block structure + 9-NN of the cloud in itself + kthvalue)', wall_ms(lambda: trim.cloud_spacing(cloud), args.reps)),
            ('cell lists (ppsx_trim_cell_slots + sort + bincount + cumsum)', wall_ms(lambda: grid.build(h), args.reps)),
            ('support kernel (ppsx_trim_face_support)', wall_ms(lambda: grid.support(verts, faces, r), args.reps)),
            ('face_support (box + cell lists + kernel)', wall_ms(lambda: trim.face_support(cloud, verts, faces, r), args.reps)),
            ('trim_mesh end to end (+ small components, compaction)', wall_ms(lambda: trim.trim_mesh(cloud, verts, faces, r), args.reps))]
    print('GPU ({} reps after warm-up):'.format(args.reps))
    for name, (med, lo_) in rows:
        print('  {:<76s} median {:10.3f} ms  min {:10.3f} ms'.format(name, med, lo_))
    out_v, out_f, info = trim.trim_mesh(cloud, verts, faces, r, spacing=spacing)
    print('  trim_mesh: {}'.format(info))
    if args.no_cpu:
        return
    sel = np.linspace(0, nf - 1, min(args.spec_faces, nf)).astype(np.int64)
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()[sel]
    t0 = time.perf_counter()
    want = S.face_support_spec(cloud_h, hv, hf, r)
    dt = (time.perf_counter() - t0) * 1e3
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    print('  {:<76s} {:10.1f} ms  (x {:.1f} = {:.0f} s for all faces)'.format('brute force of {} faces against all points'.format(sel.shape[0]), dt,
                                                                              nf / sel.shape[0], dt * nf / sel.shape[0] / 1e3))
    assert np.array_equal(keep.cpu().numpy()[sel].astype(bool), want), 'the kernel differs from the specification'
    print('  the kernel equals the specification on those {} faces ({} supported)'.format(sel.shape[0], int(want.sum())))


if __name__ == '__main__':
    main()
