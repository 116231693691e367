"""Rates of the oriented normals (ppsurf_amd/normals.py, csrc/pps_normals.hip).
    python tools/time_normals.py [--res 257] [--points 250000] [--k 8] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) for the Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res`: the incidence build
(corner-key kernel, sort, row offsets), the vertex kernel alone per weight (device events around 100 launches back to back), `vertex_normals`
end to end per weight, and `point_normals` of a seeded cloud of `--points` points near the sphere at `--k`.  Beside them the numpy specification
tests/normals_spec.py on this machine's CPU on the same mesh (checked against the device, bit for bit) -- the only baseline there is for a
new capability."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, mcubes, normals, ops, topology  # noqa: E402
import normals_spec as N  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402


BATCH = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--points', type=int, default=250000)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
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
    print('sphere R={}: {} faces, {} vertices, {} incidence entries, faces per vertex max {} mean {:.2f}'.format(
        R, nf, nv, ni, int(deg.max().item()), ni / nv))
    rng = np.random.default_rng(0)
    p = rng.standard_normal((args.points, 3))
    cloud = torch.from_numpy((0.35 * p / np.linalg.norm(p, axis=1)[:, None] * (1.0 + 0.01 * rng.standard_normal(args.points))[:, None])
                             .astype(np.float32)).to(dev)
    out = torch.empty(nv, 3, dtype=torch.float32, device=dev)

    def kernel(weight):                               # BATCH launches between two events: one launch alone is too short to time
        def run():
            for _ in range(BATCH):
                _lib.call('ppsx_normals_vertex', verts, nv, faces, nf, offsets, inc, ni, weight, out)
        return run

    blocks = ops.KnnBlocks(verts)
    idx, d2 = blocks.query(cloud, args.k, return_d2=True)
    nrm = normals.vertex_normals(verts, faces, 'area')[0]
    rows = [('incidence (ppsx_normals_corner_keys + sort + bincount + cumsum), wall', wall_ms(lambda: topology.vertex_incidence(faces, nv), args.reps))]
    for name, code in normals.WEIGHTS.items():
        rows.append(('{} launches of ppsx_normals_vertex, weight {}, device events'.format(BATCH, name), device_ms(kernel(code), args.reps)))
    for name in normals.WEIGHTS:
        rows.append(('vertex_normals(weight={}) end to end, wall'.format(name), wall_ms(lambda: normals.vertex_normals(verts, faces, name), args.reps)))
    rows += [('block structure of the vertices (ops.KnnBlocks), wall', wall_ms(lambda: ops.KnnBlocks(verts), args.reps)),
             ('search of {} points at k={} (KnnBlocks.query), device events'.format(args.points, args.k),
              device_ms(lambda: blocks.query(cloud, args.k, return_d2=True), args.reps)),
             ('{} launches of ppsx_normals_blend, device events'.format(BATCH),
              device_ms(lambda: [normals.blend_normals(idx, d2, nrm) for _ in range(BATCH)], args.reps)),
             ('point_normals({} points, k={}) end to end, wall'.format(args.points, args.k),
              wall_ms(lambda: normals.point_normals(cloud, verts, faces, k=args.k), args.reps))]
    print('GPU ({} reps after warm-up):'.format(args.reps))
    for name, (med, lo_) in rows:
        print('  {:<92s} median {:10.3f} ms  min {:10.3f} ms'.format(name, med, lo_))
    # bytes one vertex launch asks for: position, two offsets' worth and the result per vertex; a face index, the face and two corners per entry
    moved = nv * (12 + 8 + 12) + ni * (4 + 24 + 24)
    for row in rows[1:3]:
        per = row[1][0] / BATCH
        print('  one launch ({}): {:.4f} ms; it asks for {:.1f} MB -> {:.0f} GB/s (the mesh stays in the caches between launches)'.format(
            row[0].split('weight ')[1].split(',')[0], per, moved / 1e6, moved / per / 1e6))
    per = rows[7][1][0] / BATCH
    moved_b = args.points * (args.k * (8 + 4 + 12) + 12)
    print('  one blend: {:.4f} ms; it asks for {:.1f} MB -> {:.0f} GB/s'.format(per, moved_b / 1e6, moved_b / per / 1e6))
    got = {name: normals.vertex_normals(verts, faces, name) for name in normals.WEIGHTS}
    for name in normals.WEIGHTS:
        print('  vertex_normals {}: {}'.format(name, got[name][1]))
    pn, pinfo = normals.point_normals(cloud, verts, faces, k=args.k)
    radial = cloud / cloud.norm(dim=1, keepdim=True)
    print('  point_normals: {}; mean n . radial {:.6f}'.format(pinfo, float((pn * radial).sum(dim=1).mean().item())))
    if args.no_cpu:
        return
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    for name in normals.WEIGHTS:
        t0 = time.perf_counter()
        want = N.vertex_normals(hv, hf, name)
        dt = (time.perf_counter() - t0) * 1e3
        print('  {:<92s} {:10.1f} ms'.format('vertex_normals(weight={}) on the same mesh'.format(name), dt))
        assert got[name][0].cpu().numpy().tobytes() == want.tobytes(), 'the device differs from the specification ({})'.format(name)
        if name == 'area':
            t0 = time.perf_counter()
            bwant = N.blend(idx.cpu().numpy(), d2.cpu().numpy(), want)
            dt = (time.perf_counter() - t0) * 1e3
            print('  {:<92s} {:10.1f} ms'.format('blend of the device\'s neighbours ({} x {})'.format(args.points, args.k), dt))
            assert pn.cpu().numpy().tobytes() == bwant.tobytes(), 'the device blend differs from the specification'
    print('  the device equals the specification on all {} vertices (both weights) and all {} points'.format(nv, args.points))


if __name__ == '__main__':
    main()
