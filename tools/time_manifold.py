"""Rates of the manifold split (ppsurf_amd/manifold.py, csrc/pps_manifold.hip).
    python tools/time_manifold.py [--res 257] [--reps 10] [--merges 2000] [--no_cpu]
-> median ms (after one warm-up round) for the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` with `--merges`
vertex pairs and as many edge pairs merged by renaming: of two faces drawn at random (seeded) the first corner of the second is renamed
to the first corner of the first -- a pinched vertex with two fans -- and, for the edge pairs, the first two corners to the first two --
an edge with four owners.  `split_nonmanifold` end to end, and its parts: the edge runs and pairs of the topology layer (the key kernel,
one sort with indices, the runs of two), the labelling on those pairs (the rounds of hook and compress with one flag read each) with its
number of rounds, and the face kernel (device events around BATCH launches back to back); `pieces.face_components` on the same mesh for
scale, since it labels faces over the same pairs.  The numpy specification tests/manifold_spec.py runs once on this machine's CPU and is
checked against the device, byte for byte."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, manifold, mcubes, pieces, topology  # noqa: E402
import manifold_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402

BATCH = 20


def merged(faces, nv, merges, seed):
    """The faces with `merges` vertex pairs and `merges` edge pairs made one by renaming."""
    rng = np.random.default_rng(seed)
    pick = faces[rng.permutation(faces.shape[0])[:4 * merges]].reshape(2 * merges, 2, 3)
    rename = np.arange(nv, dtype=np.int64)
    rename[pick[:merges, 1, 0]] = pick[:merges, 0, 0]                  # vertex pairs
    rename[pick[merges:, 1, 0]] = pick[merges:, 0, 0]                  # edge pairs: both ends
    rename[pick[merges:, 1, 1]] = pick[merges:, 0, 1]
    return np.ascontiguousarray(rename[rename[faces]])                 # (twice: a target that was itself renamed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--merges', type=int, default=2000)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, faces = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    hv = verts.cpu().numpy()
    nv = hv.shape[0]
    hf = merged(faces.cpu().numpy(), nv, args.merges, 7)
    nf = hf.shape[0]
    v, f = verts, torch.from_numpy(hf).to(dev)
    out_v, out_f, info, source = manifold.split_nonmanifold(v, f, return_source=True)
    print('sphere R={}: {} faces, {} vertices, {} + {} merges: {}'.format(R, nf, nv, args.merges, args.merges, info))
    again = manifold.split_nonmanifold(out_v, out_f)
    assert again[0] is out_v and again[1] is out_f and again[2]['edges_nonmanifold_in'] == 0, 'the split is not idempotent'
    runs = topology.edge_runs(f, nv)
    fa, fb, ea, eb, valid = topology.pairs_of_runs(*runs)
    label, rounds = manifold._fans(f, nv, fa, fb, ea, eb, valid)
    newrow, _, _ = manifold._rows(f, nv, label)
    nv_out = info['vertices_out']
    out = torch.empty_like(f)
    _, _, comp_rounds = pieces._labels(f, nv)

    def batch():
        for _ in range(BATCH):
            _lib.call('ppsx_manifold_faces', f, nf, nv, label, newrow, nv_out, out)

    timed = [('split_nonmanifold end to end, wall', 1, wall_ms(lambda: manifold.split_nonmanifold(v, f), args.reps)),
             ('edge runs and pairs (ppsx_pieces_edge_keys, sort with indices, runs of two): {} pairs, wall'.format(int(fa.shape[0])), 1,
              wall_ms(lambda: topology.pairs_of_runs(*topology.edge_runs(f, nv)), args.reps)),
             ('corner labelling on given pairs: {} rounds of hook, compress and one flag read, wall'.format(rounds), 1,
              wall_ms(lambda: manifold._fans(f, nv, fa, fb, ea, eb, valid), args.reps)),
             ('row tables in torch (leaders, scatter_reduce amin, nonzero, bincount), wall', 1, wall_ms(lambda: manifold._rows(f, nv, label), args.reps)),
             ('ppsx_manifold_faces, device events', BATCH, device_ms(batch, args.reps)),
             ('pieces.face_components on the same mesh (pairs and {} rounds), wall'.format(comp_rounds), 1,
              wall_ms(lambda: pieces.face_components(f, nv), args.reps))]
    print('  GPU ({} reps after warm-up; device-event rows are one launch of {} back to back):'.format(args.reps, BATCH))
    for name, per, (med, lo_) in timed:
        print('    {:<100s} median {:10.4f} ms  min {:10.4f} ms'.format(name, med / per, lo_ / per))
    if args.no_cpu:
        return
    t0 = time.perf_counter()
    spec_v, spec_f, spec_info, parts = S.split_spec(hv, hf)
    dt = time.perf_counter() - t0
    assert out_v.cpu().numpy().tobytes() == spec_v.tobytes() and out_f.cpu().numpy().tobytes() == spec_f.tobytes() and info == spec_info \
        and source.cpu().numpy().tobytes() == parts['source'].tobytes() and label.cpu().numpy().tobytes() == parts['label'].tobytes(), \
        'the device differs from the specification'
    print('  CPU (numpy specification, one run, one thread): split_spec {:10.1f} s; the device equals it, byte for byte'.format(dt))


if __name__ == '__main__':
    main()
