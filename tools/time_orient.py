"""Rates of the orientation stage (ppsurf_amd/orient.py, csrc/pps_orient.hip).
    python tools/time_orient.py [--res 257] [--reps 10] [--no_cpu]
-> median ms (after one warm-up round) for the welded Marching Cubes mesh of an analytic sphere (radius 0.35) at `--res` with a seeded random
half of its faces turned.  `orient_mesh(outward)` end to end, and its parts: the pairs with their edge slots (key kernel, sort, runs of two),
the labelling with a parity on that pair list (pair signs, the rounds of hook and compress with one flag read each, the check) with its
number of rounds, the volume (the stable sort by component, the block table, block sums and component sums) and the apply kernel (device
events around BATCH launches back to back).  Next to it on the same mesh: `pieces.face_components`, which makes the same pass without a
parity (pairs and labelling, and the labelling alone as the difference), and the numpy specification tests/orient_spec.py on this machine's
CPU (checked against the device, byte for byte)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from ppsurf_amd import _lib, mcubes, orient, pieces, topology  # noqa: E402
import orient_spec as S  # noqa: E402
from timing import device_ms, wall_ms  # noqa: E402

BATCH = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=257)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    R = args.res
    g = torch.linspace(-0.5, 0.5, R, dtype=torch.float64, device=dev)
    gx, gy, gz = torch.meshgrid(g, g, g, indexing='ij')
    verts, faces = mcubes.marching_cubes_torch((0.35 - torch.sqrt(gx * gx + gy * gy + gz * gz)).contiguous(), 0.0)
    verts, good = mcubes.clean_mesh_torch(verts.to(torch.float32).to(torch.float64), faces, min_component_faces=6, welded=True, grid_coords=True)
    verts = (verts * (1.0 / (R - 1)) - 0.5).float().contiguous()
    good = good.contiguous()
    nv, nf = int(verts.shape[0]), int(good.shape[0])
    mask = torch.from_numpy(np.random.default_rng(5).random(nf) < 0.5).to(dev)
    faces = torch.where(mask[:, None], good[:, [0, 2, 1]], good).contiguous()

    out_v, out_f, info = orient.orient_mesh(verts, faces, 'outward')
    fa, fb, ea, eb, valid = topology.manifold_pair_edges(faces, nv)
    label, flip, bad, _, _, rounds = orient._parity_labels(faces, fa, fb, ea, eb, valid)
    plain_rounds = pieces._labels(faces, nv)[2]
    print('sphere R={}: {} faces, {} vertices, {} pairs, {} turned at random; {} labelling rounds with a parity, {} without'.format(
        R, nf, nv, int(fa.shape[0]), int(mask.sum().item()), rounds, plain_rounds))
    print('  orient_mesh(outward): {}'.format(info))
    # which way the mesh came out of Marching Cubes is not this tool's business: the result is coherent and its volume positive
    same, mirrored = torch.equal(out_f, good), torch.equal(out_f, good[:, [0, 2, 1]])
    assert same or mirrored, 'the oriented mesh is neither the mesh as extracted nor its mirror image'
    print('  the result is the mesh as extracted{}'.format('' if same else ', every face turned (it was wound inward)'))
    nc = info['components']
    leader = torch.nonzero(label == torch.arange(nf, dtype=torch.int32, device=dev)).reshape(-1)
    cid = torch.searchsorted(leader, label.long()).to(torch.int32)
    faces_c = torch.bincount(cid.long(), minlength=nc)
    need = torch.ones(nc, dtype=torch.bool, device=dev)
    turn = torch.ones(nc, dtype=torch.uint8, device=dev)
    out = torch.empty_like(faces)

    def batch(fn):
        def run():
            for _ in range(BATCH):
                fn()
        return run

    pairs_ms = wall_ms(lambda: topology.manifold_pair_edges(faces, nv), args.reps)
    parity_ms = wall_ms(lambda: orient._parity_labels(faces, fa, fb, ea, eb, valid), args.reps)
    plain_ms = wall_ms(lambda: pieces._labels(faces, nv), args.reps)
    timed = [('orient_mesh(outward) end to end, wall', 1, wall_ms(lambda: orient.orient_mesh(verts, faces, 'outward'), args.reps)),
             ('pairs with slots (ppsx_pieces_edge_keys + sort with indices + runs of two), wall', 1, pairs_ms),
             ('labelling with a parity: signs, {} rounds of hook, compress and one flag read, check, wall'.format(rounds), 1, parity_ms),
             ('volume: stable sort by component, block table, block sums, component sums, wall', 1,
              wall_ms(lambda: orient._volumes(verts, faces, flip, cid, leader, need, faces_c), args.reps)),
             ('ppsx_orient_apply, device events', BATCH,
              device_ms(batch(lambda: _lib.call('ppsx_orient_apply', faces, nf, cid, flip, turn, nc, out)), args.reps)),
             ('for comparison: pieces.face_components (pairs + {} rounds without a parity), wall'.format(plain_rounds), 1, plain_ms),
             ('for comparison: its labelling alone (the row above minus the pairs)', 1, (plain_ms[0] - pairs_ms[0], plain_ms[1] - pairs_ms[1]))]
    print('GPU ({} reps after warm-up; device-event rows are one launch of {} back to back):'.format(args.reps, BATCH))
    for name, per, (med, lo_) in timed:
        print('  {:<100s} median {:10.4f} ms  min {:10.4f} ms'.format(name, med / per, lo_ / per))
    if args.no_cpu:
        return
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    t0 = time.perf_counter()
    _, want_f, want_info, _ = S.orient_spec(hv, hf, 'outward')
    dt = (time.perf_counter() - t0) * 1e3
    print('CPU (numpy specification, one run, {} threads visible):'.format(os.environ.get('OMP_NUM_THREADS', '?')))
    print('  {:<100s} {:10.1f} ms'.format('orient_spec(outward) on the same mesh', dt))
    assert out_v is verts and out_f.cpu().numpy().tobytes() == want_f.tobytes() and info == want_info, 'the device differs from the specification'
    print('  the device equals the specification on all {} faces'.format(want_f.shape[0]))


if __name__ == '__main__':
    main()
