"""Delaunay edge flips of a mesh on the GPU: sliver triangles are repaired by turning diagonals, in rounds of independent flips
(csrc/pps_flip.hip).

    python -m ppsurf_amd.flip MESH OUT.ply [--max_angle 10] [--min_gain 1e-6] [--max_rounds 100]

Marching Cubes writes needles and caps, `decimate` leaves whatever diagonals its collapses produce and `fill` closes a loop with a fan;
every other mesh stage keeps the connectivity it is given or removes part of it.  This stage improves the shape of the triangles and
nothing else: the vertices stay byte for byte, and so do the face count, the borders, the Euler characteristic and every non-manifold
region.  An edge that exactly two faces hold, and run in opposite ways, is turned into the other diagonal of its quad when the two angles
opposite it sum to more than 180 degrees (the sum of their cotangents is below -min_gain), the new diagonal is no edge yet, the two new
faces do not fold over and the two old faces are within max_angle of one plane.  On a flat region the fixed point is the Delaunay
triangulation of the vertices.  Per round every such edge gets a priority, the worst first; an edge that holds the smallest priority at all
four vertices of its quad wins, and the winners, which share no vertex, flip at once.  The result is a pure function of the ordered mesh
and the three parameters.  Faces that run a shared edge the same way are skipped: run `python -m ppsurf_amd.orient` first.  The models
have no switch for this stage: run the command on the PLY that `pps.py rec` wrote.  The defaults of max_angle and min_gain are not tuned on
network output.
"""
import json
import math
import sys

import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT
NONE = -1                                  # 2^64 - 1, the priority of a pair that is no candidate, as the int64 that holds its bits


def _finite(name, value):
    return params.number(name, value, lambda x: True, 'a finite number')


def _checked_angle(max_angle):
    """max_angle as a float, or a ValueError: a finite number in (0, 90], no bool (remesh.py checks its flip_angle here)."""
    angle = _finite('max_angle', max_angle)
    if not 0.0 < angle <= 90.0:
        raise ValueError('max_angle must lie in (0, 90], got {!r}'.format(max_angle))
    return angle


def _checked_params(max_angle, min_gain, max_rounds):
    """(max_angle, min_gain as floats, max_rounds as an int) or a ValueError: max_angle finite in (0, 90], min_gain finite and >= 0,
    max_rounds an integer in 1..2^31 - 1, no bools."""
    _finite('max_angle', max_angle)                                      # both types before either range, the order the errors have always had
    gain = _finite('min_gain', min_gain)
    max_angle = _checked_angle(max_angle)
    if gain < 0.0:
        raise ValueError('min_gain must be >= 0, got {!r}'.format(min_gain))
    return max_angle, gain, params.integer('max_rounds', max_rounds, 1, MAX_COUNT, '1..2^31 - 1')


def _evaluate(v, F, cos2, min_gain, tick):
    """(fa, fb int32 [np], quad int32 [np,4], flag u8 [np], candidates, winners, valid bool [nf]) of the working faces F: one edge sort with
    keys, owners and pairs, the two kernels and one host read."""
    nv, nf, dev = int(v.shape[0]), int(F.shape[0]), F.device
    tick('sort')
    order, first, owners, valid, keys = topology.edge_runs_keys(F, nv)
    fa, fb, ea, eb, _ = topology.pairs_of_runs(order, first, owners, valid)
    pairs = int(fa.shape[0])
    prio, quad = torch.empty(pairs, dtype=torch.int64, device=dev), torch.empty(pairs, 4, dtype=torch.int32, device=dev)
    flag = torch.empty(pairs, dtype=torch.uint8, device=dev)
    if pairs == 0:
        return fa, fb, quad, flag, 0, 0, valid
    tick('kernels')
    vmin = torch.full((nv,), NONE, dtype=torch.int64, device=dev)
    _lib.call('ppsx_flip_candidates', v, nv, F, nf, fa, fb, ea, eb, pairs, keys, int(keys.shape[0]), cos2, min_gain, prio, quad, vmin)
    _lib.call('ppsx_flip_winners', prio, quad, pairs, vmin, nv, flag)
    candidates, winners = torch.stack([(prio != NONE).sum(), flag.sum()]).tolist()
    return fa, fb, quad, flag, candidates, winners, valid


def _flipped(v, f, max_angle, min_gain, max_rounds, timer=None):
    """(faces or None, info) of a checked device mesh and checked parameters; None when nothing flipped.  timer(name) is called before every
    part of a round -- sort, kernels (with the host read), apply -- and before the output (tools/time_flip.py)."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    tick = timer or (lambda name: None)
    cos2 = math.cos(math.radians(max_angle)) ** 2
    info = {'faces_in': nf, 'faces_valid': 0, 'edges_manifold': 0, 'candidates_in': 0, 'candidates_out': 0, 'flips': 0, 'rounds': 0,
            'converged': True, 'max_angle': max_angle, 'min_gain': min_gain, 'max_rounds': max_rounds}
    F, first = f, True
    while True:
        fa, fb, quad, flag, candidates, winners, valid = _evaluate(v, F, cos2, min_gain, tick)
        if first:
            info.update(faces_valid=int(valid.sum().item()), edges_manifold=int(fa.shape[0]), candidates_in=candidates)
            first = False
        if candidates == 0 or info['rounds'] == max_rounds:
            info.update(candidates_out=candidates, converged=candidates == 0)
            break
        if winners == 0:
            raise _lib.PpsError('flip_edges: {} candidates and no winner; the smallest priority always wins'.format(candidates))
        tick('apply')
        if F is f:
            F = f.clone()
        _lib.call('ppsx_flip_apply', fa, fb, quad, flag, int(fa.shape[0]), nv, F, nf)
        info['rounds'] += 1
        info['flips'] += winners
    tick('output')
    return (None if F is f else F), info


def flip_edges(verts: torch.Tensor, faces: torch.Tensor, max_angle=10.0, min_gain=1e-6, max_rounds=100):
    """(verts, faces, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] with its sliver triangles repaired by Delaunay edge
    flips, in rounds of independent flips.  Only an edge that exactly two valid faces hold and run in opposite ways
    can flip, so borders, many-owner edges and incoherent pairs come back byte for byte; the vertices are never written, the faces keep
    their count and their order, invalid faces come back as given, and no edge gains an owner.  max_angle (degrees, in (0, 90]): the two
    faces of a flipped edge lie within this angle of one plane; min_gain (>= 0): the sum of the cotangents of the two angles opposite the
    edge must be below -min_gain, a margin that keeps co-circular quads from flipping back and forth; neither default is tuned on network
    output.  The rounds stop when no edge is a candidate any more or after max_rounds rounds; that the loop ends before is proved only for
    flat regions, so info['converged'] reports it.  When nothing flipped the same tensors come back (the empty mesh and a mesh without a
    valid face are such cases).  A pure function of the ordered mesh and the three parameters.  info: faces_in, faces_valid, edges_manifold
    (the two-owner edges at the start), candidates_in, candidates_out (0 when converged, else the candidates that an evaluation after the
    last round finds), flips, rounds (those that flipped something), converged, max_angle, min_gain, max_rounds.  ValueError: max_angle no
    finite number in (0, 90], min_gain not finite or negative, max_rounds no integer in 1..2^31 - 1, a bool for any of them, non-finite
    vertices, more than 2^31 - 1 vertices or faces, CPU tensors (CpuTensorError)."""
    max_angle, min_gain, max_rounds = _checked_params(max_angle, min_gain, max_rounds)
    topology.need_device('flip_edges', verts, faces)
    v, f = topology.checked_mesh('flip_edges', verts, faces, limit=True)
    out, info = _flipped(v, f, max_angle, min_gain, max_rounds)
    return verts, faces if out is None else out, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.flip',
                                 description='Repair sliver triangles of a mesh by Delaunay edge flips; vertices, borders and non-manifold '
                                             'regions stay (GPU).  Faces that run a shared edge the same way are skipped: run '
                                             '`python -m ppsurf_amd.orient` first.')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='PLY mesh with the flipped faces; vertices and colours as read')
    ap.add_argument('--max_angle', type=float, default=10.0,
                    help='flip only where the two faces lie within this many degrees of one plane, in (0, 90] (not tuned on network output)')
    ap.add_argument('--min_gain', type=float, default=1e-6,
                    help='flip only where the sum of the two opposite cotangents is below -min_gain, >= 0 (not tuned on network output)')
    ap.add_argument('--max_rounds', type=int, default=100, help='stop after this many rounds of flips')
    args = ap.parse_args(argv)
    try:
        max_angle, min_gain, max_rounds = _checked_params(args.max_angle, args.min_gain, args.max_rounds)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.flip')
    out, info = _flipped(*mesh.to_device(limit='faces'), max_angle, min_gain, max_rounds)
    mesh.write_as_read(args.out_file, faces=out)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
