"""Subdivision of a mesh on the GPU: every edge longer than a bound is split at its midpoint, the longest first, in rounds of independent
splits (csrc/pps_subdivide.hip).

    python -m ppsurf_amd.subdivide MESH OUT.ply (--max_edge L | --factor F) [--max_rounds 100] [--max_faces N]

Every other mesh stage keeps the connectivity it is given, removes part of it or re-arranges it; this one adds resolution.  A decimated
mesh, the fan of a filled hole or a welded CAD import has triangles that span the whole part, and the stages that work per vertex
(`transfer`, `normals`, `smooth`, `denoise`) see such a face only at its three corners.  An edge whose squared length exceeds
max_edge squared is a candidate; every face votes for the longest candidate among its three edges, and an edge that all its faces voted for is
split: one new vertex at the midpoint, and every face on the edge becomes two, wound like the parent.  That is Rivara's longest-edge
bisection with waiting instead of propagation: a face whose longest edge lost to a longer edge of a neighbour waits a round, no hanging
node ever exists, and no angle falls below half the smallest angle of the triangle it came from.  The given vertices stay byte for byte and
keep their rows; borders stay borders, many-owner edges keep their owner count, a closed manifold stays one.  The result is a pure function of
the ordered mesh and the parameters, and the new vertices do not depend on the order of the faces.  The face count grows like
(edge / max_edge) squared: --max_faces is the guard against a typo.  The models have no switch for this stage: run the command on the PLY
that `pps.py rec` wrote.
"""
import json
import math
import sys

import numpy as np
import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT
MAX_FACES = (2 ** 32 - 1) // 3             # 3 nf keys, and a rank is a 32-bit word
NONE = -1                                  # 2^64 - 1, the priority of an edge that is no candidate, as the int64 that holds its bits


def _checked_params(max_edge, factor, max_rounds, max_faces):
    """(max_edge or None, factor or None as floats, max_rounds, max_faces as ints) or a ValueError: exactly one of max_edge and factor, a
    finite number > 0; max_rounds an integer in 1..2^31 - 1; max_faces None (the largest count) or an integer in 0..(2^32 - 1) // 3; no bools."""
    if (max_edge is None) == (factor is None):
        raise ValueError('exactly one of max_edge and factor must be given, got {!r} and {!r}'.format(max_edge, factor))
    max_edge, factor = (None if value is None else params.number(name, value, lambda x: x > 0, 'a finite number > 0')
                        for name, value in (('max_edge', max_edge), ('factor', factor)))
    return max_edge, factor, params.integer('max_rounds', max_rounds, 1, MAX_COUNT, '1..2^31 - 1'), _checked_max_faces(max_faces)


def _checked_max_faces(max_faces):
    """max_faces as an int, or a ValueError: None (the largest count) or an integer in 0..(2^32 - 1) // 3, no bool (remesh.py checks its
    max_faces here)."""
    return MAX_FACES if max_faces is None else params.integer('max_faces', max_faces, 0, MAX_FACES)


def _runs(F, nv):
    """(keys int64 [ne], owners int64 [ne], run_of int64 [3 nf]) of the working faces F: one edge sort, and the run of every unsorted key
    position scattered through the sort's permutation."""
    order, first, owners, _, keys = topology.edge_runs_keys(F, nv)
    start = torch.zeros(order.shape[0], dtype=torch.int64, device=F.device)
    start[first[1:]] = 1
    run_of = torch.empty_like(order)
    run_of[order] = torch.cumsum(start, 0)
    return keys, owners, run_of


def _priorities(v, keys, max2):
    """(len2 f64 [ne], prio int64 [ne]) of the runs; max2 = +inf gives the lengths alone."""
    ne = int(keys.shape[0])
    len2, prio = torch.empty(ne, dtype=torch.float64, device=v.device), torch.empty(ne, dtype=torch.int64, device=v.device)
    _lib.call('ppsx_subdivide_edges', keys, ne, v, int(v.shape[0]), max2, len2, prio)
    return len2, prio


def median_edge(v, f, edges=None):
    """The square root of the lower median of the squared lengths of the distinct edges of the valid faces of a checked device mesh, 0.0
    without a valid face (remesh.py takes its target from here).  edges: (the number of valid faces, the keys of topology.edge_runs_keys)
    from a caller that has them already, so that no mesh is sorted twice."""
    if edges is None:
        _, _, _, valid, keys = topology.edge_runs_keys(f, int(v.shape[0]))
        edges = int(valid.sum().item()), keys
    faces_valid, keys = edges
    live = int(keys.shape[0]) - (1 if faces_valid < int(f.shape[0]) else 0)            # without the run of the invalid faces
    if faces_valid == 0 or live <= 0:
        return 0.0
    len2 = torch.sort(_priorities(v, keys, math.inf)[0][:live])[0]
    return math.sqrt(len2[(live - 1) // 2].item())


def _evaluate(v, F, max2, tick):
    """(keys, run_of, choice int32 [nf], win u8 [ne], hit u8 [nf], ne, candidates, winners, hits) of the working faces F: one edge sort, the
    four kernels and one host read."""
    nf, dev = int(F.shape[0]), F.device
    tick('sort')
    keys, owners, run_of = _runs(F, int(v.shape[0]))
    ne = int(keys.shape[0])
    tick('kernels')
    prio = _priorities(v, keys, max2)[1]
    choice, votes = torch.empty(nf, dtype=torch.int32, device=dev), torch.zeros(ne, dtype=torch.int32, device=dev)
    win, hit = torch.empty(ne, dtype=torch.uint8, device=dev), torch.empty(nf, dtype=torch.uint8, device=dev)
    _lib.call('ppsx_subdivide_votes', run_of, nf, prio, ne, choice, votes)
    _lib.call('ppsx_subdivide_winners', prio, votes, owners, ne, win)
    _lib.call('ppsx_subdivide_hits', run_of, choice, nf, win, ne, hit)
    candidates, winners, hits = torch.stack([(prio != NONE).sum(), win.sum(), hit.sum()]).tolist()
    return keys, run_of, choice, win, hit, ne, candidates, winners, hits


def _subdivided(v, f, max_edge, factor, max_rounds, max_faces, timer=None):
    """(verts, faces, ends -- or None three times when nothing split --, info) of a checked device mesh and checked parameters.  timer(name)
    is called before every part of a round -- sort, kernels (with the host read), emit -- and before the output (tools/time_subdivide.py)."""
    nv0, nf0, dev = int(v.shape[0]), int(f.shape[0]), f.device
    tick = timer or (lambda name: None)
    info = {'vertices_in': nv0, 'vertices_out': nv0, 'faces_in': nf0, 'faces_valid': 0, 'faces_out': nf0, 'edges_in': 0,
            'max_edge': 0.0 if max_edge is None else max_edge, 'candidates_in': 0, 'candidates_out': 0, 'splits': 0, 'rounds': 0, 'converged': True,
            'limited': False, 'max_rounds': max_rounds, 'max_faces': max_faces, 'added': []}
    if nf0 == 0:
        return None, None, None, info
    if nf0 > MAX_FACES:
        raise ValueError('split_long_edges: at most {} faces, got {}'.format(MAX_FACES, nf0))
    # a face that is invalid for the given vertex count is out of play for good: a row [nv, 1, 2] must not come alive with the first new vertex
    tick('sort')
    _, _, _, valid, keys = topology.edge_runs_keys(f, nv0)
    info['faces_valid'] = int(valid.sum().item())
    if info['faces_valid'] == 0:
        return None, None, None, info
    V, F = v, f if info['faces_valid'] == nf0 else torch.where(valid[:, None], f, torch.full_like(f, -1))
    if max_edge is None:
        tick('kernels')
        info['max_edge'] = factor * median_edge(v, f, (info['faces_valid'], keys))
    max2 = info['max_edge'] * info['max_edge']
    ends, first = [], True
    while True:
        keys, run_of, choice, win, hit, ne, candidates, winners, hits = _evaluate(V, F, max2, tick)
        nv, nf = int(V.shape[0]), int(F.shape[0])
        if first:
            info.update(edges_in=ne - (1 if info['faces_valid'] < nf0 else 0), candidates_in=candidates)
            first = False
        limited = candidates > 0 and info['rounds'] < max_rounds and (nf + hits > max_faces or nv + winners > MAX_COUNT)
        if candidates == 0 or info['rounds'] == max_rounds or limited:
            info.update(candidates_out=candidates, converged=candidates == 0, limited=limited)
            break
        if winners == 0 or hits == 0:
            raise _lib.PpsError('split_long_edges: {} candidates and no winner; the longest edge always wins'.format(candidates))
        tick('emit')
        vslot, fslot = torch.cumsum(win, 0, dtype=torch.int64) - win, torch.cumsum(hit, 0, dtype=torch.int64) - hit
        new_v, new_e = torch.zeros(winners, 3, dtype=torch.float32, device=dev), torch.full((winners, 2), -1, dtype=torch.int64, device=dev)
        out = torch.empty(nf + hits, 3, dtype=torch.int64, device=dev)
        out[nf:] = -1                                                                  # what a hit that emit refuses would leave: an invalid face
        _lib.call('ppsx_subdivide_emit', V, nv, keys, win, vslot, ne, winners, F, nf, run_of, choice, hit, fslot, hits, new_v, new_e, out)
        V, F = torch.cat([V, new_v]), out
        ends.append(new_e)
        info['rounds'] += 1
        info['splits'] += winners
        info['added'].append(winners)
    tick('output')
    info.update(vertices_out=int(V.shape[0]), faces_out=int(F.shape[0]))
    if info['splits'] == 0:
        return None, None, None, info
    if info['faces_valid'] < nf0:
        F[:nf0] = torch.where(valid[:, None], F[:nf0], f)
    return V, F, torch.cat(ends), info


def split_long_edges(verts: torch.Tensor, faces: torch.Tensor, max_edge=None, factor=None, max_rounds=100, max_faces=None, return_ends=False):
    """(verts f32 [nv + splits, 3], faces int64 [nf + new faces, 3], info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] with
    every edge longer than max_edge split at its midpoint, the longest first, in rounds of independent splits; with
    return_ends (verts, faces, ends, info), ends int64 [splits,2] the two ends a < b of every new vertex in row order -- an end may be an
    earlier new vertex -- which with info['added'], the splits per round, lets a caller interpolate any attribute round by round.  Exactly
    one of max_edge (a length in the mesh's units) and factor (max_edge = factor x the square root of the lower median of the squared
    lengths of the distinct edges) is given, a finite number > 0.  The given vertices keep their rows and bytes, the given faces their
    rows (a split face keeps one half there, the other is appended), a face that is invalid as given comes back as given and takes no part.
    Any edge can split, borders and many-owner edges too: every face on it is cut through the one new vertex.  The rounds stop when no edge
    is a candidate any more (info['converged']), after max_rounds rounds, or before a round that would take the faces above max_faces
    (default (2^32 - 1) // 3) or the vertices above 2^31 - 1 (info['limited']; nothing of that round is applied).  An edge whose midpoint
    rounds onto one of its ends is never a candidate.  When nothing was split the same tensors come back (the empty mesh and a mesh without a
    valid face are such cases).  A pure function of the ordered mesh and the parameters.  info: vertices_in, vertices_out, faces_in,
    faces_valid, faces_out, edges_in, max_edge (the float used), candidates_in, candidates_out, splits, rounds, converged, limited,
    max_rounds, max_faces, added.  ValueError: both or neither of max_edge and factor, one that is no finite number > 0, max_rounds no
    integer in 1..2^31 - 1, max_faces no integer in 0..(2^32 - 1) // 3, a bool for any of them, non-finite vertices, more than 2^31 - 1
    vertices or (2^32 - 1) // 3 faces, CPU tensors (CpuTensorError)."""
    max_edge, factor, max_rounds, max_faces = _checked_params(max_edge, factor, max_rounds, max_faces)
    topology.need_device('split_long_edges', verts, faces)
    v, f = topology.checked_mesh('split_long_edges', verts, faces, limit=True)
    out_v, out_f, ends, info = _subdivided(v, f, max_edge, factor, max_rounds, max_faces)
    if out_v is None:
        out_v, out_f, ends = verts, faces, torch.zeros(0, 2, dtype=torch.int64, device=f.device)
    return (out_v, out_f, ends, info) if return_ends else (out_v, out_f, info)


def midpoint_colors(colors, ends, added):
    """uint8 [nv + splits, c]: `colors` uint8 [nv, c] of the given vertices with the colour of every new vertex appended (host arrays): per
    channel (ca + cb + 1) >> 1 of its two ends in integers, round by round -- the ends of a round are all older than the round."""
    out = np.asarray(colors, dtype=np.uint8)
    ends, at = np.asarray(ends, dtype=np.int64).reshape(-1, 2), 0
    for count in added:
        a, b = ends[at:at + count, 0], ends[at:at + count, 1]
        out = np.concatenate([out, ((out[a].astype(np.int64) + out[b].astype(np.int64) + 1) >> 1).astype(np.uint8)])
        at += count
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.subdivide',
                                 description='Split every edge longer than a bound at its midpoint, the longest first (longest-edge bisection, '
                                             'GPU).  The given vertices and borders stay; new vertices take the mean colour of their ends.')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='subdivided PLY mesh')
    bound = ap.add_mutually_exclusive_group(required=True)
    bound.add_argument('--max_edge', type=float, help='the longest edge that is left, a length in file units > 0')
    bound.add_argument('--factor', type=float, help='the longest edge that is left as a multiple of the median edge length of the mesh, > 0')
    ap.add_argument('--max_rounds', type=int, default=100, help='stop after this many rounds of splits')
    ap.add_argument('--max_faces', type=int, default=None,
                    help='stop before the round that would take the mesh above this many faces: the face count grows like (edge / max_edge) '
                         'squared, so this is the guard against a typo in the bound (default {}, the most the stage can hold)'.format(MAX_FACES))
    args = ap.parse_args(argv)
    try:
        max_edge, factor, max_rounds, max_faces = _checked_params(args.max_edge, args.factor, args.max_rounds, args.max_faces)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.subdivide')
    nv, colors = int(mesh.verts.shape[0]), mesh.colors
    try:
        out_v, out_f, ends, info = _subdivided(*mesh.to_device(limit='faces'), max_edge, factor, max_rounds, max_faces)
    except ValueError as e:
        raise SystemExit('{}: {}'.format(args.mesh, e))
    if out_v is None:
        mesh.write_as_read(args.out_file)
    else:
        # the given vertices keep their rows and bytes, so they are written as read; only the new ones come back from the centred float32 frame
        if colors is not None:
            colors = midpoint_colors(colors, ends.cpu().numpy(), info['added'])
        origin = np.concatenate([np.arange(nv, dtype=np.int64), np.full(info['splits'], -1, dtype=np.int64)])
        mesh.write_origin(args.out_file, origin, out_v, out_f, colors)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
