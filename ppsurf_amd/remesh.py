"""Isotropic remeshing of a mesh on the GPU: short-edge collapse, tangential relaxation and the loop that chains them with `subdivide` and
`flip` (csrc/pps_remesh.hip).

    python -m ppsurf_amd.remesh MESH OUT.ply (--target_edge L | --factor F) [--iters 5] [--relax_lam 0.5] [--flip_angle 10]
                                             [--max_faces N] [--stage remesh|collapse|relax]

Marching Cubes writes needles: short edges that no flip removes and no split shortens, and every per-vertex and per-face stage (`normals`,
`denoise`, `smooth`, `transfer`, `trim`) reads that triangulation.  `decimate` collapses by quadric error, `flip` turns diagonals, `subdivide`
splits long edges and `smooth` relaxes vertices; this module adds the two operators that were missing and the loop of Botsch and Kobbelt
(2004) around the four: with L the target edge, every iteration splits the edges longer than 4/3 L, collapses the edges shorter than 4/5 L
to their midpoint unless that would make an edge longer than 4/3 L or fold a face, flips towards Delaunay, and moves every vertex towards
the mean of its neighbours within its tangent plane.  The result has edges near one length and no needles.  Only regular vertices -- a
closed fan of faces, every edge of it shared by exactly two faces -- are collapsed or moved: borders and non-manifold regions come back byte
for byte from those two operators, as from every other stage.  Delaunay flips stand in for the valence flips of the paper, and nothing is
projected back onto the input surface: the relaxation keeps a vertex in its tangent plane, which on a curved surface is not the surface.
The result is a pure function of the ordered mesh and the parameters.  The models have no switch for this stage: run the command on the PLY
that `pps.py rec` wrote.  No default here is tuned on network output.
"""
import json
import math
import sys

import numpy as np
import torch

from . import _lib, decimate, flip, mesh_cli, meshio, params, subdivide, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT
MAX_ITERS = 1000
NONE = -1                                  # 2^64 - 1, the first word of the priority of an entry that is no candidate, as an int64
STAGES = ('remesh', 'collapse', 'relax')


def _checked_collapse(min_edge, max_edge, max_rounds):
    """(min_edge float, max_edge float or None, max_rounds int) or a ValueError: min_edge a finite number > 0, max_edge None or a finite
    number >= min_edge, max_rounds an integer in 1..2^31 - 1, no bools."""
    least = params.number('min_edge', min_edge, lambda x: x > 0, 'a finite number > 0')
    if max_edge is not None:
        max_edge = params.number('max_edge', max_edge, lambda x: x >= least, 'None or a finite number >= min_edge = {!r}'.format(min_edge))
    return least, max_edge, params.integer('max_rounds', max_rounds, 1, MAX_COUNT, '1..2^31 - 1')


def _checked_relax(iters, lam, name='lam'):
    """(iters int, lam float) or a ValueError: iters an integer in 0..1000, lam a finite number in (0, 1], no bools."""
    return params.integer('iters', iters, 0, MAX_ITERS), params.number(name, lam, lambda x: 0.0 < x <= 1.0, 'a finite number in (0, 1]')


def _checked_remesh(target_edge, factor, iters, relax_lam, flip_angle, max_faces):
    """The six parameters of the loop in their types, or a ValueError: exactly one of target_edge and factor, a finite number > 0; iters an
    integer in 0..1000; relax_lam finite in (0, 1]; flip_angle and max_faces by the rules of flip.py and subdivide.py; no bools."""
    if (target_edge is None) == (factor is None):
        raise ValueError('exactly one of target_edge and factor must be given, got {!r} and {!r}'.format(target_edge, factor))
    target_edge, factor = (None if value is None else params.number(name, value, lambda x: x > 0, 'a finite number > 0')
                           for name, value in (('target_edge', target_edge), ('factor', factor)))
    iters, relax_lam = _checked_relax(iters, relax_lam, 'relax_lam')
    return target_edge, factor, iters, relax_lam, flip._checked_angle(flip_angle), subdivide._checked_max_faces(max_faces)


def _short_edges(P, F, rows, min2, max2):
    """prio int64 [ne,3] holding u64 bits: the candidates of a collapse round."""
    nv, nf, ne = int(P.shape[0]), int(F.shape[0]), int(rows['nbr'].shape[0])
    prio = torch.empty(ne, 3, dtype=torch.int64, device=F.device)
    _lib.call('ppsx_remesh_short_edges', P, nv, F, nf, rows['offsets'], rows['nbr'], rows['src'], ne, rows['inc_offsets'], rows['inc'],
              int(rows['inc'].shape[0]), rows['regular'], min2, max2, prio)
    return prio


def _collapsed(v, f, min_edge, max_edge, max_rounds, timer=None):
    """(kept vertex rows int64 ascending, their positions f32, re-indexed faces, info) of a checked device mesh and checked parameters.  The
    rows are None when nothing collapsed and the mesh comes back as given.  timer(name) is called before every part of a round -- rows,
    kernels (with the host read), apply -- and before the output (tools/time_remesh.py)."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    tick = timer or (lambda name: None)
    F = f[topology.valid_faces(f, nv)].contiguous()
    info = {'faces_in': nf, 'faces_valid': int(F.shape[0]), 'faces_out': nf, 'vertices_in': nv, 'vertices_out': nv, 'rounds': 0, 'collapses': 0,
            'candidates': 0, 'locked_vertices': 0, 'converged': True, 'min_edge': min_edge, 'max_edge': max_edge, 'max_rounds': max_rounds}
    if F.shape[0] == 0:
        return None, None, f, info
    min2, max2 = min_edge * min_edge, (math.inf if max_edge is None else max_edge * max_edge)
    P, first = v.double(), True
    while True:
        tick('rows')
        rows = decimate._rows(F, nv)
        tick('kernels')
        prio = _short_edges(P, F, rows, min2, max2)
        flag = decimate._winners(rows, prio, nv)
        candidates = int((prio[:, 0] != NONE).sum().item())
        if first:
            info.update(candidates=candidates, locked_vertices=nv - int(rows['regular'].sum().item()))
            first = False
        if candidates == 0 or info['rounds'] == max_rounds:
            info['converged'] = candidates == 0
            break
        win = torch.nonzero(flag).reshape(-1)
        if win.shape[0] == 0:
            raise _lib.PpsError('collapse_short_edges: {} candidates and no winner; the shortest edge always wins'.format(candidates))
        tick('apply')
        F = decimate._apply(P, F, rows, torch.zeros(int(prio.shape[0]), 3, dtype=torch.float64, device=f.device), win)
        info['rounds'] += 1
        info['collapses'] += int(win.shape[0])
    tick('output')
    if info['collapses'] == 0:
        return None, None, f, info
    kept, out_v, out_f = decimate._compacted(P, F, nv)
    info.update(faces_out=int(F.shape[0]), vertices_out=int(kept.shape[0]))
    return kept, out_v, out_f, info


def collapse_short_edges(verts: torch.Tensor, faces: torch.Tensor, min_edge, max_edge=None, max_rounds=1000):
    """(verts, faces, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] with every edge shorter than min_edge collapsed to its
    midpoint, the shortest first, in rounds of independent collapses (the rounds are those of section 22 with another
    candidate rule).  An edge is a candidate when both ends are regular, it passes the link rule, its squared length is strictly below
    min_edge squared (an edge of length 0 qualifies), no face that holds one of its ends turns over with that end at the midpoint, and --
    with max_edge given -- no neighbour of its ends is farther than max_edge from the midpoint (Botsch and Kobbelt's guard: a collapse must
    not make an edge that the next split would cut).  The fold rule asks for a positive (n . n'), so a face without area at an end of the
    edge blocks the collapse: only the two faces on the edge itself may be needles.  Borders and non-manifold regions come back byte for
    byte; a closed manifold stays closed and manifold with its Euler characteristic.  All winners of a round collapse; the rounds stop
    when an evaluation finds no candidate (info['converged']) or after max_rounds.  Invalid faces are dropped, the vertices no face uses
    are dropped with the order of the rest kept, the faces are re-indexed and keep their order; a vertex that never moved comes back byte
    for byte.  When nothing collapsed the same tensors come back.  A pure function of the ordered mesh and the parameters.  info: faces_in,
    faces_valid, faces_out, vertices_in, vertices_out, rounds, collapses, candidates (of the first evaluation), locked_vertices (not
    regular at the start), converged, min_edge, max_edge, max_rounds.  ValueError: min_edge no finite number > 0, max_edge neither None nor
    a finite number >= min_edge, max_rounds no integer in 1..2^31 - 1, a bool for any of them, non-finite vertices, more than 2^31 - 1
    vertices or faces, CPU tensors (CpuTensorError)."""
    min_edge, max_edge, max_rounds = _checked_collapse(min_edge, max_edge, max_rounds)
    topology.need_device('collapse_short_edges', verts, faces)
    v, f = topology.checked_mesh('collapse_short_edges', verts, faces, limit=True)
    kept, out_v, out_f, info = _collapsed(v, f, min_edge, max_edge, max_rounds)
    if kept is None:
        return verts, faces, info
    return out_v, out_f, info


def _relaxed(v, f, iters, lam, timer=None):
    """(positions f32 or None when no pass ran, info) of a checked device mesh and checked parameters."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    tick = timer or (lambda name: None)
    info = {'vertices': nv, 'regular': 0, 'moved': 0, 'states': [0, 0, 0, 0], 'iters': iters, 'lam': lam}
    if nv == 0 or nf == 0:
        return None, info
    tick('rows')
    rows = decimate._rows(f, nv)
    info['regular'] = int(rows['regular'].sum().item())
    if iters == 0:
        return None, info
    tick('kernels')
    x, y = v.double(), torch.empty(nv, 3, dtype=torch.float64, device=v.device)
    state = torch.empty(nv, dtype=torch.uint8, device=v.device)
    for _ in range(iters):
        _lib.call('ppsx_remesh_relax_pass', x, nv, f, nf, rows['offsets'], rows['nbr'], int(rows['nbr'].shape[0]), rows['inc_offsets'], rows['inc'],
                  int(rows['inc'].shape[0]), rows['regular'], lam, y, state)
        x, y = y, x
    tick('output')
    out = x.float()
    info['moved'] = int((out.view(torch.int32) != v.view(torch.int32)).any(dim=1).sum().item())
    info['states'] = torch.bincount(state.long(), minlength=4).tolist()
    return out, info


def relax_tangential(verts: torch.Tensor, faces: torch.Tensor, iters=1, lam=0.5):
    """(verts f32 [nv,3], faces, info): `iters` Jacobi passes of tangential relaxation over the device mesh verts f32 [nv,3] / faces int64
    [nf,3].  A regular vertex moves by lam times the part of its Laplacian step (the mean of its neighbours minus
    itself) that lies in its tangent plane, the plane across the sum of the cross products of its faces; nothing takes a square root.  Only
    regular vertices move: borders and non-manifold fans are copied bit for bit (state 0).  A vertex also stays where that normal has no
    length or the step is not finite (state 2), and where one of its faces, with the vertex at its new place and the other corners at
    their old ones, would turn over or has no area (state 3); state 1 is a vertex that moved.  The neighbours move in the same pass, so
    that guard is a filter and no proof that no face folds: check the result with `intersect` where it matters.  The state is fp64 from
    the widened input to one rounding after the last pass; the faces are returned as given.  info: vertices, regular, moved (rows whose
    bytes changed), states (how many vertices the last pass left in state 0, 1, 2, 3; zeros when no pass ran), iters, lam.  ValueError:
    iters no integer in 0..1000, lam no finite number in (0, 1], a bool for either, non-finite vertices, more than 2^31 - 1 vertices or
    faces, CPU tensors (CpuTensorError)."""
    iters, lam = _checked_relax(iters, lam)
    topology.need_device('relax_tangential', verts, faces)
    v, f = topology.checked_mesh('relax_tangential', verts, faces, limit=True)
    out, info = _relaxed(v, f, iters, lam)
    return (verts if out is None else out), faces, info


def _remeshed(v, f, target_edge, factor, iters, relax_lam, flip_angle, max_faces, colors=None, timer=None):
    """(origin int64 [nv out] on the host, verts f32, faces, colors, info) of a checked device mesh and checked parameters: origin is the
    given row of every output vertex, -1 for one that a split made; colors (a host array or None) are carried along -- a split gives the
    rounded mean of its ends, a collapse keeps the surviving end's.  The meshes between the four steps are float32, as if the public
    functions were chained by hand."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    tick = timer or (lambda name: None)
    tick('median')
    target = target_edge if factor is None else factor * (subdivide.median_edge(v, f) if nf else 0.0)
    low, high = (4.0 * target) / 5.0, (4.0 * target) / 3.0
    info = {'target_edge': target, 'low': low, 'high': high, 'faces_in': nf, 'faces_out': nf, 'vertices_in': nv, 'vertices_out': nv, 'iters': iters,
            'relax_lam': relax_lam, 'flip_angle': flip_angle, 'max_faces': max_faces, 'iterations': [], 'limited': False}
    origin = np.arange(nv, dtype=np.int64)
    valid = nf > 0 and bool(topology.valid_faces(f, nv).any().item())
    if not valid or not target > 0.0:
        return origin, v, f, colors, info
    V, F = v, f
    for _ in range(iters):
        tick('split')
        out_v, out_f, ends, split = subdivide._subdivided(V, F, high, None, 100, max_faces)
        if out_v is not None:
            V, F = out_v, out_f
            origin = np.concatenate([origin, np.full(split['splits'], -1, dtype=np.int64)])
            if colors is not None:
                colors = subdivide.midpoint_colors(colors, ends.cpu().numpy(), split['added'])
        tick('collapse')
        kept, out_v, out_f, collapse = _collapsed(V, F, low, high, 1000)
        if kept is not None:
            V, F = out_v, out_f
            rows = kept.cpu().numpy()
            origin = origin[rows]
            if colors is not None:
                colors = np.asarray(colors)[rows]
        tick('flip')
        out_f, flips = flip._flipped(V, F, flip_angle, 1e-6, 100)
        if out_f is not None:
            F = out_f
        tick('relax')
        out_v, relax = _relaxed(V, F, 1, relax_lam)
        if out_v is not None:
            V = out_v
        info['iterations'].append({'splits': split['splits'], 'collapses': collapse['collapses'], 'flips': flips['flips'], 'moved': relax['moved']})
        info['limited'] = info['limited'] or bool(split['limited'])
    info.update(faces_out=int(F.shape[0]), vertices_out=int(V.shape[0]))
    return origin, V, F, colors, info


def remesh_isotropic(verts: torch.Tensor, faces: torch.Tensor, target_edge=None, factor=None, iters=5, relax_lam=0.5, flip_angle=10.0,
                     max_faces=None):
    """(verts f32, faces int64, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] remeshed towards one edge length (Botsch and
    Kobbelt 2004).  Exactly one of target_edge (a length in the mesh's units) and factor (a multiple of the median
    edge of the input, `subdivide`'s median) is given; with L the target, low = 4/5 L and high = 4/3 L, every one of the `iters`
    iterations is by definition
        split_long_edges(max_edge=high, max_faces=max_faces), collapse_short_edges(low, high), flip_edges(max_angle=flip_angle),
        relax_tangential(1, relax_lam)
    with float32 meshes between them, and the result equals that chain written by hand, byte for byte.  Delaunay flips stand in for the
    paper's valence flips; nothing is projected back onto the input surface.  What each step leaves alone stays: collapse and relaxation
    touch only regular vertices, flips only two-owner edges within flip_angle of flat, and splits cut borders too.  A mesh without a valid
    face, or whose target is not above 0, comes back as given.  None of the defaults is tuned on network output.  info: target_edge, low,
    high, faces_in, faces_out, vertices_in, vertices_out, iters, relax_lam, flip_angle, max_faces, iterations (per iteration: splits,
    collapses, flips, moved), limited (a split stopped at max_faces).  ValueError: both or neither of target_edge and factor, one that is no
    finite number > 0, iters no integer in 0..1000, relax_lam no finite number in (0, 1], flip_angle not in (0, 90], max_faces no integer
    in 0..(2^32 - 1) // 3, a bool for any of them, non-finite vertices, more than 2^31 - 1 vertices or faces, CPU tensors
    (CpuTensorError)."""
    params = _checked_remesh(target_edge, factor, iters, relax_lam, flip_angle, max_faces)
    topology.need_device('remesh_isotropic', verts, faces)
    v, f = topology.checked_mesh('remesh_isotropic', verts, faces, limit=True)
    _, out_v, out_f, _, info = _remeshed(v, f, *params)
    if out_v is v and out_f is f:
        return verts, faces, info
    return out_v, out_f, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.remesh',
                                 description='Remesh towards one edge length: split long edges, collapse short ones, flip, relax within the '
                                             'tangent plane (GPU).  Borders and non-manifold regions are neither collapsed nor moved.')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='remeshed PLY mesh; a collapse keeps the colour of the surviving end, a split gives the mean of its ends')
    bound = ap.add_mutually_exclusive_group(required=True)
    bound.add_argument('--target_edge', type=float, help='the edge length to aim for, in file units, > 0')
    bound.add_argument('--factor', type=float, help='the edge length to aim for as a multiple of the median edge of the mesh, > 0')
    ap.add_argument('--iters', type=int, default=5, help='iterations of the loop; with --stage relax the passes (0..1000)')
    ap.add_argument('--relax_lam', type=float, default=0.5, help='the step of the relaxation in (0, 1] (not tuned on network output)')
    ap.add_argument('--flip_angle', type=float, default=10.0, help='flip only where the two faces lie within this many degrees of one plane')
    ap.add_argument('--max_faces', type=int, default=None, help='a split stops before the round that would take the mesh above this many faces')
    ap.add_argument('--stage', choices=STAGES, default='remesh',
                    help='remesh: the loop; collapse: the short-edge collapse alone, below 4/5 of the target and without an upper bound; '
                         'relax: --iters passes of the relaxation alone')
    args = ap.parse_args(argv)
    try:
        target_edge, factor, iters, relax_lam, flip_angle, max_faces = _checked_remesh(args.target_edge, args.factor, args.iters, args.relax_lam,
                                                                                      args.flip_angle, args.max_faces)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.remesh')
    v, f = mesh.to_device(limit='faces')
    if args.stage == 'relax':
        out_v, info = _relaxed(v, f, iters, relax_lam)
        origin, out_f, colors = np.arange(int(v.shape[0]), dtype=np.int64), f, mesh.colors
        out_v = v if out_v is None else out_v
    elif args.stage == 'collapse':
        target = target_edge if factor is None else factor * (subdivide.median_edge(v, f) if int(f.shape[0]) else 0.0)
        if not target > 0.0:
            raise SystemExit('{} has no edge to take a target from'.format(args.mesh))
        kept, out_v, out_f, info = _collapsed(v, f, (4.0 * target) / 5.0, None, 1000)
        if kept is None:
            origin, out_v, out_f, colors = np.arange(int(v.shape[0]), dtype=np.int64), v, f, mesh.colors
        else:
            origin = kept.cpu().numpy()
            colors = None if mesh.colors is None else np.asarray(mesh.colors)[origin]
    else:
        origin, out_v, out_f, colors, info = _remeshed(v, f, target_edge, factor, iters, relax_lam, flip_angle, max_faces, colors=mesh.colors)
    mesh.write_origin(args.out_file, origin, out_v, out_f, colors)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
