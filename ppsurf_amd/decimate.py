"""Edge-collapse decimation of a mesh on the GPU: quadric error metric, rounds of independent collapses (csrc/pps_decimate.hip; DESIGN.md
section 22).

    python -m ppsurf_amd.decimate MESH OUT.ply --max_faces N [--max_rounds R]

`simplify` clusters vertices on a grid: fast, but at coarse grids it flips faces and makes non-manifold edges.  This stage takes a mesh down
to a face budget by collapsing edges (Garland and Heckbert): a closed manifold stays closed and manifold, a flat region stays exactly flat,
and a collapse that would fold the surface is refused.  Per round every edge between two regular vertices that passes the link rule gets
a position (the quadric of the faces around it, pulled to its midpoint), a cost and a priority; an edge that holds the smallest priority
in the neighbourhood of both its ends wins, and the winners, which share no end and no neighbour of an end, collapse at once.  Borders and
non-manifold regions are never touched: their vertices come back byte for byte.  The result is a pure function of the ordered mesh,
max_faces and max_rounds.  The models have no switch for this stage: run the command on the PLY that `pps.py rec` wrote.
"""
import json
import sys

import numpy as np
import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT
MIN_FACES = 4                              # a tetrahedron: no closed surface has fewer
SIGN = -2 ** 63                            # x ^ SIGN orders the bits of a u64 kept in an int64 as the u64 orders


def _checked_params(max_faces, max_rounds):
    """(max_faces, max_rounds) as ints or a ValueError: max_faces an integer in 4..2^31 - 1, max_rounds in 1..2^31 - 1, no bools."""
    return (params.integer('max_faces', max_faces, MIN_FACES, MAX_COUNT, '{}..2^31 - 1'.format(MIN_FACES)),
            params.integer('max_rounds', max_rounds, 1, MAX_COUNT, '1..2^31 - 1'))


def _rows(F, nv):
    """The rows of a round of the contiguous device faces F: adjacency (offsets, nbr, mult, src), incidence (inc_offsets, inc) and the
    regular vertices u8 [nv]."""
    offsets, nbr, mult, _ = topology.adjacency_rows(F, nv)
    inc_offsets, inc, _ = topology.incidence_rows(F, nv)
    ne = int(nbr.shape[0])
    src = torch.repeat_interleave(torch.arange(nv, dtype=torch.int32, device=F.device), offsets[1:] - offsets[:-1], output_size=ne)
    regular = torch.empty(nv, dtype=torch.uint8, device=F.device)
    _lib.call('ppsx_decimate_regular', offsets, mult, ne, inc_offsets, int(inc.shape[0]), nv, regular)
    return {'offsets': offsets, 'nbr': nbr, 'mult': mult, 'src': src, 'inc_offsets': inc_offsets, 'inc': inc, 'regular': regular}


def _winners(rows, prio, nv):
    """flag u8 [ne] of the priorities prio of a round: the vertex minimum, the ring minimum and the winners (remesh.py takes its rounds
    through here too)."""
    ne, dev = int(rows['nbr'].shape[0]), prio.device
    flag = torch.empty(ne, dtype=torch.uint8, device=dev)
    m1, best = torch.empty(nv, 3, dtype=torch.int64, device=dev), torch.empty(nv, 3, dtype=torch.int64, device=dev)
    _lib.call('ppsx_decimate_vertex_min', rows['offsets'], rows['nbr'], ne, nv, prio, m1)
    _lib.call('ppsx_decimate_ring_min', rows['offsets'], rows['nbr'], ne, nv, m1, best)
    _lib.call('ppsx_decimate_winners', rows['src'], rows['nbr'], ne, nv, prio, best, flag)
    return flag


def _candidates(P, F, rows):
    """(prio int64 [ne,3] holding u64 bits, x f64 [ne,3], fell u8 [ne], flag u8 [ne]) of a round: the four kernels."""
    nv, nf, ne, dev = int(P.shape[0]), int(F.shape[0]), int(rows['nbr'].shape[0]), F.device
    prio, x = torch.empty(ne, 3, dtype=torch.int64, device=dev), torch.empty(ne, 3, dtype=torch.float64, device=dev)
    fell = torch.empty(ne, dtype=torch.uint8, device=dev)
    _lib.call('ppsx_decimate_edges', P, nv, F, nf, rows['offsets'], rows['nbr'], rows['src'], ne, rows['inc_offsets'], rows['inc'],
              int(rows['inc'].shape[0]), rows['regular'], prio, x, fell)
    return prio, x, fell, _winners(rows, prio, nv)


def _first(prio, win, need):
    """The `need` entries of win with the smallest priorities: three stable sorts, the least significant word first."""
    p = prio[win]
    order = torch.sort(p[:, 2], stable=True)[1]
    order = order[torch.sort((p[:, 1] ^ SIGN)[order], stable=True)[1]]
    order = order[torch.sort(p[:, 0][order], stable=True)[1]]
    return win[order[:need]]


def _apply(P, F, rows, x, win):
    """The collapses of the winners: P moves in place, the renamed faces that keep three corners come back in their order."""
    nv, nf, dev = int(P.shape[0]), int(F.shape[0]), F.device
    rename = torch.arange(nv, dtype=torch.int32, device=dev)
    _lib.call('ppsx_decimate_move', win, int(win.shape[0]), rows['src'], rows['nbr'], int(rows['nbr'].shape[0]), x, P, nv, rename)
    out, keep = torch.empty_like(F), torch.empty(nf, dtype=torch.uint8, device=dev)
    _lib.call('ppsx_decimate_rename', F, nf, nv, rename, out, keep)
    return out[keep.bool()]


def _compacted(P, F, nv):
    """(kept vertex rows int64 ascending, their positions f32, re-indexed faces) of the working mesh after the rounds: the vertices no face
    uses are dropped with the order of the rest kept (remesh.py ends its collapse here too)."""
    used, remap = topology.used_rows(F, nv)
    kept = torch.nonzero(used).reshape(-1)
    return kept, P[kept].float(), remap[F]


def _decimate_rows(v, f, max_faces, max_rounds, timer=None):
    """(kept vertex rows int64 ascending, their positions f32, re-indexed faces, info) of a checked device mesh and checked parameters.  The
    rows are None when the mesh comes back as given.  timer(name) is called before every part of a round (tools/time_decimate.py)."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    tick = timer or (lambda name: None)
    F = f[topology.valid_faces(f, nv)].contiguous()
    info = {'faces_in': nf, 'faces_valid': int(F.shape[0]), 'faces_out': nf, 'vertices_in': nv, 'vertices_out': nv, 'rounds': 0, 'collapses': 0,
            'fallbacks': 0, 'locked_vertices': 0, 'reached': int(F.shape[0]) <= max_faces, 'max_faces': max_faces, 'max_rounds': max_rounds}
    if F.shape[0] == 0:
        return None, None, f, info
    tick('rows')
    rows = _rows(F, nv)
    info['locked_vertices'] = nv - int(rows['regular'].sum().item())
    if F.shape[0] <= max_faces:
        return None, None, f, info
    P = v.double()
    fallbacks = torch.zeros((), dtype=torch.int64, device=f.device)
    while True:
        tick('kernels')
        prio, x, fell, flag = _candidates(P, F, rows)
        tick('select')
        win = torch.nonzero(flag).reshape(-1)
        need = (int(F.shape[0]) - max_faces + 1) // 2
        if win.shape[0] == 0:
            break
        if win.shape[0] > need:
            win = _first(prio, win, need)
        fallbacks += fell[win].sum()
        tick('apply')
        F = _apply(P, F, rows, x, win)
        info['rounds'] += 1
        info['collapses'] += int(win.shape[0])
        if F.shape[0] <= max_faces or info['rounds'] >= max_rounds:
            break
        tick('rows')
        rows = _rows(F, nv)
    tick('output')
    kept, out_v, out_f = _compacted(P, F, nv)
    info.update(faces_out=int(F.shape[0]), vertices_out=int(kept.shape[0]), fallbacks=int(fallbacks.item()), reached=int(F.shape[0]) <= max_faces)
    return kept, out_v, out_f, info


def decimate_mesh(verts: torch.Tensor, faces: torch.Tensor, max_faces, max_rounds=1000):
    """(verts, faces, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] taken down to at most max_faces faces by quadric edge
    collapses, in rounds of independent collapses.  Only an edge between two regular vertices -- each with a closed
    fan of faces, every edge of it shared by exactly two faces -- can collapse, so borders and non-manifold regions come back byte for byte;
    a closed manifold stays closed and manifold with its Euler characteristic; a collapse that would turn a face over is refused.  The
    rounds stop at the budget, when no edge can collapse any more, or after max_rounds; a face count above the budget at the end is a
    result, not an error: info['reached'] is False.  Invalid faces are dropped, the vertices no face uses are dropped with the order of the
    rest kept, the faces are re-indexed and keep their order; a vertex that never moved comes back byte for byte.  An empty mesh, a mesh
    without a valid face and a mesh within the budget come back as given.  A pure function of the ordered mesh, max_faces and max_rounds.
    info: faces_in, faces_valid, faces_out, vertices_in, vertices_out, rounds, collapses, fallbacks (collapses placed at the midpoint),
    locked_vertices (the vertices that are not regular at the start), reached, max_faces, max_rounds.  ValueError: max_faces no integer in
    4..2^31 - 1, max_rounds no integer in 1..2^31 - 1, a bool for either, non-finite vertices, more than 2^31 - 1 vertices or faces, CPU
    tensors (CpuTensorError)."""
    max_faces, max_rounds = _checked_params(max_faces, max_rounds)
    topology.need_device('decimate_mesh', verts, faces)
    v, f = topology.checked_mesh('decimate_mesh', verts, faces, limit=True)
    kept, out_v, out_f, info = _decimate_rows(v, f, max_faces, max_rounds)
    if kept is None:
        return verts, faces, info
    return out_v, out_f, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.decimate',
                                 description='Decimate a mesh to a face budget by quadric edge collapses; borders and non-manifold regions stay (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='decimated PLY mesh; a vertex keeps the colour of its row, a moved vertex that of the surviving end '
                                     '(the smaller index) of its edge')
    ap.add_argument('--max_faces', type=int, required=True, help='the face budget, at least 4')
    ap.add_argument('--max_rounds', type=int, default=1000, help='stop after this many rounds of collapses')
    args = ap.parse_args(argv)
    try:
        max_faces, max_rounds = _checked_params(args.max_faces, args.max_rounds)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.decimate')
    kept, out_v, out_f, info = _decimate_rows(*mesh.to_device(limit='faces'), max_faces, max_rounds)
    if kept is None:
        mesh.write_as_read(args.out_file)
    else:
        # a vertex that never moved is written as read; a moved one from its float32 position
        kept = kept.cpu().numpy()
        mesh.write_origin(args.out_file, kept, out_v, out_f, None if mesh.colors is None else np.asarray(mesh.colors)[kept])
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
