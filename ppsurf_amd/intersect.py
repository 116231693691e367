"""Self-intersections of a mesh on the GPU: which pairs of faces cross, and the mesh without them (csrc/pps_intersect.hip; DESIGN.md
section 29).

    python -m ppsurf_amd.intersect MESH [OUT.ply] [--action remove|select] [--pairs_out P.npy] [--max_pairs N]

`decimate` and `flip` refuse a move that folds a face over, but only next to the move; `smooth`, `denoise`, `fill`, a coarse `simplify` and
`weld --eps` can push one part of a surface through another and no stage notices.  This one says whether the mesh still is a surface: it
flags every face that crosses another one, lists the crossing pairs, and can cut the offenders out so that `fill` can close the wound.
Only LIVE faces take part -- valid for the vertex count and with nine finite coordinates.  A pair is tested when the boxes of the two faces
overlap and they share at most one vertex INDEX; it crosses when an edge of one passes strictly through the plane of the other, inside
that triangle, in fp64 on the float32 input (with one shared vertex only the two edges opposite it are asked).  Faces that share an edge or
all three indices are never a pair: a fold onto a neighbour across the common edge is coplanar contact and out of scope.  Coincident but
unwelded vertices are not shared, so run `weld` first or every seam reports its neighbours.  NOT detected, by design: coplanar overlaps,
contacts where a vertex lies exactly in the other face's plane, zero-area faces -- these are contacts, not crossings.  The result is a pure
function of the ordered mesh: it does not depend on the cell edge, the table capacity, which faces go through the cell lists and which
through the list of large faces, the launch shape or the order in which candidates are met.  The models have no switch for this stage: run
the command on the PLY that `pps.py rec` or another stage wrote.
"""
import json
import math
import sys

import numpy as np
import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)
from .trim import SupportGrid, _f32_not_below

MAX_COUNT = topology.MAX_COUNT
MAX_PAIRS = 2 ** 24
QUANTILE = 0.99                            # of the sorted extents: the cell edge; see cell_edge
F32_MAX = float(np.finfo(np.float32).max)


def _checked_params(max_pairs):
    """max_pairs as an int, or a ValueError: an integer in 0..2^31 - 1, no bool."""
    return params.integer('max_pairs', max_pairs, 0, MAX_COUNT, '0..2^31 - 1')


def face_boxes(v, f):
    """(lo f32 [nf,3], hi f32 [nf,3], ext f32 [nf], live u8 [nf]) of ppsx_intersect_boxes on a checked device mesh."""
    nf, dev = int(f.shape[0]), f.device
    lo, hi = torch.empty(nf, 3, dtype=torch.float32, device=dev), torch.empty(nf, 3, dtype=torch.float32, device=dev)
    ext, live = torch.empty(nf, dtype=torch.float32, device=dev), torch.empty(nf, dtype=torch.uint8, device=dev)
    _lib.call('ppsx_intersect_boxes', v, int(v.shape[0]), f, nf, lo, hi, ext, live)
    return lo, hi, ext, live


def cell_edge(ext, live):
    """The extent above which a face is large, a float: with e the ascending extents of the live faces, q = e[ceil(0.99 (n - 1))], and the
    largest extent itself when that is at most 2 q.  The cost of a face is the anchors in the cells it opens, which grows like h^2 on a
    surface, plus one box test per large face, which every face pays: on a uniform mesh (Marching Cubes, a remeshed scan) the largest
    extent is within a factor two of the quantile and no face need be large; the few long faces of a decimated or filled mesh would
    otherwise set the cell edge for everyone, so they go to the list.  0.0 when no face is live."""
    e = torch.sort(ext[live != 0])[0]
    n = int(e.shape[0])
    if n == 0:
        return 0.0
    q, top = e[[int(math.ceil(QUANTILE * (n - 1))), n - 1]].tolist()
    return float(top) if top <= 2.0 * q else float(q)


class _Lists:
    """The broad phase of one mesh: the small live faces (ext <= large_above) with the cell lists of their box lower corners, cell edge
    h >= large_above and never below the anchors' longest box edge / (2^20 - 1), and the large live faces as a plain list.  When no finite
    cell edge serves (coordinates near the largest float) every live face is large: slow and correct."""

    def __init__(self, lo, ext, live, large_above, cell, capacity):
        alive = live != 0
        small = torch.nonzero(alive & (ext <= large_above))[:, 0].contiguous()
        self.grid, self.h = None, 0.0
        if small.shape[0] > 0:
            with np.errstate(over='ignore'):                       # a box wider than the largest float has the extent +inf
                grid = SupportGrid(lo[small].contiguous(), capacity)
            h = float(grid.edge_for(max(large_above, 0.0)) if cell is None else _f32_not_below(cell))
            if h == 0.0:
                h = 1.0                                            # every anchor at one point and every extent zero: any edge gives one cell
            if not h >= large_above:
                raise ValueError('the cell edge {} is below large_above {}'.format(h, large_above))
            if math.isfinite(float(grid.ext)) and h <= F32_MAX and 1.0 / h <= F32_MAX and float(grid.ext) / h <= float((1 << 20) - 1):
                self.grid, self.h = grid.build(h), h
            else:
                small = small[:0]
        self.small = small
        self.large = torch.nonzero(alive & (ext > large_above))[:, 0].contiguous() if small.shape[0] > 0 else torch.nonzero(alive)[:, 0].contiguous()

    def args(self):
        """(small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl): the arguments of the two walks between `live` and the
        outputs; without cell lists everything before `large` is NULL or zero."""
        g, nl = self.grid, int(self.large.shape[0])
        if g is None:
            return None, 0, None, None, 0.0, 0.0, None, 0, None, None, self.large, nl
        return self.small, int(self.small.shape[0]), g._vec3(g.lo), g._vec3(g.hi), float(g.h), float(g.inv_h), g._table, g.capacity, g.order, g.offsets, self.large, nl

    def count(self, v, f, lo, hi, live, flag, count, boxed):
        small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl = self.args()
        _lib.call('ppsx_intersect_count', v, int(v.shape[0]), f, int(f.shape[0]), lo, hi, live, small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets,
                  large, nl, flag, count, boxed)

    def emit(self, v, f, lo, hi, live, count, pair_offsets, pairs):
        small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl = self.args()
        _lib.call('ppsx_intersect_emit', v, int(v.shape[0]), f, int(f.shape[0]), lo, hi, live, small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets,
                  large, nl, count, pair_offsets, int(pairs.shape[0]), pairs)


def _walk(v, f, max_pairs, want_pairs, cell=None, capacity=None, large_above=None, timer=None):
    """(flag u8 [nf], pairs int64 [np,2] ascending or None, info) of a checked device mesh.  timer(name) is called before every part -- boxes,
    lists, count, emit, output (tools/time_intersect.py)."""
    nf, dev = int(f.shape[0]), f.device
    tick = timer or (lambda name: None)
    info = {'faces_in': nf, 'faces_live': 0, 'faces_intersecting': 0, 'pairs': 0, 'boxed_pairs': 0, 'pairs_listed': True, 'max_pairs': max_pairs}
    empty = torch.zeros(0, 2, dtype=torch.int64, device=dev)
    if nf == 0:
        return torch.zeros(0, dtype=torch.uint8, device=dev), empty if want_pairs else None, info
    tick('boxes')
    lo, hi, ext, live = face_boxes(v, f)
    tick('lists')
    lists = _Lists(lo, ext, live, cell_edge(ext, live) if large_above is None else float(large_above), cell, capacity)
    tick('count')
    flag, count = torch.empty(nf, dtype=torch.uint8, device=dev), torch.empty(nf, dtype=torch.int32, device=dev)
    boxed = torch.empty(nf, dtype=torch.int32, device=dev)
    lists.count(v, f, lo, hi, live, flag, count, boxed)
    faces_live, flagged, total, boxed_total = torch.stack([live.sum(), flag.sum(), count.sum(), boxed.sum()]).tolist()
    info.update(faces_live=faces_live, faces_intersecting=flagged, pairs=total, boxed_pairs=boxed_total, pairs_listed=total <= max_pairs)
    pairs = None
    if want_pairs:
        pairs = empty
        if 0 < total <= max_pairs:
            tick('emit')
            offsets = torch.cumsum(count, 0, dtype=torch.int64) - count
            rows = torch.full((total, 2), -1, dtype=torch.int64, device=dev)
            lists.emit(v, f, lo, hi, live, count, offsets, rows)
            keys = torch.sort((rows[:, 0] << 32) | rows[:, 1])[0]                      # f, g < 2^31: the canonical order
            pairs = torch.stack([keys >> 32, keys & 0xFFFFFFFF], dim=1).contiguous()
    tick('output')
    return flag, pairs, info


def _checked(what, verts, faces):
    """The device mesh of a public function.  Non-finite vertices are taken: a face with such a corner is not live."""
    topology.need_device(what, verts, faces)
    return topology.checked_mesh(what, verts, faces, limit=True, finite=False)


def self_intersections(verts: torch.Tensor, faces: torch.Tensor, max_pairs=MAX_PAIRS, return_pairs=False, cell=None, capacity=None,
                       large_above=None):
    """(flags bool [nf], info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3]: flags[f] is set when face f crosses some other face
    (DESIGN.md section 29); with return_pairs (flags, pairs, info), pairs int64 [np,2] the crossing pairs f < g in ascending order of (f, g),
    so that flags[f] is set exactly when f occurs in pairs.  Only live faces take part: valid for nv vertices and with nine finite
    coordinates (non-finite vertices are no error here); a pair is tested when the boxes overlap and the faces share at most one vertex
    index -- coincident but unwelded vertices are not shared, weld first.  Not detected, by design: coplanar overlaps, contacts where a
    vertex lies exactly in the other face's plane, zero-area faces.  When the mesh has more than max_pairs crossing pairs they are not
    listed: info['pairs_listed'] is False and pairs is empty, flags and counts stay exact.  float64 or non-contiguous input is taken like its
    float32 contiguous copy; the inputs are not written.  A pure function of the ordered mesh: `cell` (the cell edge, >= large_above),
    `capacity` (of the cell table) and `large_above` (the extent above which a face is walked as a list entry instead of through the
    cells) are test switches, results do not depend on them.  info: faces_in, faces_live, faces_intersecting, pairs, boxed_pairs (the pairs
    f < g that reached the edge tests), pairs_listed, max_pairs.  ValueError: max_pairs no integer in 0..2^31 - 1 (or a bool), more than
    2^31 - 1 vertices or faces, CPU tensors (CpuTensorError)."""
    max_pairs = _checked_params(max_pairs)
    v, f = _checked('self_intersections', verts, faces)
    flag, pairs, info = _walk(v, f, max_pairs, return_pairs, cell, capacity, large_above)
    return (flag.bool(), pairs, info) if return_pairs else (flag.bool(), info)


def remove_self_intersections(verts: torch.Tensor, faces: torch.Tensor):
    """(verts, faces_kept, kept_rows, info): the device mesh without the faces that `self_intersections` flags.  The vertices come back as
    given (the same tensor), the faces in order without the flagged ones, kept_rows int64 the rows of `faces` that stayed; when nothing is
    flagged `faces` itself comes back.  The holes this cuts are for fill.fill_holes to close.  info as self_intersections, and faces_out."""
    v, f = _checked('remove_self_intersections', verts, faces)
    flag, _, info = _walk(v, f, MAX_PAIRS, False)
    info['faces_out'] = info['faces_in'] - info['faces_intersecting']
    if info['faces_intersecting'] == 0:
        return verts, faces, torch.arange(int(faces.shape[0]), dtype=torch.int64, device=faces.device), info
    rows = torch.nonzero(flag == 0)[:, 0].contiguous()
    return verts, faces[rows].contiguous(), rows, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.intersect',
                                 description='Find the faces of a mesh that cross another face (GPU) and report, remove or select them.  Faces that '
                                             'share an edge are never a pair and unwelded seams are not shared vertices: weld first.  Coplanar '
                                             'overlaps and contacts exactly in a plane are not detected.')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', nargs='?', default=None, help='PLY mesh to write; without it the command only reports')
    ap.add_argument('--action', choices=('remove', 'select'), default=None,
                    help='what OUT holds: the mesh without the crossing faces (remove, the default) or only the crossing faces (select); '
                         'vertices and colours are written as read')
    ap.add_argument('--pairs_out', default=None, help='.npy file for the crossing pairs, int64 [np,2] ascending')
    ap.add_argument('--max_pairs', type=int, default=MAX_PAIRS, help='do not list the pairs of a mesh that has more than this many')
    args = ap.parse_args(argv)
    try:
        max_pairs = _checked_params(args.max_pairs)
    except ValueError as e:
        ap.error(str(e))
    if args.out_file is None and args.action is not None:
        ap.error('--action needs an output file')
    if args.out_file is not None:
        meshio.need_ply_output(ap, args.out_file)
    if args.pairs_out is not None and not args.pairs_out.lower().endswith('.npy'):
        ap.error('--pairs_out must end in .npy')
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.intersect')
    flag, pairs, info = _walk(*mesh.to_device(limit='faces'), max_pairs, args.pairs_out is not None)
    if args.pairs_out is not None:
        np.save(args.pairs_out, pairs.cpu().numpy())
    if args.out_file is not None:
        flag = flag.cpu().numpy().astype(bool)
        mesh.write_as_read(args.out_file, faces=mesh.faces[flag if args.action == 'select' else ~flag])
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
