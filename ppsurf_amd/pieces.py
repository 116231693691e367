"""Isolated pieces of a mesh on the GPU: the connected components of its faces, a table per component, and the rules that drop components
(csrc/pps_pieces.hip).

    python -m ppsurf_amd.pieces MESH OUT.ply [--min_faces N] [--min_diag_frac F] [--keep_largest K]

Reconstruction leaves floating blobs in empty space next to a noisy scan, and the trim leaves islands around the openings of a sparse one.
The reference's rule, remove_small_connected_components(num_faces = 6), walks a bounded neighbourhood per face and stops at 32 faces; this
module labels the components in full, so "below 500 faces", "smaller than a tenth of the model" and "the largest piece" are one call.  Two
valid faces are adjacent when they share an undirected edge that exactly two valid faces hold (the product's own rule); a component is
named by its leader, its smallest face index.  The table holds counts, minima and maxima only, so it is exact in any order of
accumulation, and the result is a pure function of (verts, faces, rules).  At least one rule must be given and none has a default: none
has been tuned on network output.  The models have no switch for this stage: run the command on the PLY that `pps.py rec` wrote; it
prints the eight largest components, so thresholds can be picked from one run.
"""
import json
import math
import sys

import numpy as np
import torch

from . import _lib, labels, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT
TOP = 8                                    # the command lists that many first-ranked components


def _checked_count(name, value):
    return None if value is None else params.integer(name, value, 1, MAX_COUNT, '1..2^31 - 1')


def _checked_rules(min_faces, min_diag_frac, keep_largest):
    """(min_faces int or None, min_diag_frac float or None, keep_largest int or None) or a ValueError: the counts integers in 1..2^31 - 1,
    the fraction finite in [0, 1], at least one rule."""
    min_faces, keep_largest = _checked_count('min_faces', min_faces), _checked_count('keep_largest', keep_largest)
    if min_diag_frac is not None:
        if isinstance(min_diag_frac, bool) or not isinstance(min_diag_frac, (int, float, np.integer, np.floating)):
            raise ValueError('min_diag_frac must be a number in [0, 1], got {!r}'.format(min_diag_frac))
        min_diag_frac = float(min_diag_frac)
        if not (math.isfinite(min_diag_frac) and 0.0 <= min_diag_frac <= 1.0):
            raise ValueError('min_diag_frac must be a finite number in [0, 1], got {}'.format(min_diag_frac))
    if min_faces is None and min_diag_frac is None and keep_largest is None:
        raise ValueError('no rule: give min_faces, min_diag_frac or keep_largest')
    return min_faces, min_diag_frac, keep_largest


def _labels(f, nv):
    """(label int32 [nf], valid bool [nf], rounds) of contiguous device faces: hooking and compressing until a hook launch changes nothing.
    The rounds depend on the face order and on timing; the labels do not."""
    nf = int(f.shape[0])
    fa, fb, valid = topology.manifold_pairs(f, nv)
    own = torch.arange(nf, dtype=torch.int32, device=f.device)
    label = torch.where(valid, own, torch.full_like(own, -1))
    pairs, rounds = int(fa.shape[0]), 0
    if pairs > 0:
        rounds = labels.fixed_point(lambda changed: _lib.call('ppsx_pieces_hook', fa, fb, pairs, label, nf, changed),
                                    lambda: labels.compress(label, nf), f.device)
    return label, valid, rounds


def _diag2(lo, hi):
    """(dx dx + dy dy) + dz dz in fp64 of f32 boxes [..., 3], every operation rounded on its own (torch tensors or numpy arrays)."""
    d = hi.double() - lo.double() if torch.is_tensor(lo) else hi.astype(np.float64) - lo.astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _table(v, f):
    """The component table of a checked device mesh, with `cid` int32 [nf] (the number of a face's component, -1 for an invalid face) and
    `rounds` next to the entries of `component_table`."""
    nv, nf, dev = int(v.shape[0]), int(f.shape[0]), f.device
    label, valid, rounds = _labels(f, nv)
    _, leader, number = labels.leaders(label)
    nc = int(leader.shape[0])
    cid = torch.where(valid, number[label.clamp(min=0).long()], torch.full_like(number, -1)).to(torch.int32)
    count = torch.empty(nc, dtype=torch.int64, device=dev)
    lo, hi = torch.empty(nc, 3, dtype=torch.float32, device=dev), torch.empty(nc, 3, dtype=torch.float32, device=dev)
    _lib.call('ppsx_pieces_stats', v, nv, f, nf, label, cid, nc, count, lo, hi)
    box_diag2 = 0.0
    if nc > 0:
        box_diag2 = float(_diag2(torch.amin(lo, 0).cpu().numpy(), torch.amax(hi, 0).cpu().numpy()))
    return {'label': label, 'leader': leader, 'faces': count, 'lo': lo, 'hi': hi, 'diag2': _diag2(lo, hi), 'box_diag2': box_diag2,
            'cid': cid, 'rounds': rounds, 'faces_valid': int(valid.sum().item())}


def _rank(count):
    """int64 [nc]: the place of every component by faces descending, then leader ascending (the components come in ascending leader)."""
    order = torch.sort(count, descending=True, stable=True)[1]
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.shape[0], dtype=torch.int64, device=count.device)
    return rank


def _selected(table, rank, min_faces, min_diag_frac, keep_largest):
    """bool [nc]: the components that pass every rule given (ppsx_pieces_select)."""
    nc = int(table['leader'].shape[0])
    keep = torch.empty(nc, dtype=torch.uint8, device=table['leader'].device)
    _lib.call('ppsx_pieces_select', table['faces'], table['lo'], table['hi'], rank, nc, int(min_faces is not None), min_faces or 1,
              int(min_diag_frac is not None), min_diag_frac or 0.0, int(keep_largest is not None), keep_largest or 1, table['box_diag2'], keep)
    return keep.bool()


def face_components(faces: torch.Tensor, nv: int) -> torch.Tensor:
    """label int32 [nf] on the device: the smallest face index of the component of every valid face of faces int64 [nf,3], -1 for an
    invalid one.  A face is valid when its indices lie in [0, nv) and are pairwise distinct; two valid faces are adjacent when they share an
    undirected edge that exactly two valid faces hold."""
    topology.need_device('face_components', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_COUNT or faces.shape[0] > MAX_COUNT:
        raise ValueError('nv and the number of faces must be in 0..2^31 - 1, got {} and {}'.format(nv, faces.shape[0]))
    return _labels(faces.contiguous(), int(nv))[0]


def component_table(verts: torch.Tensor, faces: torch.Tensor) -> dict:
    """The components of the device mesh verts f32 [nv,3] / faces int64 [nf,3] in ascending leader, as device tensors: label int32 [nf],
    leader int64 [nc], faces int64 [nc] (the counts), lo and hi f32 [nc,3] (the box of the corners of the component's faces, -0.0 taken as
    +0.0), diag2 f64 [nc] (the squared diagonal of that box); and box_diag2, a Python float, the same over the box of all components (0.0
    without one).  ValueError: non-finite vertices, more than 2^31 - 1 vertices or faces, CPU tensors (CpuTensorError)."""
    topology.need_device('component_table', verts, faces)
    v, f = topology.checked_mesh('component_table', verts, faces, limit=True)
    table = _table(v, f)
    return {k: table[k] for k in ('label', 'leader', 'faces', 'lo', 'hi', 'diag2', 'box_diag2')}


def _pieces_rows(verts, faces, min_faces, min_diag_frac, keep_largest):
    """(kept vertex rows int64 ascending, re-indexed faces, info, top) of a checked device mesh and checked rules: the removal on row
    numbers, so that a caller can gather whatever it keeps per vertex.  The rows are None when the mesh comes back as given (no valid
    face).  top: the first-ranked components as [leader, faces, diag2 / box_diag2] (None where box_diag2 is 0)."""
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    table = _table(verts, faces)
    nc = int(table['leader'].shape[0])
    info = {'faces_in': nf, 'faces_valid': table['faces_valid'], 'faces_out': nf, 'vertices_in': nv, 'vertices_out': nv, 'components': nc,
            'components_kept': 0, 'largest_faces': 0, 'box_diag2': table['box_diag2'], 'min_faces': min_faces, 'min_diag_frac': min_diag_frac,
            'keep_largest': keep_largest}
    if nc == 0:
        return None, faces, info, []
    rank = _rank(table['faces'])
    keep = _selected(table, rank, min_faces, min_diag_frac, keep_largest)
    cid = table['cid'].long()
    kept = faces[(cid >= 0) & keep[cid.clamp(min=0)]]
    used, remap = topology.used_rows(kept, nv)
    rows = torch.nonzero(used).reshape(-1)
    out_f = remap[kept]
    first = torch.sort(rank)[1][:TOP]
    D2 = table['box_diag2']
    top = [[int(l), int(n), float(np.float64(d) / np.float64(D2)) if D2 > 0 else None]
           for l, n, d in zip(table['leader'][first].tolist(), table['faces'][first].tolist(), table['diag2'][first].tolist())]
    info.update(faces_out=int(out_f.shape[0]), vertices_out=int(rows.shape[0]), components_kept=int(keep.sum().item()),
                largest_faces=int(table['faces'].max().item()))
    return rows, out_f, info, top


def remove_pieces(verts: torch.Tensor, faces: torch.Tensor, min_faces=None, min_diag_frac=None, keep_largest=None):
    """(verts, faces, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] without the components that fail a rule.  Each rule is
    optional, at least one must be given, and a component is kept when it passes every rule given: min_faces = N, it has at least N faces;
    min_diag_frac = F in [0, 1], the squared diagonal of its box is at least (F F) times that of the box of all components (fp64, no
    square root); keep_largest = K, it is among the first K by faces descending, then leader ascending, ranked over all components.  The
    kept faces come in their given order, invalid faces are dropped, the vertices no kept face references are dropped with the order of
    the rest kept, the faces are re-indexed, and the surviving vertex rows come back byte for byte.  An empty mesh and a mesh without a
    valid face come back as given.  info: faces_in, faces_valid, faces_out, vertices_in, vertices_out, components, components_kept,
    largest_faces, box_diag2, and the three rules as given.  ValueError: a rule that is a bool, a count that is no integer in
    1..2^31 - 1, a fraction not finite in [0, 1], no rule at all, non-finite vertices, more than 2^31 - 1 vertices or faces, CPU tensors
    (CpuTensorError)."""
    min_faces, min_diag_frac, keep_largest = _checked_rules(min_faces, min_diag_frac, keep_largest)
    topology.need_device('remove_pieces', verts, faces)
    v, f = topology.checked_mesh('remove_pieces', verts, faces, limit=True)
    rows, out_f, info, _ = _pieces_rows(v, f, min_faces, min_diag_frac, keep_largest)
    if rows is None:
        return verts, faces, info
    return verts[rows], out_f, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.pieces',
                                 description='Remove the isolated pieces of a mesh: its face components by size, by extent or by rank (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='PLY mesh without the dropped components')
    ap.add_argument('--min_faces', type=int, default=None, help='keep the components with at least this many faces')
    ap.add_argument('--min_diag_frac', type=float, default=None,
                    help='keep the components whose box diagonal is at least this fraction of the diagonal of the whole; in [0, 1]')
    ap.add_argument('--keep_largest', type=int, default=None, help='keep this many components, the ones with the most faces')
    args = ap.parse_args(argv)
    try:
        rules = _checked_rules(args.min_faces, args.min_diag_frac, args.keep_largest)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.pieces')
    rows, out_f, info, top = _pieces_rows(*mesh.to_device(limit='faces'), *rules)
    if rows is None:
        mesh.write_as_read(args.out_file)
    else:
        mesh.write_rows(args.out_file, rows, out_f)
    report = dict(info, top=top)
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main(sys.argv[1:])
