"""Weld of a mesh on the GPU: vertices that coincide, or lie within a tolerance, become one row, and the faces this collapses leave
(csrc/pps_weld.hip).

    python -m ppsurf_amd.weld MESH OUT.ply [--eps E] [--drop_duplicates]

Every other mesh stage reads connectivity from vertex row numbers: two faces are neighbours only when they name the same rows.  That holds
for the meshes `pps.py rec` writes and fails for most meshes from elsewhere: an STL is three private corners per facet, an OBJ export
splits vertices along its seams, scanners and CAD tools write soups.  This stage is the front door for those: weld, then orient, pieces,
decimate, normals.  Rows i != j are linked when ((dx dx + dy dy) + dz dz) <= eps * eps in fp64 on the float32 vertices; the clusters are
the connected components of the links and the leader of a cluster is its smallest row.  That is single linkage and it CHAINS: a row of
points each within eps of the next is one cluster, however far apart its ends lie.  It is the price of an answer that is a pure function
of (verts, faces, eps, drop_duplicates) and does not depend on the vertex order of a greedy merge or on timing; keep eps well below the
shortest edge that should survive.  The leaders come out in ascending row, byte for byte -- nothing is averaged -- and a leader that no
kept face references stays: the weld deletes duplicates and nothing else, so `vertex_clusters` also deduplicates a bare cloud.  A face
that was invalid as given or that has two corners in one cluster leaves; the others keep their order and their winding.  The models have
no switch for this stage: the meshes `rec` writes are welded already.
"""
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib, labels, mesh_cli, meshio, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)
from .trim import SupportGrid, _f32_not_below

MAX_COUNT = topology.MAX_COUNT
H_FLOOR = 2.0 ** -100                      # the least cell edge (eps = 0, or all rows at one point): 1 / h stays a float32; no result depends on it


def _checked_eps(eps):
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise ValueError('eps must be a finite number >= 0, got {!r}'.format(eps))
    eps = float(eps)
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError('eps must be a finite number >= 0, got {}'.format(eps))
    return eps


def _clusters(v, eps, cell=None, capacity=None):
    """(leader int32 [nv], rounds) of contiguous finite device vertices f32 [nv,3]: the cell lists of trim.SupportGrid, then hooking and
    compressing until a hook launch changes nothing.  The rounds depend on the vertex order and on timing; the leaders do not.  `cell`
    (any cell edge > 0) and `capacity` (of the cell table) are test switches: results do not depend on them."""
    nv = int(v.shape[0])
    label = torch.arange(nv, dtype=torch.int32, device=v.device)
    if nv == 0:
        return label, 0
    grid = SupportGrid(v, capacity)
    # a cell edge of eps, of the box's longest edge when eps is larger than that, and never below the floor or the grid's 2^20 cells per axis
    grid.build(grid.edge_for(max(min(eps, float(grid.ext)), H_FLOOR)) if cell is None else _f32_not_below(cell))
    def hook(changed):
        _lib.call('ppsx_weld_hook', grid.pts, nv, grid._vec3(grid.lo), grid._vec3(grid.hi), float(grid.h), float(grid.inv_h), grid._table,
                  grid.capacity, grid.order, grid.offsets, eps, label, changed)
    return label, labels.fixed_point(hook, lambda: labels.compress(label, nv), v.device)


def _dropped_duplicates(kept):
    """bool [n]: False for a kept face whose set of three indices an earlier kept face holds (either winding).  Integer work in torch."""
    n = int(kept.shape[0])
    if n == 0:
        return torch.ones(0, dtype=torch.bool, device=kept.device)
    corners = torch.sort(kept, dim=1)[0]
    inverse = torch.unique(corners, dim=0, return_inverse=True)[1]
    index = torch.arange(n, dtype=torch.int64, device=kept.device)
    first = torch.full((int(inverse.max().item()) + 1,), n, dtype=torch.int64, device=kept.device).scatter_reduce_(0, inverse, index, 'amin')
    return first[inverse] == index


def _weld_rows(verts, faces, eps, drop_duplicates, cell=None, capacity=None):
    """(leader rows int64 ascending, new faces, info) of a checked device mesh and a checked eps: the weld on row numbers, so that a
    caller can gather whatever it keeps per vertex.  The rows are None when the mesh comes back as given: no two rows linked and either no
    valid face or every face valid and no duplicate dropped."""
    nv, nf, dev = int(verts.shape[0]), int(faces.shape[0]), faces.device
    leader, _ = _clusters(verts, eps, cell, capacity)
    _, rows, number = labels.leaders(leader)
    sizes = torch.bincount(leader.long(), minlength=nv)
    newrow = number[leader.long()].contiguous()
    out = torch.empty_like(faces)
    code = torch.empty(nf, dtype=torch.uint8, device=dev)
    _lib.call('ppsx_weld_faces', faces, nf, nv, newrow, out, code)
    kept = out[code == 0]
    invalid, collapsed, valid = int((code == 1).sum().item()), int((code == 2).sum().item()), int(kept.shape[0])
    duplicate = 0
    if drop_duplicates:
        kept = kept[_dropped_duplicates(kept)]
        duplicate = valid - int(kept.shape[0])
    info = {'vertices_in': nv, 'vertices_out': int(rows.shape[0]), 'clusters_merged': int((sizes >= 2).sum().item()),
            'largest_cluster': int(sizes.max().item()) if nv else 0, 'faces_in': nf, 'faces_invalid': invalid, 'faces_collapsed': collapsed,
            'faces_duplicate': duplicate, 'faces_out': int(kept.shape[0]), 'eps': eps, 'drop_duplicates': drop_duplicates}
    if info['vertices_out'] == nv and (valid == 0 or (invalid == 0 and duplicate == 0)):          # (no merge: nothing collapsed)
        info['faces_out'] = nf
        return None, faces, info
    return rows, kept, info


def vertex_clusters(verts: torch.Tensor, eps=0.0) -> torch.Tensor:
    """leader int32 [nv] on the device: the smallest row of the cluster of every row of verts f32 [nv,3].  Rows i != j are linked when
    ((dx dx + dy dy) + dz dz) <= eps * eps (fp64 on the float32 values, every operation rounded on its own; with eps = 0: equal
    coordinates, -0.0 equal to +0.0); the clusters are the connected components of the links -- single linkage, which chains.
    verts[leader == arange(nv)] is the cloud without its duplicates.  ValueError: an eps that is a bool, no number, not finite or < 0,
    non-finite vertices, more than 2^31 - 1 rows, a CPU tensor (CpuTensorError)."""
    eps = _checked_eps(eps)
    topology.need_device('vertex_clusters', verts)
    v, _ = topology.checked_mesh('vertex_clusters', verts, torch.zeros((0, 3), dtype=torch.int64, device=verts.device), limit=True)
    return _clusters(v, eps)[0]


def weld_mesh(verts: torch.Tensor, faces: torch.Tensor, eps=0.0, drop_duplicates=False):
    """(verts, faces, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] with every cluster of `vertex_clusters` as one row.
    The clusters are single linkage: a row of points each within eps of the next is ONE cluster although its ends lie further apart; that
    is what makes the result independent of the vertex order and of timing.  Vertices out: the leaders (the smallest row of every
    cluster) in ascending row, byte for byte -- no averaging; a leader that no kept face references stays.  Faces out: in their given
    order and winding with the corners renumbered, without the faces that are invalid as given (an index outside [0, nv) or two equal
    indices) and without the valid ones that have two corners in one cluster; with drop_duplicates also without every kept face whose set
    of three new indices an earlier kept face holds, in either winding.  The same tensors come back when no two rows are linked and
    either no face is valid (an empty mesh included) or every face is valid and no duplicate is dropped.  info: vertices_in,
    vertices_out, clusters_merged (clusters of at least two rows), largest_cluster, faces_in, faces_invalid, faces_collapsed,
    faces_duplicate, faces_out, eps, drop_duplicates.  ValueError: an eps that is a bool, no number, not finite or < 0, non-finite
    vertices, more than 2^31 - 1 vertices or faces, CPU tensors (CpuTensorError)."""
    eps = _checked_eps(eps)
    topology.need_device('weld_mesh', verts, faces)
    v, f = topology.checked_mesh('weld_mesh', verts, faces, limit=True)
    rows, out_f, info = _weld_rows(v, f, eps, bool(drop_duplicates))
    if rows is None:
        return verts, faces, info
    return verts[rows], out_f, info


def read_input(path: str):
    """(verts float64 [nv,3], faces int [nf,3], colours uint8 [nv,3] or None, double) of the command's input: a PLY or an OBJ through
    meshio.read_mesh_file; an .stl, binary or ascii, as the soup it stores -- three private corners per facet, no colours, not double."""
    if os.path.splitext(path)[1].lower() == '.stl':
        verts = meshio.read_stl_vertices(path)
        return verts, np.arange(verts.shape[0], dtype=np.int64).reshape(-1, 3), None, False
    return meshio.read_mesh_file(path)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.weld',
                                 description='Weld a mesh: coincident and close vertices become one row, collapsed faces leave (GPU).')
    ap.add_argument('mesh', help='PLY, OBJ or STL mesh')
    ap.add_argument('out_file', help='welded PLY mesh')
    ap.add_argument('--eps', type=float, default=0.0,
                    help='vertices within this distance of each other, in file units, become one; chains of such vertices too.  0 (the '
                         'default): equal after the cast to float32 of the coordinates relative to the centre of the mesh\'s box')
    ap.add_argument('--drop_duplicates', action='store_true', help='drop a face whose three vertices an earlier face holds, in either winding')
    args = ap.parse_args(argv)
    try:
        eps = _checked_eps(args.eps)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.weld', reader=read_input)
    local, f = mesh.to_device(limit='faces')
    pairs_in = int(topology.manifold_pair_edges(f, int(local.shape[0]))[0].shape[0])
    rows, out_f, info = _weld_rows(local, f, eps, args.drop_duplicates)
    if rows is None:
        mesh.write_as_read(args.out_file)
    else:
        mesh.write_rows(args.out_file, rows, out_f)
    pairs_out = int(topology.manifold_pair_edges(out_f.contiguous(), info['vertices_out'])[0].shape[0])
    report = dict(info, pairs_in=pairs_in, pairs_out=pairs_out, closed=2 * pairs_out == 3 * info['faces_out'])
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main(sys.argv[1:])
