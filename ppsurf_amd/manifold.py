"""Manifold split of a mesh on the GPU: an edge that three and more faces hold and a vertex whose faces form several fans are cut apart
by duplicating vertices (csrc/pps_manifold.hip).

    python -m ppsurf_amd.manifold MESH OUT.ply

The other mesh stages step around non-manifold geometry: the decimation only collapses edges between regular vertices, the hole filling
leaves alone loops through a non-manifold fan, the orientation calls a solid that touches another along an edge open, and the face
components treat an edge with three and more owners as joining nothing.  The vertex clustering makes such edges at coarse grids, Marching
Cubes can put four triangles on one edge, and a weld at eps > 0 glues parts at edges and points.  This stage repairs them.  Corner
c = 3 f + k of a valid face names the vertex faces[f, k].  Across every edge that exactly two valid faces hold, the corners of the two
faces at each end of the edge are linked; a fan is a connected component of the links and its leader is its smallest corner.  At a vertex
the fan with the smallest leader keeps the row, every other fan gets a new row with the same position, appended in ascending order of fan
leader, and every corner is renamed to its fan's row.  After that no edge has more than two valid owners and the valid faces at every
vertex form one fan -- a path or a cycle across two-owner edges -- so every vertex with a face and without a border is regular.
Vertices are duplicated and never moved; faces are never added, removed, reordered or re-wound; the result is a pure function of the
ordered mesh and a second run changes nothing.  The cut closes nothing: the faces of a many-owner edge that the fans do not pair become
borders, and two holes that touch at one vertex become one figure-eight loop, which the hole filling leaves alone.  The models have no
switch for this stage: run the command on the PLY that `pps.py rec` or another stage wrote.
"""
import json
import sys

import torch

from . import _lib, labels, mesh_cli, meshio, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT


def _checked_corners(what, nf):
    """ValueError when the 3 nf corners of nf faces do not fit an int32 label."""
    if 3 * int(nf) > MAX_COUNT:
        raise ValueError('{}: at most (2^31 - 1) / 3 faces (one int32 label per corner), got {}'.format(what, nf))


def _fans(f, nv, fa, fb, ea, eb, valid):
    """(label int32 [3 nf], rounds) of contiguous device faces and their pair list: label[c] = c for the corners of the valid faces and
    -1 for the others, then hooking and compressing until a hook launch changes nothing.  The rounds depend on the face order and on
    timing; the labels do not."""
    nf = int(f.shape[0])
    own = torch.arange(3 * nf, dtype=torch.int32, device=f.device)
    label = torch.where(valid.repeat_interleave(3), own, torch.full_like(own, -1))
    pairs, rounds = int(fa.shape[0]), 0
    if pairs > 0:
        rounds = labels.fixed_point(lambda changed: _lib.call('ppsx_manifold_hook', f, nf, nv, fa, fb, ea, eb, pairs, label, changed),
                                    lambda: labels.compress(label, 3 * nf), f.device)
    return label, rounds


def _rows(f, nv, label):
    """(newrow int64 [3 nf], source int64 [nv_out], fans int64 [nv]) of the corner labels at their fixed point: per vertex the fan with
    the smallest leader keeps the row, the other fans get the rows nv, nv + 1, ... in ascending leader; newrow is set at the leaders (the
    identity elsewhere, never read), source is the given row of every output row and fans the number of fans at every given vertex.
    Integer work on small tables in torch."""
    nc, dev = int(label.shape[0]), f.device
    leader = torch.nonzero(label == torch.arange(nc, dtype=torch.int32, device=dev)).reshape(-1)   # ascending (no numbers: not labels.leaders)
    at = f.reshape(-1)[leader]                                                                         # the vertex every fan names
    first = torch.full((nv,), nc, dtype=torch.int64, device=dev).scatter_reduce_(0, at, leader, 'amin')
    extra = first[at] != leader
    row = at.clone()
    row[extra] = nv + torch.arange(int(extra.sum().item()), dtype=torch.int64, device=dev)
    newrow = torch.arange(nc, dtype=torch.int64, device=dev)
    newrow[leader] = row
    return newrow, torch.cat([torch.arange(nv, dtype=torch.int64, device=dev), at[extra]]), torch.bincount(at, minlength=nv)


def _edge_counts(owners):
    return int((owners == 1).sum().item()), int((owners == 2).sum().item()), int((owners >= 3).sum().item())


def _split_rows(verts, faces):
    """(source rows int64 [nv_out], new faces or None, info) of a checked device mesh: the split on row numbers, so that a caller can
    gather whatever it keeps per vertex.  The faces are None when the mesh comes back as given: no vertex has a second fan, and the
    source rows are 0 .. nv - 1."""
    nv, nf, dev = int(verts.shape[0]), int(faces.shape[0]), faces.device
    runs = topology.edge_runs(faces, nv)
    fa, fb, ea, eb, valid = topology.pairs_of_runs(*runs)
    border, manifold, nonmanifold = _edge_counts(runs[2])
    label, _ = _fans(faces, nv, fa, fb, ea, eb, valid)
    newrow, source, fans = _rows(faces, nv, label)
    nv_out = int(source.shape[0])
    info = {'vertices_in': nv, 'vertices_out': nv_out, 'vertices_split': int((fans >= 2).sum().item()),
            'max_fans': int(fans.max().item()) if nv else 0, 'faces_in': nf, 'faces_valid': int(valid.sum().item()),
            'edges_border_in': border, 'edges_border_out': border, 'edges_manifold_in': manifold, 'edges_manifold_out': manifold,
            'edges_nonmanifold_in': nonmanifold}
    if nv_out == nv:
        info['closed_out'] = 2 * manifold == 3 * info['faces_valid']
        return source, None, info
    if nv_out > MAX_COUNT:
        raise ValueError('the split mesh would have {} vertices, more than 2^31 - 1'.format(nv_out))
    out = torch.empty_like(faces)
    _lib.call('ppsx_manifold_faces', faces, nf, nv, label, newrow, nv_out, out)
    border, manifold, _ = _edge_counts(topology.edge_runs(out, nv_out)[2])
    info.update(edges_border_out=border, edges_manifold_out=manifold, closed_out=2 * manifold == 3 * info['faces_valid'])
    return source, out, info


def corner_fans(faces: torch.Tensor, nv: int) -> torch.Tensor:
    """label int32 [3 nf] on the device for faces int64 [nf,3]: corner c = 3 f + k of a valid face f names the vertex faces[f, k], and
    label[c] is the smallest corner of its fan; -1 for the corners of an invalid face.  A face is valid when its indices lie in [0, nv)
    and are pairwise distinct.  Across every undirected edge that exactly two valid faces hold, the two corners that name one end of the
    edge are linked, and likewise the two at the other end; a fan is a connected component of the links.  The faces around a manifold
    vertex are one fan; `label == arange(3 nf)` marks one corner per fan."""
    topology.need_device('corner_fans', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_COUNT or faces.shape[0] > MAX_COUNT:
        raise ValueError('nv and the number of faces must be in 0..2^31 - 1, got {} and {}'.format(nv, faces.shape[0]))
    _checked_corners('corner_fans', faces.shape[0])
    f = faces.contiguous()
    return _fans(f, int(nv), *topology.manifold_pair_edges(f, int(nv)))[0]


def split_nonmanifold(verts: torch.Tensor, faces: torch.Tensor, return_source=False):
    """(verts, faces, info) of the device mesh verts [nv,3] / faces int64 [nf,3] with every vertex that has several fans (`corner_fans`)
    split: the fan with the smallest leader keeps the vertex's row, every other fan gets a new row after the nv given ones, in ascending
    order of fan leader, with the vertex's position byte for byte, and every corner of a valid face is renamed to its fan's row.  An
    invalid face is copied as given, a vertex without a valid face stays, the faces keep their order and their winding.  Afterwards no
    edge has more than two valid owners and the valid faces at every vertex form one fan; a second call returns its arguments.  Nothing
    is closed: faces of a many-owner edge that the fans do not pair become borders.  The same tensors come back when no vertex has a
    second fan, the empty mesh included.  info: vertices_in, vertices_out, vertices_split (given vertices with at least two fans),
    max_fans, faces_in, faces_valid, edges_border_in / edges_border_out (one owner), edges_manifold_in / edges_manifold_out (two),
    edges_nonmanifold_in (three and more; there is none afterwards), closed_out (2 edges_manifold_out == 3 faces_valid).  With
    return_source a fourth value comes back: source int64 [vertices_out] on the device, the given row of every output row, for callers
    that carry attributes per vertex (colours[source], normals[source]).
    ValueError: non-finite vertices, more than 2^31 - 1 vertices or faces, 3 nf > 2^31 - 1, CPU tensors (CpuTensorError)."""
    topology.need_device('split_nonmanifold', verts, faces)
    v, f = topology.checked_mesh('split_nonmanifold', verts, faces, limit=True)
    _checked_corners('split_nonmanifold', f.shape[0])
    source, out, info = _split_rows(v, f)
    res = (verts, faces, info) if out is None else (verts[source], out, info)
    return res + (source,) if return_source else res


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.manifold',
                                 description='Split the non-manifold edges and vertices of a mesh by duplicating vertices (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='PLY mesh with the split vertices appended')
    args = ap.parse_args(argv)
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.manifold')
    source, out, info = _split_rows(*mesh.to_device(limit='corners'))
    if out is None:
        mesh.write_as_read(args.out_file)
    else:
        mesh.write_rows(args.out_file, source, out)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
