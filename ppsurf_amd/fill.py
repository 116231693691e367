"""Hole filling of a mesh on the GPU: every border loop of at most `max_edges` edges is closed (csrc/pps_fill.hip).

    python -m ppsurf_amd.fill MESH OUT.ply --max_edges N

The trim by support keeps an open scan open, and punches pinholes wherever the scan is locally sparse; the smoothing then treats every
pinhole rim as a border.  The reference has no mesh repair; `pps.py rec` / `predict` reach this module through the models'
`gen_fill_holes`.  A loop of three edges gets one triangle, a longer one a fan around a new vertex at the centroid of the loop (summed in
fp64 in loop order from its smallest vertex).  Everything given stays byte for byte; the new vertices and faces are appended.  Loops
through a vertex where two holes touch, through a non-manifold fan, and the edges of a free triangle are left alone.  The result is a pure
function of (verts, faces, max_edges) and does not depend on the order of the faces.
"""
import json
import sys

import numpy as np
import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here like from the siblings)

MAX_EDGES = 4096


def _checked_max_edges(max_edges, name='max_edges'):
    """max_edges as an int, or a ValueError: an integer in 3..4096, no bool."""
    return params.integer(name, max_edges, 3, MAX_EDGES)


def fill_holes(verts: torch.Tensor, faces: torch.Tensor, max_edges: int):
    """(verts f32 [nv + new_vertices, 3], faces int64 [nf + new_faces, 3], info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3]:
    the given rows first, unchanged, then one vertex per filled loop of more than three edges and the new faces, loop by loop in ascending
    leader.  An empty mesh and a mesh without rims come back as given.  info: vertices, faces_valid, border_edges (edges of one valid face,
    before), loose_triangles, rim_vertices, nonsimple_rim_vertices, loops_filled, new_vertices, new_faces, border_edges_left, max_edges.
    ValueError: max_edges no integer in 3..4096, non-finite vertices, more than 2^31 - 1 vertices or faces, CPU tensors (CpuTensorError)."""
    max_edges = _checked_max_edges(max_edges)
    topology.need_device('fill_holes', verts, faces)
    v, f = topology.checked_mesh('fill_holes', verts, faces, limit=True)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    info = {'vertices': nv, 'faces_valid': 0, 'border_edges': 0, 'loose_triangles': 0, 'rim_vertices': 0, 'nonsimple_rim_vertices': 0,
            'loops_filled': 0, 'new_vertices': 0, 'new_faces': 0, 'border_edges_left': 0, 'max_edges': max_edges}
    if nv == 0 or nf == 0:
        return v, faces, info
    offsets, nbr, mult, valid = topology.adjacency_rows(f, nv)
    border = int((mult == 1).sum().item()) // 2                       # every edge sits in the rows of both its ends
    info.update(faces_valid=valid, border_edges=border, border_edges_left=border)
    if border == 0:
        return v, faces, info
    succ, cand, rim_edges, rim_vertices, simple = topology.rim_rows(f, nv, offsets, nbr, mult)
    # an edge of one face is a rim half-edge unless its face is loose, and a loose triangle has three of them
    info.update(loose_triangles=(border - rim_edges) // 3, rim_vertices=rim_vertices, nonsimple_rim_vertices=rim_vertices - simple)
    nc = int(cand.shape[0])
    if nc == 0:
        return v, faces, info
    found = torch.zeros(nc, dtype=torch.int32, device=v.device)
    _lib.call('ppsx_fill_loops', cand, nc, succ, nv, max_edges, found)
    keep = found > 0
    leader, length = cand[keep].contiguous(), found[keep].contiguous()
    nl = int(leader.shape[0])
    if nl == 0:
        return v, faces, info
    fan = (length > 3).to(torch.int64)
    rows = torch.where(length > 3, length.to(torch.int64), torch.ones_like(fan))
    vslot, foff = torch.cumsum(fan, 0) - fan, torch.cumsum(rows, 0) - rows           # exclusive: the new vertex and the first new face of a loop
    nnew, nfnew, edges = int(fan.sum().item()), int(rows.sum().item()), int(length.sum().item())
    if nv + nnew > topology.MAX_COUNT or nf + nfnew > topology.MAX_COUNT:
        raise ValueError('fill_holes: the filled mesh would have more than 2^31 - 1 vertices or faces')
    new_v = torch.zeros(nnew, 3, dtype=torch.float32, device=v.device)               # what a loop that emit refuses would leave: a zero vertex
    new_f = torch.full((nfnew, 3), -1, dtype=torch.int64, device=v.device)           # and invalid faces
    _lib.call('ppsx_fill_emit', v, nv, succ, leader, length, vslot, foff, nl, new_v, nnew, new_f, nfnew)
    info.update(loops_filled=nl, new_vertices=nnew, new_faces=nfnew, border_edges_left=border - edges)
    return torch.cat([v, new_v]), torch.cat([f, new_f]), info


def loop_colors(colors, faces, nv):
    """uint8 [new, c]: the colour of every new vertex from the NEW faces of a filled mesh (host arrays; the first nv vertices are the old
    ones with `colors` uint8 [nv, c]): per channel (sum + L // 2) // L over the L vertices of its loop, in integer arithmetic.  A fan face is
    (s_{j+1}, s_j, new vertex), so the loop of a new vertex is the second column of the faces that end in it."""
    colors, faces = np.asarray(colors), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fans = faces[faces[:, 2] >= nv]
    new = int(fans[:, 2].max()) + 1 - nv if fans.shape[0] else 0
    total, count = np.zeros((new, colors.shape[1]), dtype=np.int64), np.zeros(new, dtype=np.int64)
    np.add.at(total, fans[:, 2] - nv, colors[fans[:, 1]].astype(np.int64))
    np.add.at(count, fans[:, 2] - nv, 1)
    return ((total + (count // 2)[:, None]) // np.maximum(count, 1)[:, None]).astype(np.uint8)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.fill', description='Close the small holes of a mesh: border loops of at most N edges (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='filled PLY mesh')
    ap.add_argument('--max_edges', type=int, required=True, help='the longest border loop that is closed, 3..{}'.format(MAX_EDGES))
    args = ap.parse_args(argv)
    try:
        max_edges = _checked_max_edges(args.max_edges, '--max_edges')
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.fill')
    nv, colors = int(mesh.verts.shape[0]), mesh.colors
    out_v, out_f, info = fill_holes(*mesh.to_device(), max_edges)
    out_f = out_f.cpu().numpy()
    # the old vertices keep the file's own values; only the new ones come back from the centred float32 frame
    out_v = np.concatenate([mesh.verts, out_v[nv:].cpu().numpy().astype(np.float64) + mesh.centre[None]])
    if colors is not None:
        colors = np.concatenate([colors, loop_colors(colors, out_f[mesh.faces.shape[0]:], nv)])
    meshio.write_ply_mesh(args.out_file, out_v, out_f, double=mesh.double, colors_u8=colors)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
