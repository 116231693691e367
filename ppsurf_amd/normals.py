"""Oriented normals on the GPU: per vertex on a mesh, per point on a scan (csrc/pps_normals.hip).

    python -m ppsurf_amd.normals MESH OUT.ply [--weight area|max] [--points SCAN --points_out SCAN_OUT.ply --k 8]

The reference writes positions only; `pps.py rec` / `predict` reach this module through the models' `gen_normals`.  A vertex normal is the
normalised fp64 sum of the cross products of the faces around the vertex, walked in ascending face index: weighted by area ('area') or by
Nelson Max's 1 / (|e1|^2 |e2|^2) ('max', Max 1999).  A scan point takes the inverse-squared-distance blend of the normals of its k nearest
vertices (ops.KnnBlocks: exact, ordered by (d2, index)), so an unoriented scan gets the orientation of the surface reconstructed from it.
Both are pure functions of their inputs; the normals follow the winding of the faces and nothing is re-oriented.
"""
import json
import os
import sys

import numpy as np
import torch

from . import _lib, mesh_cli, meshio, ops, params, topology
from .topology import CpuTensorError, vertex_incidence  # noqa: F401  (their home is topology.py; the names stay importable from here)

MAX_K = 256
WEIGHTS = {'area': 0, 'max': 1}


def _checked_weight(weight):
    if not isinstance(weight, str) or weight not in WEIGHTS:
        raise ValueError('weight must be \'area\' or \'max\', got {!r}'.format(weight))
    return weight


def _checked_k(k):
    return params.integer('k', k, 1, MAX_K)


def _vertex_normals(v, f, weight):
    """(normals f32 [nv,3], valid faces) of a checked device mesh."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    offsets, inc, valid = topology.incidence_rows(f, nv)
    out = torch.empty(nv, 3, dtype=torch.float32, device=v.device)          # the kernel writes every row
    _lib.call('ppsx_normals_vertex', v, nv, f, nf, offsets, inc, int(inc.shape[0]), WEIGHTS[weight], out)
    return out, valid


def _zero_rows(n):
    return int((n == 0).all(dim=1).sum().item())


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor, weight: str = 'area'):
    """(normals f32 [nv,3], info) for the device mesh verts f32 [nv,3] / faces int64 [nf,3]: per vertex the normalised fp64 sum over its valid
    faces, in ascending face index, of the cross product of the two edges that leave the vertex ('area'), divided by the product of their
    squared lengths ('max').  The normals follow the winding; a vertex without a valid face, or whose sum has no finite positive length, gets
    (0, 0, 0).  info: vertices, faces_valid, zero_normals, weight.  ValueError: an unknown weight, non-finite vertices, CPU tensors
    (CpuTensorError)."""
    weight = _checked_weight(weight)
    topology.need_device('vertex_normals', verts, faces)
    v, f = topology.checked_mesh('vertex_normals', verts, faces, limit=True)
    out, valid = _vertex_normals(v, f, weight)
    return out, {'vertices': int(v.shape[0]), 'faces_valid': valid, 'zero_normals': _zero_rows(out), 'weight': weight}


def blend_normals(idx: torch.Tensor, d2: torch.Tensor, normals: torch.Tensor, eps: float = 1e-30) -> torch.Tensor:
    """f32 [m,3]: per row the sum of normals f32 [nv,3] at idx int64 [m,k] with the weights 1 / (double(d2) + eps), d2 f32 [m,k], in column
    order in fp64, normalised; entries of idx outside [0, nv) are skipped and a row whose sum has no finite positive length is (0, 0, 0)."""
    topology.need_device('blend_normals', idx, d2, normals)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and normals.dtype == torch.float32
    assert idx.dim() == 2 and idx.shape == d2.shape and normals.dim() == 2 and normals.shape[1] == 3
    idx, d2, normals = idx.contiguous(), d2.contiguous(), normals.contiguous()
    out = torch.empty((idx.shape[0], 3), dtype=torch.float32, device=idx.device)
    _lib.call('ppsx_normals_blend', idx, d2, idx.shape[0], idx.shape[1], normals, normals.shape[0], float(eps), out)
    return out


def point_normals(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, k: int = 8, weight: str = 'area'):
    """(normals f32 [m,3], info) for points f32 [m,3] in the frame of the device mesh verts / faces: the blend of the `weight` vertex normals
    of the min(k, nv) nearest vertices, weighted by 1 / (d2 + 1e-30); k = 1 gives the nearest vertex's normal.  info: points, vertices, k (as
    used), zero_normals, weight.  ValueError: an unknown weight, k outside 1..256, no vertices, non-finite vertices or points, CPU tensors
    (CpuTensorError)."""
    weight, k = _checked_weight(weight), _checked_k(k)
    dev = topology.need_device('point_normals', points, verts, faces)
    assert points.dim() == 2 and points.shape[1] == 3
    v, f = topology.checked_mesh('point_normals', verts, faces, limit=True)
    p = points.contiguous().float()
    if not bool(torch.isfinite(p).all()):
        raise ValueError('point_normals: non-finite points')
    nv, m = int(v.shape[0]), int(p.shape[0])
    if nv == 0:
        raise ValueError('point_normals: the mesh has no vertices')
    k = min(k, nv)
    if m == 0:
        out = torch.empty((0, 3), dtype=torch.float32, device=dev)
    else:
        idx, d2 = ops.KnnBlocks(v).query(p, k, return_d2=True)
        out = blend_normals(idx, d2, _vertex_normals(v, f, weight)[0])
    return out, {'points': m, 'vertices': nv, 'k': k, 'zero_normals': _zero_rows(out), 'weight': weight}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.normals', description='Write a mesh with oriented vertex normals, and optionally a '
                                 'scan with the normals of that surface (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='PLY mesh with nx ny nz')
    ap.add_argument('--weight', default='area', help='area (faces weigh in by their area) or max (Nelson Max\'s weights)')
    ap.add_argument('--points', default=None, help='scan in the mesh\'s frame: .ply, .las, .pcd, .off, .obj, .xyz or .npy')
    ap.add_argument('--points_out', default=None, help='PLY point cloud with nx ny nz')
    ap.add_argument('--k', type=int, default=8, help='nearest vertices blended per scan point (1: the nearest vertex)')
    args = ap.parse_args(argv)
    try:
        weight, k = _checked_weight(args.weight), _checked_k(args.k)
    except ValueError as e:
        ap.error(str(e))
    if (args.points is None) != (args.points_out is None):
        ap.error('--points and --points_out go together')
    meshio.need_ply_output(ap, args.out_file, args.points_out, plural=True)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.normals')
    local, dev_faces = mesh.to_device()
    nrm, info = vertex_normals(local, dev_faces, weight)
    mesh.write_as_read(args.out_file, normals=nrm)
    if args.points is not None:
        pts = np.asarray(meshio.load_pts(args.points))[:, :3].astype(np.float64)
        if not np.isfinite(pts).all():
            raise SystemExit('{} has non-finite points'.format(args.points))
        if mesh.verts.shape[0] == 0:
            raise SystemExit('{} has no vertices to take normals from'.format(args.mesh))
        pts_double = os.path.splitext(args.points)[1].lower() == '.las' or (
            os.path.splitext(args.points)[1].lower() == '.ply' and meshio.ply_stores_doubles(args.points))
        scan = torch.from_numpy(meshio.centred_f32(pts, mesh.centre)).to(local.device)                 # the scan on the mesh's centre: one frame
        pn, pinfo = point_normals(scan, local, dev_faces, k=k, weight=weight)
        meshio.write_ply_points_normals(args.points_out, pts, pn.cpu().numpy(), double=pts_double)
        info = dict(info, points=pinfo['points'], k=pinfo['k'], zero_point_normals=pinfo['zero_normals'])
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
