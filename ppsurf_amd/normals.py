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

from . import _lib, meshio, ops

MAX_K = 256
MAX_COUNT = 2 ** 31 - 1
WEIGHTS = {'area': 0, 'max': 1}
_SENTINEL = 2 ** 63 - 1


class CpuTensorError(_lib.PpsError, ValueError):
    """CPU tensors given to vertex_normals / point_normals: the PpsError of every module's device guard, and a ValueError like their other
    argument errors."""


def _checked_weight(weight):
    if not isinstance(weight, str) or weight not in WEIGHTS:
        raise ValueError('weight must be \'area\' or \'max\', got {!r}'.format(weight))
    return weight


def _checked_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError('k must be an integer in 1..{}, got {!r}'.format(MAX_K, k))
    return int(k)


def _need_device(what, *tensors):
    try:
        return _lib.need_device(what, *tensors)
    except _lib.PpsError as e:
        raise CpuTensorError(str(e)) from None


def _checked_mesh(what, verts, faces):
    assert verts.dim() == 2 and verts.shape[1] == 3 and faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    v, f = verts.contiguous().float(), faces.contiguous()
    if v.shape[0] > MAX_COUNT or f.shape[0] > MAX_COUNT:
        raise ValueError('{}: at most 2^31 - 1 vertices and faces, got {} and {}'.format(what, v.shape[0], f.shape[0]))
    if not bool(torch.isfinite(v).all()):
        raise ValueError('{}: the mesh has non-finite vertices'.format(what))
    return v, f


def _corner_keys(faces, nv):
    """Sorted keys int64 [3 nf] of ppsx_normals_corner_keys: (vertex << 32) | face, the three keys of an invalid face last."""
    nf = int(faces.shape[0])
    keys = torch.empty(3 * nf, dtype=torch.int64, device=faces.device)
    _lib.call('ppsx_normals_corner_keys', faces, nf, nv, keys)
    return torch.sort(keys)[0]


def _incidence(keys, nv):
    keys = keys[keys != _SENTINEL]
    offsets = torch.zeros(nv + 1, dtype=torch.int64, device=keys.device)
    offsets[1:] = torch.cumsum(torch.bincount(keys >> 32, minlength=nv), 0)
    return offsets, (keys & 0xFFFFFFFF).to(torch.int32)


def vertex_incidence(faces: torch.Tensor, nv: int):
    """(offsets int64 [nv + 1], inc int32 [ni]) on the device: row i lists the valid faces that hold vertex i in ascending face index (a
    duplicated face is two faces).  A face is valid when its indices lie in [0, nv) and are pairwise distinct.  One key per corner from the
    kernel and one sort; the keys are distinct, so the rows do not depend on the sort implementation."""
    _need_device('vertex_incidence', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_COUNT or faces.shape[0] > MAX_COUNT:
        raise ValueError('nv and the number of faces must be in 0..2^31 - 1, got {} and {}'.format(nv, faces.shape[0]))
    return _incidence(_corner_keys(faces.contiguous(), int(nv)), int(nv))


def _vertex_normals(v, f, weight):
    """(normals f32 [nv,3], valid faces) of a checked device mesh."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    keys = _corner_keys(f, nv)
    offsets, inc = _incidence(keys, nv)
    out = torch.empty(nv, 3, dtype=torch.float32, device=v.device)          # the kernel writes every row
    _lib.call('ppsx_normals_vertex', v, nv, f, nf, offsets, inc, int(inc.shape[0]), WEIGHTS[weight], out)
    return out, int(inc.shape[0]) // 3


def _zero_rows(n):
    return int((n == 0).all(dim=1).sum().item())


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor, weight: str = 'area'):
    """(normals f32 [nv,3], info) for the device mesh verts f32 [nv,3] / faces int64 [nf,3]: per vertex the normalised fp64 sum over its valid
    faces, in ascending face index, of the cross product of the two edges that leave the vertex ('area'), divided by the product of their
    squared lengths ('max').  The normals follow the winding; a vertex without a valid face, or whose sum has no finite positive length, gets
    (0, 0, 0).  info: vertices, faces_valid, zero_normals, weight.  ValueError: an unknown weight, non-finite vertices, CPU tensors
    (CpuTensorError)."""
    weight = _checked_weight(weight)
    _need_device('vertex_normals', verts, faces)
    v, f = _checked_mesh('vertex_normals', verts, faces)
    out, valid = _vertex_normals(v, f, weight)
    return out, {'vertices': int(v.shape[0]), 'faces_valid': valid, 'zero_normals': _zero_rows(out), 'weight': weight}


def blend_normals(idx: torch.Tensor, d2: torch.Tensor, normals: torch.Tensor, eps: float = 1e-30) -> torch.Tensor:
    """f32 [m,3]: per row the sum of normals f32 [nv,3] at idx int64 [m,k] with the weights 1 / (double(d2) + eps), d2 f32 [m,k], in column
    order in fp64, normalised; entries of idx outside [0, nv) are skipped and a row whose sum has no finite positive length is (0, 0, 0)."""
    _need_device('blend_normals', idx, d2, normals)
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
    dev = _need_device('point_normals', points, verts, faces)
    assert points.dim() == 2 and points.shape[1] == 3
    v, f = _checked_mesh('point_normals', verts, faces)
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
    from .transfer import _ply_stores_doubles
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
    for name in (args.out_file, args.points_out):
        if name is not None and os.path.splitext(name)[1].lower() != '.ply':
            ap.error('the outputs are .ply files')
    if not torch.cuda.is_available():
        raise _lib.PpsError('python -m ppsurf_amd.normals runs on the GPU only; there is no CPU fallback')
    double = False
    if os.path.splitext(args.mesh)[1].lower() == '.ply':
        verts, faces = meshio.read_ply_mesh(args.mesh, dtype=np.float64)
        double = _ply_stores_doubles(args.mesh)
        colors = meshio.read_ply_vertex_colors(args.mesh)
    else:
        verts, faces, colors = meshio.load_mesh_any(args.mesh)
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(verts).all():
        raise SystemExit('{} has non-finite vertices'.format(args.mesh))
    # centred on the mesh's box centre in float64 on the host and only then cast to float32 (geo-referenced coordinates)
    centre = (verts.min(axis=0) + verts.max(axis=0)) * 0.5 if verts.shape[0] else np.zeros(3)
    dev = torch.device('cuda')
    local = torch.from_numpy((verts - centre[None]).astype(np.float32)).to(dev)
    dev_faces = torch.from_numpy(np.asarray(faces, dtype=np.int64).reshape(-1, 3)).to(dev)
    nrm, info = vertex_normals(local, dev_faces, weight)
    meshio.write_ply_mesh_normals(args.out_file, verts, faces, nrm.cpu().numpy(), colors_u8=colors, double=double)
    if args.points is not None:
        pts = np.asarray(meshio.load_pts(args.points))[:, :3].astype(np.float64)
        if not np.isfinite(pts).all():
            raise SystemExit('{} has non-finite points'.format(args.points))
        if verts.shape[0] == 0:
            raise SystemExit('{} has no vertices to take normals from'.format(args.mesh))
        pts_double = os.path.splitext(args.points)[1].lower() == '.las' or (
            os.path.splitext(args.points)[1].lower() == '.ply' and _ply_stores_doubles(args.points))
        scan = torch.from_numpy((pts - centre[None]).astype(np.float32)).to(dev)          # the scan on the mesh's centre: one frame
        pn, pinfo = point_normals(scan, local, dev_faces, k=k, weight=weight)
        meshio.write_ply_points_normals(args.points_out, pts, pn.cpu().numpy(), double=pts_double)
        info = dict(info, points=pinfo['points'], k=pinfo['k'], zero_point_normals=pinfo['zero_normals'])
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
