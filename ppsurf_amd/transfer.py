"""Colour transfer from a scan to a mesh on the GPU: every vertex takes the inverse-squared-distance blend of the colours of its k nearest scan
points (csrc/pps_transfer.hip).

    python -m ppsurf_amd.transfer MESH SCAN OUT.ply [--k 8]

The reference writes uncoloured meshes (source/poco_model.py:269 `mesh.export`); `pps.py rec` / `predict` reach this module through the models'
`gen_color_k`.  The neighbours come from ops.KnnBlocks (exact, ordered by (d2, index)); the blend walks them in that order in fp64, so the
colours are a pure function of the cloud, its colours and the vertices: no float atomics, no dependence on the launch shape.
"""
import json
import sys

import numpy as np
import torch

from . import _lib, meshio, ops

MAX_K = 256


def blend_rgba(idx: torch.Tensor, d2: torch.Tensor, rgba: torch.Tensor, eps: float = 1e-30) -> torch.Tensor:
    """uint8 [m,4]: per row the blend of rgba uint8 [n,4] at idx int64 [m,k] with the weights 1 / (double(d2) + eps), d2 f32 [m,k], summed in
    column order in fp64 and rounded half up; entries of idx outside [0, n) are skipped and a row without a valid entry is 0 0 0 0."""
    _lib.need_device('blend_rgba', idx, d2, rgba)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and rgba.dtype == torch.uint8
    assert idx.dim() == 2 and idx.shape == d2.shape and rgba.dim() == 2 and rgba.shape[1] == 4
    idx, d2, rgba = idx.contiguous(), d2.contiguous(), rgba.contiguous()
    out = torch.empty((idx.shape[0], 4), dtype=torch.uint8, device=idx.device)
    _lib.call('ppsx_blend_rgba_u8', idx, d2, idx.shape[0], idx.shape[1], rgba, rgba.shape[0], float(eps), out)
    return out


def transfer_colors(cloud_pts: torch.Tensor, cloud_rgb, verts: torch.Tensor, k: int = 8):
    """(rgba uint8 [m,4], nearest_d2 f32 [m]) on the device for verts f32 [m,3] against the cloud f32 [n,3] with colours uint8 [n,3] (alpha 255)
    or [n,4], a device tensor or a host array that is uploaded.  min(k, n) neighbours; k = 1 is nearest-point transfer.  nearest_d2 is the
    squared distance to the nearest cloud point, for a later trim by support."""
    dev = _lib.need_device('transfer_colors', cloud_pts, verts)
    if not 1 <= int(k) <= MAX_K:
        raise ValueError('k must be in 1..{}, got {}'.format(MAX_K, k))
    assert cloud_pts.dim() == 2 and cloud_pts.shape[1] == 3 and verts.dim() == 2 and verts.shape[1] == 3
    n, m = int(cloud_pts.shape[0]), int(verts.shape[0])
    if n == 0:
        raise ValueError('transfer_colors: the cloud has no points')
    if not torch.is_tensor(cloud_rgb):
        cloud_rgb = torch.from_numpy(np.array(cloud_rgb, dtype=np.uint8)).to(dev)          # (a copy: from_numpy wants a writable array)
    _lib.need_device('transfer_colors', cloud_pts, cloud_rgb)
    if cloud_rgb.dtype != torch.uint8 or cloud_rgb.dim() != 2 or cloud_rgb.shape[0] != n or cloud_rgb.shape[1] not in (3, 4):
        raise ValueError('transfer_colors: colours must be uint8 [{}, 3 or 4], got {} {}'.format(n, cloud_rgb.dtype, tuple(cloud_rgb.shape)))
    if cloud_rgb.shape[1] == 3:
        cloud_rgb = torch.cat([cloud_rgb, torch.full((n, 1), 255, dtype=torch.uint8, device=dev)], dim=1)
    if m == 0:
        return torch.empty((0, 4), dtype=torch.uint8, device=dev), torch.empty((0,), dtype=torch.float32, device=dev)
    idx, d2 = ops.KnnBlocks(cloud_pts).query(verts, min(int(k), n), return_d2=True)
    return blend_rgba(idx, d2, cloud_rgb), d2[:, 0].contiguous()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.transfer', description='Colour a mesh from the point colours of a scan (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh in the scan\'s frame')
    ap.add_argument('scan', help='coloured scan: .ply, .las, .pcd, .off or .obj')
    ap.add_argument('out_file', help='coloured PLY mesh')
    ap.add_argument('--k', type=int, default=8, help='neighbours blended per vertex (1: nearest point)')
    args = ap.parse_args(argv)
    if not 1 <= args.k <= MAX_K:
        raise SystemExit('--k must be in 1..{}'.format(MAX_K))
    _lib.need_gpu('python -m ppsurf_amd.transfer')
    rgb = meshio.load_pts_colors(args.scan)
    if rgb is None:
        raise SystemExit('{} carries no colours'.format(args.scan))
    pts = np.asarray(meshio.load_pts(args.scan))[:, :3].astype(np.float64)
    finite = np.isfinite(pts).all(axis=1)
    pts, rgb = pts[finite], rgb[finite]                           # non-finite rows leave together with their colours
    if pts.shape[0] == 0:
        raise SystemExit('{} has no finite point'.format(args.scan))
    verts, faces, _, double = meshio.read_mesh_file(args.mesh)      # the mesh's own colours are not looked at
    centre = meshio.box_centre(pts)                                # both on the scan's box
    dev = torch.device('cuda')
    cloud = torch.from_numpy(meshio.centred_f32(pts, centre)).to(dev)
    local = torch.from_numpy(meshio.centred_f32(verts, centre)).to(dev)
    rgba, d2 = transfer_colors(cloud, rgb, local, k=args.k)
    meshio.write_ply_mesh(args.out_file, verts, faces, double=double, colors_u8=rgba.cpu().numpy())
    dist = np.sqrt(d2.cpu().numpy().astype(np.float64))
    report = {'vertices': int(verts.shape[0]), 'points': int(pts.shape[0]), 'k': min(args.k, int(pts.shape[0])),
              'mean_nearest': float(dist.mean()) if dist.size else None, 'max_nearest': float(dist.max()) if dist.size else None}
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main(sys.argv[1:])
