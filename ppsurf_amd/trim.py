"""Trim by support on the GPU: faces of a reconstructed mesh that no point of the scan stands for are dropped (csrc/pps_trim.hip; DESIGN.md
section 15).

    python -m ppsurf_amd.trim MESH SCAN OUT.ply (--factor F | --dist D) [--spacing_k 8]

The occupancy network closes every surface: the back of a facade, the underside of a terrain tile.  The reference has no trim;
`pps.py rec` / `predict` reach this module through the models' `gen_trim_factor`.  A face is supported when some cloud point lies within the
radius r of the TRIANGLE (not merely of its corners): d2(p, triangle) <= r * r in fp64 on the float32 inputs.  That is a pure function of the
cloud, the mesh and r: no dependence on the cell grid, the table capacity, the launch shape or the order in which points are visited.
With `--factor` the radius is F times the cloud's spacing (`cloud_spacing`); `--dist` gives it in file units.
"""
import json
import sys

import numpy as np
import torch

from . import _lib, meshio, ops
from .cells import CellGrid, MAX_AXIS

MAX_SPACING_K = 255


def _f32_not_below(x):
    """The smallest float32 >= x (x > 0 finite float64)."""
    f = np.float32(x)
    return f if np.float64(f) >= np.float64(x) else np.nextafter(f, np.float32(np.inf))


class SupportGrid(CellGrid):
    """The cell lists of one float32 device cloud [n,3], n >= 1, for queries of radius <= the cell edge: per occupied cell the run of its
    points in `order`.  `capacity` is a test switch: results do not depend on it."""

    def __init__(self, pts: torch.Tensor, capacity=None):
        _lib.need_device('SupportGrid', pts)
        assert pts.dim() == 2 and pts.shape[1] == 3 and pts.shape[0] >= 1
        self.pts = pts.contiguous().float()
        self.n = int(self.pts.shape[0])
        super().__init__(self.pts, capacity)
        self.h = self.inv_h = self.order = self.offsets = None

    def edge_for(self, radius):
        """h = max(r, ext / (2^20 - 1)) as the float32 not below it: never below r, never more than 2^20 cells along an axis."""
        return _f32_not_below(max(float(radius), float(np.float64(self.ext) / np.float64(MAX_AXIS - 1))))

    def build(self, h):
        """Cell lists for the cell edge h: one insertion kernel writes every point's slot, a stable sort and ops.row_offsets make the lists."""
        self._scratch()
        self.h = np.float32(h)
        self.inv_h = np.float32(1.0) / self.h
        slot = torch.empty(self.n, dtype=torch.int64, device=self.device)
        _lib.call('ppsx_trim_cell_slots', self.pts, self.n, self._vec3(self.lo), self._vec3(self.hi), float(self.h), float(self.inv_h), self._table,
                  self.capacity, slot)
        self.order = torch.sort(slot, stable=True)[1].contiguous()
        self.offsets = ops.row_offsets(slot, self.capacity)
        return self

    def support(self, verts: torch.Tensor, faces: torch.Tensor, radius: float) -> torch.Tensor:
        """uint8 [nf] of ppsx_trim_face_support against the lists of `build`."""
        out = torch.empty(faces.shape[0], dtype=torch.uint8, device=self.device)
        _lib.call('ppsx_trim_face_support', verts, verts.shape[0], faces, faces.shape[0], self.pts, self.n, self._vec3(self.lo), self._vec3(self.hi),
                  float(self.h), float(self.inv_h), self._table, self.capacity, self.order, self.offsets, float(radius), out)
        return out


def _radius(radius):
    r = float(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError('the radius must be a finite number > 0, got {}'.format(radius))
    return r


def _checked_cloud(what, cloud):
    assert cloud.dim() == 2 and cloud.shape[1] == 3
    if cloud.shape[0] == 0:
        raise ValueError('{}: the cloud has no points'.format(what))
    cloud = cloud.contiguous().float()
    if not bool(torch.isfinite(cloud).all()):
        raise ValueError('{}: the cloud has non-finite coordinates'.format(what))
    return cloud


def cloud_spacing(cloud: torch.Tensor, k: int = 8) -> float:
    """sqrt(float64(m)), m the lower median (rank (n - 1) // 2 in ascending order) of the float32 squared distances of every point of the
    device cloud f32 [n,3] to its k-th nearest other point: column k of the exact (k + 1)-NN search of the cloud in itself."""
    _lib.need_device('cloud_spacing', cloud)
    if not 1 <= int(k) <= MAX_SPACING_K:
        raise ValueError('spacing_k must be in 1..{}, got {}'.format(MAX_SPACING_K, k))
    n, k = int(cloud.shape[0]), int(k)
    if n <= k:
        raise ValueError('cloud_spacing needs more than k = {} points, got {}'.format(k, n))
    cloud = cloud.contiguous().float()
    _, d2 = ops.KnnBlocks(cloud).query(cloud, k + 1, return_d2=True)
    m = torch.kthvalue(d2[:, k].contiguous(), (n - 1) // 2 + 1)[0]
    return float(np.sqrt(np.float64(np.float32(m.item()))))


def face_support(cloud: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, radius: float, cell=None, capacity=None) -> torch.Tensor:
    """bool [nf] on the device: face f of verts f32 [nv,3] / faces int64 [nf,3] has a point of the cloud f32 [n,3] within `radius` of its
    triangle.  A face with an index outside [0, nv) or a non-finite corner is unsupported.  `cell` (a cell edge >= radius) and `capacity` (of
    the cell table) are test switches: results do not depend on them."""
    dev = _lib.need_device('face_support', cloud, verts, faces)
    r = _radius(radius)
    assert verts.dim() == 2 and verts.shape[1] == 3 and faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    nf = int(faces.shape[0])
    if nf == 0 or cloud.shape[0] == 0:
        return torch.zeros(nf, dtype=torch.bool, device=dev)
    grid = SupportGrid(_checked_cloud('face_support', cloud), capacity)
    h = grid.edge_for(r) if cell is None else _f32_not_below(cell)
    return grid.build(h).support(verts.contiguous().float(), faces.contiguous(), r).bool()


def _trim_rows(cloud, verts, faces, radius, min_component_faces):
    """(kept vertex rows int64 ascending, re-indexed faces, number of supported faces): the trim on row numbers, so that a caller can gather
    whatever it keeps per vertex."""
    from . import reconstruct
    keep = face_support(cloud, verts, faces, radius)
    rows = torch.arange(verts.shape[0], dtype=torch.int64, device=verts.device)
    rows, out_f = reconstruct.small_components_removed(rows, faces[keep], min_component_faces)
    return rows, out_f, int(keep.sum().item())


def trim_mesh(cloud: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, radius: float, min_component_faces=6, spacing=None):
    """(verts, faces, info) of the mesh without its unsupported faces: then reconstruct.small_components_removed drops the components of at
    most `min_component_faces` faces the cut left behind and the unreferenced vertices, order kept, faces re-indexed.  Device tensors in and
    out.  info: faces_in, faces_supported, faces_out, vertices_in, vertices_out, radius and spacing (what the caller derived the radius
    from, passed through).  An empty or non-finite cloud is a ValueError."""
    _lib.need_device('trim_mesh', cloud, verts, faces)
    r = _radius(radius)
    cloud = _checked_cloud('trim_mesh', cloud)
    rows, out_f, supported = _trim_rows(cloud, verts, faces, r, min_component_faces)
    info = {'faces_in': int(faces.shape[0]), 'faces_supported': supported, 'faces_out': int(out_f.shape[0]), 'vertices_in': int(verts.shape[0]),
            'vertices_out': int(rows.shape[0]), 'radius': r, 'spacing': None if spacing is None else float(spacing)}
    return verts[rows], out_f, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.trim', description='Drop the faces of a mesh that no point of a scan supports (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh in the scan\'s frame')
    ap.add_argument('scan', help='the scan: .ply, .las, .pcd, .off, .obj, .stl, .xyz, .npy')
    ap.add_argument('out_file', help='trimmed PLY mesh')
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument('--factor', type=float, default=None, help='radius = FACTOR x the spacing of the scan')
    how.add_argument('--dist', type=float, default=None, help='radius in file units')
    ap.add_argument('--spacing_k', type=int, default=8, help='the spacing is the median distance to the k-th nearest other point')
    args = ap.parse_args(argv)
    given = args.factor if args.factor is not None else args.dist
    if not (np.isfinite(given) and given > 0):
        ap.error('--factor / --dist must be a finite number > 0')
    if not 1 <= args.spacing_k <= MAX_SPACING_K:
        ap.error('--spacing_k must be in 1..{}'.format(MAX_SPACING_K))
    meshio.need_ply_output(ap, args.out_file)
    _lib.need_gpu('python -m ppsurf_amd.trim')
    pts = np.asarray(meshio.load_pts(args.scan))[:, :3].astype(np.float64)
    pts = pts[np.isfinite(pts).all(axis=1)]
    if pts.shape[0] == 0:
        raise SystemExit('{} has no finite point'.format(args.scan))
    verts, faces, colors, double = meshio.read_mesh_file(args.mesh)
    centre = meshio.box_centre(pts)                                # both on the scan's box
    dev = torch.device('cuda')
    cloud = torch.from_numpy(meshio.centred_f32(pts, centre)).to(dev)
    local = torch.from_numpy(meshio.centred_f32(verts, centre)).to(dev)
    spacing = None
    if args.factor is not None:
        if pts.shape[0] <= args.spacing_k:
            raise SystemExit('{} has {} finite points: --factor needs more than --spacing_k'.format(args.scan, pts.shape[0]))
        spacing = cloud_spacing(cloud, args.spacing_k)
        radius = float(np.float64(args.factor) * np.float64(spacing))
    else:
        radius = float(args.dist)
    # the vertices (and colours) are written as read: the trim works on row numbers, not on the float32 copies
    rows, out_f, supported = _trim_rows(cloud, local, torch.from_numpy(np.asarray(faces, dtype=np.int64)).to(dev), radius, 6)
    rows, out_f = rows.cpu().numpy(), out_f.cpu().numpy()
    meshio.write_ply_mesh(args.out_file, verts[rows], out_f, double=double, colors_u8=None if colors is None else np.asarray(colors)[rows])
    report = {'faces_in': int(np.asarray(faces).shape[0]), 'faces_supported': supported, 'faces_out': int(out_f.shape[0]),
              'vertices_in': int(verts.shape[0]), 'vertices_out': int(rows.shape[0]), 'points': int(pts.shape[0]), 'radius': radius,
              'spacing': spacing}
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main(sys.argv[1:])
