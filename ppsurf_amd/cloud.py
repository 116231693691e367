"""Preparation of a raw scan before reconstruction: voxel-grid subsampling to a point budget and statistical outlier removal, on the GPU
(csrc/pps_cloud.hip).

    python -m ppsurf_amd.cloud IN OUT [--max_points 250000] [--voxel_size H] [--outlier_k 16] [--outlier_ratio 2.0]

The reference tells its users to sub-sample large clouds to ~250k points themselves (source/occupancy_data_module.py:183-184) and has no
outlier filter; `pps.py rec` / `predict` reach this module through the data modules' `max_points`, `voxel_size`, `outlier_k`, `outlier_ratio`.

Order of the stages (fixed):
  1. rows with a non-finite coordinate are dropped;
  2. the box centre is subtracted IN THE INPUT'S OWN TYPE and only then the cloud is cast to float32 (a geo-referenced cloud, UTM eastings
     around 5e5, must not meet float32 before it is centred);
  3. voxel stage: with `voxel_size` a grid of that step; with `max_points` the finest grid of G cells along the longest box edge,
     h = float32(ext / G), whose number of occupied cells is within the budget -- bisection of the integer G in [1, 2^20], 20 counting
     passes.  Every occupied cell keeps the one of its own points that is nearest to the cell centre.  A cloud of at most `max_points`
     points is kept whole; a cloud without extent keeps its first point;
  4. outlier stage on what stage 3 kept: mean distance m_i to the `outlier_k` nearest neighbours, kept when m_i <= mu + ratio * sigma.
     So kept <= max_points: the budget is an upper bound, not a target.
The result is the ascending list of kept ROWS OF THE INPUT and a report; it is a pure function of the input (no float atomics, no dependence
on launch shape or on the order in which threads reach the cell table).
"""
import json
import os
import sys

import numpy as np
import torch

from . import _lib, meshio, ops
from .cells import CellGrid


class VoxelGrid(CellGrid):
    """The voxel stage for one float32 device cloud [n,3]: the cell grid and the two entry points."""

    def __init__(self, pts: torch.Tensor, capacity=None):
        _lib.need_device('VoxelGrid', pts)
        assert pts.dim() == 2 and pts.shape[1] == 3 and pts.shape[0] >= 1
        self.pts = pts.contiguous().float()
        self.n = int(self.pts.shape[0])
        super().__init__(self.pts, capacity)

    def count_rc(self, h, inv_h, unchecked=True):
        """(status, number of occupied cells) of pps_cloud_voxel_count; the count is meaningless unless status == 0."""
        self._scratch()
        rc = _lib.call('pps_cloud_voxel_count', self.pts, self.n, self._vec3(self.lo), self._vec3(self.hi), float(h), float(inv_h), self._table,
                       self.capacity, self._count, unchecked=unchecked)
        return rc, (int(self._count.item()) if rc == 0 else -1)

    def count(self, h, inv_h=None):
        return self.count_rc(h, self._inv(h, inv_h), unchecked=False)[1]

    def count_at(self, G):
        return self.count(*self.step(G))

    def select(self, h, inv_h=None):
        """Ascending int64 indices (device) of the point kept by every occupied cell."""
        self._scratch(best=True)
        keep = torch.empty(self.n, dtype=torch.uint8, device=self.pts.device)
        _lib.call('pps_cloud_voxel_select', self.pts, self.n, self._vec3(self.lo), self._vec3(self.hi), float(h), float(self._inv(h, inv_h)),
                  self._table, self._best, self.capacity, self._count, keep)
        return torch.nonzero(keep).reshape(-1)


def mean_knn_distance(d2: torch.Tensor) -> torch.Tensor:
    """m f64 [n] of the squared (k+1)-NN distances d2 f32 [n, k+1] (ops.KnnBlocks.query(..., return_d2=True)); column 0 is dropped."""
    _lib.need_device('mean_knn_distance', d2)
    d2 = d2.contiguous()
    assert d2.dtype == torch.float32 and d2.dim() == 2 and d2.shape[1] >= 2
    m = torch.empty(d2.shape[0], dtype=torch.float64, device=d2.device)
    _lib.call('pps_cloud_mean_knn_dist', d2, d2.shape[0], d2.shape[1] - 1, m)
    return m


def outlier_stats(m: torch.Tensor, ratio: float) -> torch.Tensor:
    """f64 [3] on the device: mean, population standard deviation, mean + ratio * deviation of m, summed in a fixed order."""
    assert m.is_cuda and m.dtype == torch.float64 and m.is_contiguous() and m.shape[0] >= 1
    out = torch.empty(3, dtype=torch.float64, device=m.device)
    _lib.call('pps_cloud_outlier_stats', m, m.shape[0], float(ratio), out)
    return out


def outlier_keep(m: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    """Ascending int64 indices (device) of the points with m <= stats[2]."""
    keep = torch.empty(m.shape[0], dtype=torch.uint8, device=m.device)
    _lib.call('pps_cloud_outlier_keep', m, m.shape[0], stats, keep)
    return torch.nonzero(keep).reshape(-1)


def remove_outliers(pts: torch.Tensor, k: int, ratio: float):
    """Statistical outlier removal of a float32 device cloud -> (ascending kept indices, stats f64 [3] on the host or None).  n <= k keeps
    everything."""
    n = int(pts.shape[0])
    if n <= k:
        return torch.arange(n, dtype=torch.int64, device=pts.device), None
    _, d2 = ops.KnnBlocks(pts).query(pts, int(k) + 1, return_d2=True)
    m = mean_knn_distance(d2)
    stats = outlier_stats(m, ratio)
    return outlier_keep(m, stats), stats.cpu().numpy()


def prepare_cloud(pts, max_points=None, voxel_size=None, outlier_k=0, outlier_ratio=2.0, device='cuda', _capacity=None):
    """Indices (ascending int64 numpy array, rows of `pts`) of the points a reconstruction should use, and a report dictionary.

    pts: numpy array [n, >= 3] of any float type (the host path: centred in its own type, then uploaded to `device`) or a device tensor.
    A host tensor or a non-GPU `device` raises PpsError: there is no CPU implementation.  `_capacity` forces the size of the cell table (tests)."""
    if max_points is not None and voxel_size is not None:
        raise ValueError('max_points and voxel_size exclude each other: a budget chooses its own grid')
    if max_points is not None and int(max_points) < 1:
        raise ValueError('max_points must be positive')
    if voxel_size is not None and not float(voxel_size) > 0:
        raise ValueError('voxel_size must be positive')
    if torch.is_tensor(pts):
        _lib.need_device('prepare_cloud', pts)
        device = pts.device
        xyz = pts[:, :3]
        finite = torch.isfinite(xyz).all(dim=1)
        rows = torch.nonzero(finite).reshape(-1).cpu().numpy()
        xyz = xyz[finite]
        if xyz.shape[0] > 0:
            xyz = xyz - (xyz.min(dim=0)[0] + xyz.max(dim=0)[0]) * 0.5
        n_in = int(pts.shape[0])
    else:
        _lib.need_gpu('prepare_cloud', device)
        arr = np.asarray(pts)
        if arr.dtype.kind != 'f':
            arr = arr.astype(np.float64)
        xyz = arr[:, :3]
        finite = np.isfinite(xyz).all(axis=1)
        rows = np.nonzero(finite)[0]
        if rows.shape[0] < xyz.shape[0]:
            xyz = xyz[finite]
        if xyz.shape[0] > 0:
            xyz = xyz - (xyz.min(axis=0) + xyz.max(axis=0)) * xyz.dtype.type(0.5)
        n_in = int(arr.shape[0])
    report = {'rows': n_in, 'nonfinite_dropped': n_in - int(rows.shape[0]), 'G': None, 'h': None, 'kept_voxel': int(rows.shape[0]),
              'mu': None, 'sigma': None, 'threshold': None, 'removed_outliers': 0, 'kept': int(rows.shape[0])}
    if rows.shape[0] == 0:
        return rows.astype(np.int64), report
    dev_pts = (xyz if torch.is_tensor(xyz) else torch.from_numpy(np.ascontiguousarray(xyz.astype(np.float32))).to(device)).float().contiguous()
    n = int(dev_pts.shape[0])
    sel = None                                                   # None: everything
    if voxel_size is not None or (max_points is not None and n > int(max_points)):
        grid = VoxelGrid(dev_pts, capacity=_capacity)
        if not grid.ext > 0:                                     # one point, or all points equal: h = 0 never reaches a kernel
            sel = torch.zeros(1, dtype=torch.int64, device=dev_pts.device)
        else:
            if voxel_size is not None:
                h = np.float32(voxel_size)
                inv_h = np.float32(1.0) / h
            else:
                report['G'] = grid.search(int(max_points))
                h, inv_h = grid.step(report['G'])
            report['h'] = float(h)
            sel = grid.select(h, inv_h)
            if max_points is not None and sel.shape[0] > int(max_points):          # only G = 1 is accepted without having been counted
                raise _lib.PpsError('max_points={} is below the {} cells of the coarsest grid'.format(max_points, sel.shape[0]))
        report['kept_voxel'] = int(sel.shape[0])
    if outlier_k:
        sub = dev_pts if sel is None else dev_pts[sel]
        keep, stats = remove_outliers(sub, int(outlier_k), float(outlier_ratio))
        if stats is not None:
            report.update(mu=float(stats[0]), sigma=float(stats[1]), threshold=float(stats[2]), removed_outliers=int(sub.shape[0] - keep.shape[0]))
            sel = keep if sel is None else sel[keep]
    idx = rows if sel is None else rows[sel.cpu().numpy()]
    report['kept'] = int(idx.shape[0])
    return idx.astype(np.int64), report


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.cloud', description='Sub-sample a raw scan to a point budget and remove outliers (GPU).')
    ap.add_argument('in_file')
    ap.add_argument('out_file', help='.npy (all columns, dtype preserved) or .xyz.ply / .ply (float32 x y z)')
    ap.add_argument('--max_points', type=int, default=250000)
    ap.add_argument('--voxel_size', type=float, default=None, help='explicit grid step in file units (replaces --max_points)')
    ap.add_argument('--outlier_k', type=int, default=16, help='neighbours of the statistical filter, 0 switches it off')
    ap.add_argument('--outlier_ratio', type=float, default=2.0)
    args = ap.parse_args(argv)
    ext = os.path.splitext(args.out_file)[1].lower()
    if ext not in ('.npy', '.ply'):
        raise SystemExit('unknown output type {!r}: use .npy or .xyz.ply'.format(args.out_file))
    pts = meshio.load_pts(args.in_file)
    idx, report = prepare_cloud(pts, max_points=None if args.voxel_size is not None else args.max_points, voxel_size=args.voxel_size,
                                outlier_k=args.outlier_k, outlier_ratio=args.outlier_ratio)
    out = pts[idx]                                               # gathered from the ORIGINAL array: all columns, original type
    os.makedirs(os.path.dirname(os.path.abspath(args.out_file)), exist_ok=True)
    if ext == '.npy':
        np.save(args.out_file, out)
    else:
        meshio.write_ply_points(args.out_file, out[:, :3])
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main(sys.argv[1:])
