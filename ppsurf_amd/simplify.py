"""Mesh simplification to a face budget on the GPU: Lindstrom's quadric vertex clustering (csrc/pps_simplify.hip).

    python -m ppsurf_amd.simplify IN OUT [--max_faces N | --voxel_size H] [--placement quadric|mean]

The reference writes its Marching Cubes mesh at the grid's own density and has no decimation; `pps.py rec` / `predict` reach this module through
the models' `gen_max_faces`.

  1. a grid of G cells along the longest box edge (h = ext / G in fp64) or of step `voxel_size`; every occupied cell becomes one output
     vertex, cells are numbered by their lowest vertex index;
  2. a face survives when its three corners lie in three different cells; `max_faces` bisects the integer G in [1, 2^20] with 20 counting
     passes for the finest grid whose survivor count is within the budget (the count is taken before duplicate removal: an upper bound);
  3. the vertex of a cell minimises the sum of the squared, area^2-weighted distances to the planes of the faces that touch the cell, with a
     Tikhonov pull of 1e-3 of the trace towards the mean of the cell's vertices; it falls back to that mean where the optimum leaves the cell;
  4. faces are remapped, collapsed and duplicate ones (same unordered triple, first kept) are dropped, then unreferenced vertices.
The result is a pure function of the mesh and G: integer atomics only, fixed order of the fp64 operations.
"""
import json
import os
import sys

import numpy as np
import torch

from . import _lib, meshio, ops, topology
from .cells import CellGrid

PLACEMENTS = ('quadric', 'mean')


def _cross(u, w):
    """u x w with every product and difference a rounding of its own (torch.cross may contract)."""
    return torch.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], dim=1)


class ClusterGrid(CellGrid):
    """The clustering of one device mesh (verts f64 [nv,3], faces int64 [nf,3]): the cell grid, counting pass and the simplification itself."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor, capacity=None):
        _lib.need_device('ClusterGrid', verts, faces)
        assert verts.dim() == 2 and verts.shape[1] == 3 and verts.shape[0] >= 1 and faces.dim() == 2 and faces.shape[1] == 3
        self.verts = verts.to(torch.float64).contiguous()
        self.faces = faces.to(torch.int64).contiguous()
        self.nv, self.nf = int(self.verts.shape[0]), int(self.faces.shape[0])
        if not bool(torch.isfinite(self.verts).all()):
            raise ValueError('simplification needs finite vertices')
        if self.nf and (int(self.faces.min()) < 0 or int(self.faces.max()) >= self.nv):
            raise ValueError('face index outside the vertices')
        super().__init__(self.verts, capacity)
        self._leader = torch.empty(self.nv, dtype=torch.int64, device=self.device)

    def _scratch(self):
        super()._scratch(best=True)

    def leaders_rc(self, h, inv_h, unchecked=True):
        """(status, leader int64 [nv] (device, reused by the next call), occupied cells) of pps_simplify_leaders."""
        self._scratch()
        rc = _lib.call('pps_simplify_leaders', self.verts, self.nv, self._vec3(self.lo), self._vec3(self.hi), float(h), float(inv_h), self._table,
                       self._best, self.capacity, self._leader, self._count, unchecked=unchecked)
        return rc, self._leader, (int(self._count.item()) if rc == 0 else -1)

    def leaders(self, h, inv_h=None):
        return self.leaders_rc(h, self._inv(h, inv_h), unchecked=False)[1:]

    def survivors(self, leader):
        _lib.call('pps_simplify_count', self.faces, self.nf, leader, self.nv, self._count)
        return int(self._count.item())

    def count_step(self, h, inv_h=None):
        """Faces whose corners lie in three different cells of the grid of step h (before duplicate removal)."""
        if self.nf == 0 or not self.ext > 0:
            return 0
        return self.survivors(self.leaders(h, inv_h)[0])

    def count(self, G):
        return self.count_step(*self.step(G)) if self.ext > 0 else 0

    count_at = count

    def run(self, G=None, placement='quadric', h=None, keep=False):
        """Simplify on the grid of G cells along the longest edge (or of step h) -> (verts f64 [V,3], faces int64 [F,3], report).  keep=True adds
        the intermediate device arrays to the report under '_debug' (tests)."""
        if placement not in PLACEMENTS:
            raise ValueError('placement must be one of {}'.format(PLACEMENTS))
        if (G is None) == (h is None):
            raise ValueError('give G or h')
        dev = self.verts.device
        report = {'faces_in': self.nf, 'verts_in': self.nv, 'G': None if G is None else int(G), 'h': None, 'cells': 0, 'survivors': 0,
                  'faces_out': 0, 'verts_out': 0, 'fallback': 0, 'flipped': 0}
        empty = (torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev))
        if not self.ext > 0:                                       # one position: h = 0 never reaches a kernel, no face can survive
            report['cells'] = 1
            return empty + (report,)
        if h is None:
            h, inv_h = self.step(int(G))
        else:
            h = np.float64(h)
            inv_h = np.float64(1.0) / h
        report['h'] = float(h)
        leader, ncell = self.leaders(h, inv_h)
        report['cells'] = ncell
        report['survivors'] = self.survivors(leader) if self.nf else 0
        if report['survivors'] == 0:
            return empty + (report,)
        flag = leader == torch.arange(self.nv, dtype=torch.int64, device=dev)
        cid = (torch.cumsum(flag, 0) - 1)[leader].contiguous()                  # rank of the cell's leader among the leaders
        corner_ids = cid[self.faces.reshape(-1)].contiguous()
        c_order, c_off = ops.csr_build(corner_ids, ncell)
        v_order, v_off = ops.csr_build(cid, ncell)
        A = torch.empty((ncell, 6), dtype=torch.float64, device=dev)
        b, xhat, pos = (torch.empty((ncell, 3), dtype=torch.float64, device=dev) for _ in range(3))
        fell = torch.empty(ncell, dtype=torch.uint8, device=dev)
        _lib.call('pps_simplify_place', self.verts, self.nv, self.faces, self.nf, cid, ncell, c_order, c_off, v_order, v_off, self._vec3(self.lo),
                  self._vec3(self.hi), float(h), float(inv_h), 1 if placement == 'mean' else 0, A, b, xhat, pos, fell)
        new = corner_ids.reshape(-1, 3)
        alive = (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 0] != new[:, 2])
        src = torch.nonzero(alive).reshape(-1)                                  # input face of every survivor
        new = new[src]
        srt = torch.sort(new, dim=1)[0]
        if ncell < 2_000_000:
            _, finv = torch.unique((srt[:, 0] * ncell + srt[:, 1]) * ncell + srt[:, 2], return_inverse=True)
        else:
            _, finv = torch.unique(srt, dim=0, return_inverse=True)
        first = torch.full((int(finv.max()) + 1,), new.shape[0], dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, finv, torch.arange(new.shape[0], device=dev), reduce='amin')
        first = torch.sort(first)[0]                                            # first face of every unordered triple, input order kept
        new, src = new[first], src[first]
        old = self.verts[self.faces[src]]
        n_old = _cross(old[:, 1] - old[:, 0], old[:, 2] - old[:, 0])
        moved = pos[new]
        n_new = _cross(moved[:, 1] - moved[:, 0], moved[:, 2] - moved[:, 0])
        dot = (n_old[:, 0] * n_new[:, 0] + n_old[:, 1] * n_new[:, 1]) + n_old[:, 2] * n_new[:, 2]
        used, remap = topology.used_rows(new, ncell)
        out_v, out_f = pos[used], remap[new]
        report.update(faces_out=int(out_f.shape[0]), verts_out=int(out_v.shape[0]), fallback=int(fell.sum()), flipped=int((~(dot > 0)).sum()))
        if keep:
            report['_debug'] = {'leader': leader.clone(), 'cid': cid, 'A': A, 'b': b, 'xhat': xhat, 'pos': pos, 'fallback': fell, 'used': used}
        return out_v, out_f, report


def simplify_mesh(verts, faces, max_faces=None, voxel_size=None, placement='quadric', device='cuda', _capacity=None):
    """(verts, faces, report) of the mesh simplified to at most `max_faces` faces, or on a grid of step `voxel_size`.

    verts [nv,3] / faces [nf,3]: device tensors (device tensors come back, vertices in the input's float type, faces int64) or host arrays
    (uploaded to `device`; numpy arrays come back).  A host tensor or a non-GPU `device` raises PpsError: there is no CPU implementation.  A mesh
    with nf <= max_faces is returned unchanged.  `_capacity` forces the size of the cell table (tests)."""
    if (max_faces is None) == (voxel_size is None):
        raise ValueError('max_faces and voxel_size exclude each other, and one of them is needed: a budget chooses its own grid')
    if max_faces is not None and int(max_faces) < 0:
        raise ValueError('max_faces must not be negative')
    if voxel_size is not None and not float(voxel_size) > 0:
        raise ValueError('voxel_size must be positive')
    if placement not in PLACEMENTS:
        raise ValueError('placement must be one of {}'.format(PLACEMENTS))
    host = not torch.is_tensor(verts)
    if host:
        if torch.is_tensor(faces):
            raise _lib.PpsError('simplify_mesh takes vertices and faces of one kind: device tensors or host arrays')
        _lib.need_gpu('simplify_mesh', device)
        v_in, f_in = np.asarray(verts), np.asarray(faces)
        if v_in.dtype.kind != 'f':
            v_in = v_in.astype(np.float64)
        dv = torch.from_numpy(np.ascontiguousarray(v_in)).to(device)
        df = torch.from_numpy(np.ascontiguousarray(f_in.astype(np.int64))).to(device)
    else:
        _lib.need_device('simplify_mesh', verts, faces)
        dv, df = verts, faces
    nv, nf = int(dv.shape[0]), int(df.shape[0])
    report = {'faces_in': nf, 'verts_in': nv, 'G': None, 'h': None, 'cells': None, 'survivors': nf, 'faces_out': nf, 'verts_out': nv,
              'fallback': 0, 'flipped': 0}
    if nv == 0 or (max_faces is not None and nf <= int(max_faces)):
        return verts, faces, report
    grid = ClusterGrid(dv, df, capacity=_capacity)
    if voxel_size is not None:
        out_v, out_f, report = grid.run(h=float(voxel_size), placement=placement)
    else:
        G = grid.search(int(max_faces))
        out_v, out_f, report = grid.run(G=G, placement=placement)
        if report['faces_out'] > int(max_faces):                   # only G = 1 is accepted without having been counted
            raise _lib.PpsError('max_faces={} is below the {} faces of the coarsest grid'.format(max_faces, report['faces_out']))
    out_v = out_v.to(dv.dtype)
    if host:
        return out_v.cpu().numpy(), out_f.cpu().numpy(), report
    return out_v, out_f, report


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.simplify', description='Simplify a triangle mesh by quadric vertex clustering (GPU).')
    ap.add_argument('in_file', help='.ply or .obj')
    ap.add_argument('out_file', help='.ply')
    ap.add_argument('--max_faces', type=int, default=None, help='face budget: the finest grid whose output stays within it')
    ap.add_argument('--voxel_size', type=float, default=None, help='explicit grid step in file units (replaces --max_faces)')
    ap.add_argument('--placement', choices=PLACEMENTS, default='quadric')
    args = ap.parse_args(argv)
    if (args.max_faces is None) == (args.voxel_size is None):
        ap.error('give exactly one of --max_faces and --voxel_size')
    if args.max_faces is not None and args.max_faces < 0:
        ap.error('--max_faces must not be negative')
    if args.voxel_size is not None and not args.voxel_size > 0:
        ap.error('--voxel_size must be positive')
    ext = os.path.splitext(args.in_file)[1].lower()
    if ext not in ('.ply', '.obj') or os.path.splitext(args.out_file)[1].lower() != '.ply':
        ap.error('reads .ply or .obj and writes .ply')
    verts, faces, _, double = meshio.read_mesh_file(args.in_file)
    out_v, out_f, report = simplify_mesh(verts, faces, max_faces=args.max_faces, voxel_size=args.voxel_size, placement=args.placement)
    meshio.write_ply_mesh(args.out_file, out_v, out_f, double=double)
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main(sys.argv[1:])
