"""Taubin lambda|mu smoothing of a mesh on the GPU with a border rule (csrc/pps_smooth.hip).

    python -m ppsurf_amd.smooth MESH OUT.ply --iters N [--lam 0.5] [--mu -0.53]

The refined vertices carry the network's high-frequency error, and a trimmed border is a saw-tooth of voxel-sized steps.  The reference has
no smoothing; `pps.py rec` / `predict` reach this module through the models' `gen_smooth_iters`.  One iteration is a shrinking Jacobi pass
with factor `lam` and an inflating one with factor `mu` (Taubin 1995): every vertex moves by the factor towards the mean of its neighbours,
summed in fp64 in ascending neighbour order.  A border vertex (one with an edge that a single face holds) takes only its neighbours along
the border, so a cut relaxes along itself.  The result is a pure function of (verts, faces, iters, lam, mu); the topology is not changed.
"""
import json
import math
import sys

import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError, mesh_adjacency  # noqa: F401  (their home is topology.py; the names stay importable from here)

MAX_ITERS = 1000


def _checked_params(iters, lam, mu):
    """(iters int, lam float, mu float) or a ValueError: iters an integer in 0..1000, lam finite in (0, 1], mu finite and 0 or < -lam."""
    iters = params.integer('iters', iters, 0, MAX_ITERS)
    lam, mu = float(lam), float(mu)                                     # lam and mu stay loose: whatever float() takes
    if not (math.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError('lam must be a finite number in (0, 1], got {}'.format(lam))
    if not (math.isfinite(mu) and (mu == 0.0 or mu < -lam)):
        raise ValueError('mu must be 0 (plain Laplacian smoothing) or a finite number < -lam = {}, got {}'.format(-lam, mu))
    return iters, lam, mu


def smooth_mesh(verts: torch.Tensor, faces: torch.Tensor, iters: int, lam: float = 0.5, mu: float = -0.53):
    """(verts f32 [nv,3], faces, info): `iters` iterations of pass(lam), pass(mu) over the device mesh verts f32 [nv,3] / faces int64 [nf,3].
    The state is fp64 from the widened input to one rounding after the last pass; the passes ping-pong two buffers.  The faces are returned
    as given.  info: vertices, faces_valid, border_vertices, moved_vertices (rows whose bytes changed), iters, lam, mu.  ValueError: iters no
    integer in 0..1000, lam not finite in (0, 1], mu neither 0 nor finite < -lam, non-finite vertices, CPU tensors (CpuTensorError)."""
    iters, lam, mu = _checked_params(iters, lam, mu)
    topology.need_device('smooth_mesh', verts, faces)
    v, f = topology.checked_mesh('smooth_mesh', verts, faces)
    nv = int(v.shape[0])
    offsets, nbr, mult, valid = topology.adjacency_rows(f, nv)
    ne = int(nbr.shape[0])
    out = v
    if iters > 0 and nv > 0:
        x, y = v.double(), torch.empty(nv, 3, dtype=torch.float64, device=v.device)
        for _ in range(iters):
            for s in (lam, mu):
                _lib.call('ppsx_smooth_pass', x, nv, offsets, nbr, mult, ne, s, y)
                x, y = y, x
        out = x.float()
    src = torch.repeat_interleave(torch.arange(nv, dtype=torch.int64, device=v.device), offsets[1:] - offsets[:-1])
    info = {'vertices': nv, 'faces_valid': valid,
            'border_vertices': int(torch.unique(src[mult == 1]).shape[0]),
            'moved_vertices': int((out.view(torch.int32) != v.view(torch.int32)).any(dim=1).sum().item()), 'iters': iters, 'lam': lam, 'mu': mu}
    return out, faces, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.smooth', description='Smooth a mesh with Taubin\'s lambda|mu filter (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='smoothed PLY mesh')
    ap.add_argument('--iters', type=int, required=True, help='iterations, each a pass with --lam and a pass with --mu')
    ap.add_argument('--lam', type=float, default=0.5, help='shrinking factor in (0, 1]')
    ap.add_argument('--mu', type=float, default=-0.53, help='inflating factor < -lam, or 0 for plain Laplacian smoothing')
    args = ap.parse_args(argv)
    try:
        iters, lam, mu = _checked_params(args.iters, args.lam, args.mu)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.smooth')
    out_v, _, info = smooth_mesh(*mesh.to_device(), iters, lam, mu)
    mesh.write_moved(args.out_file, out_v)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
