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
import os
import sys

import numpy as np
import torch

from . import _lib, meshio

MAX_ITERS = 1000
MAX_VERTICES = 2 ** 31 - 1
_SENTINEL = 2 ** 63 - 1


class CpuTensorError(_lib.PpsError, ValueError):
    """CPU tensors given to smooth_mesh: the PpsError of every module's device guard, and a ValueError like its other argument errors."""


def _checked_params(iters, lam, mu):
    """(iters int, lam float, mu float) or a ValueError: iters an integer in 0..1000, lam finite in (0, 1], mu finite and 0 or < -lam."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= int(iters) <= MAX_ITERS:
        raise ValueError('iters must be an integer in 0..{}, got {!r}'.format(MAX_ITERS, iters))
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError('lam must be a finite number in (0, 1], got {}'.format(lam))
    if not (math.isfinite(mu) and (mu == 0.0 or mu < -lam)):
        raise ValueError('mu must be 0 (plain Laplacian smoothing) or a finite number < -lam = {}, got {}'.format(-lam, mu))
    return int(iters), lam, mu


def _half_edges(faces, nv):
    """Sorted keys int64 [6 nf] of ppsx_smooth_half_edges: (src << 32) | dst, the six keys of an invalid face last."""
    nf = int(faces.shape[0])
    keys = torch.empty(6 * nf, dtype=torch.int64, device=faces.device)
    _lib.call('ppsx_smooth_half_edges', faces, nf, nv, keys)
    return torch.sort(keys)[0]


def _adjacency(keys, nv):
    uniq, counts = torch.unique_consecutive(keys, return_counts=True)
    live = uniq != _SENTINEL
    uniq, counts = uniq[live], counts[live]
    offsets = torch.zeros(nv + 1, dtype=torch.int64, device=keys.device)
    offsets[1:] = torch.cumsum(torch.bincount(uniq >> 32, minlength=nv), 0)
    return offsets, (uniq & 0xFFFFFFFF).to(torch.int32), counts.to(torch.int32)


def mesh_adjacency(faces: torch.Tensor, nv: int):
    """(offsets int64 [nv + 1], nbr int32 [ne], mult int32 [ne]) on the device: row i lists the distinct vertices that share a valid face
    with vertex i, ascending, and the number of valid faces on each of those edges.  A face is valid when its indices lie in [0, nv) and
    are pairwise distinct.  One key per half-edge from the kernel, one sort, the distinct keys with their counts (not pps_csr: its rank step
    is quadratic in a crowded row, and a fan vertex of a simplified mesh is such a row).  Does not depend on the order of the faces."""
    _lib.need_device('mesh_adjacency', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_VERTICES:
        raise ValueError('nv must be in 0..2^31 - 1, got {}'.format(nv))
    return _adjacency(_half_edges(faces.contiguous(), int(nv)), int(nv))


def smooth_mesh(verts: torch.Tensor, faces: torch.Tensor, iters: int, lam: float = 0.5, mu: float = -0.53):
    """(verts f32 [nv,3], faces, info): `iters` iterations of pass(lam), pass(mu) over the device mesh verts f32 [nv,3] / faces int64 [nf,3].
    The state is fp64 from the widened input to one rounding after the last pass; the passes ping-pong two buffers.  The faces are returned
    as given.  info: vertices, faces_valid, border_vertices, moved_vertices (rows whose bytes changed), iters, lam, mu.  ValueError: iters no
    integer in 0..1000, lam not finite in (0, 1], mu neither 0 nor finite < -lam, non-finite vertices, CPU tensors (CpuTensorError)."""
    iters, lam, mu = _checked_params(iters, lam, mu)
    try:
        _lib.need_device('smooth_mesh', verts, faces)
    except _lib.PpsError as e:
        raise CpuTensorError(str(e)) from None
    assert verts.dim() == 2 and verts.shape[1] == 3 and faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    v = verts.contiguous().float()
    if not bool(torch.isfinite(v).all()):
        raise ValueError('smooth_mesh: the mesh has non-finite vertices')
    nv = int(v.shape[0])
    keys = _half_edges(faces.contiguous(), nv)
    offsets, nbr, mult = _adjacency(keys, nv)
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
    info = {'vertices': nv, 'faces_valid': int((keys != _SENTINEL).sum().item()) // 6,
            'border_vertices': int(torch.unique(src[mult == 1]).shape[0]),
            'moved_vertices': int((out.view(torch.int32) != v.view(torch.int32)).any(dim=1).sum().item()), 'iters': iters, 'lam': lam, 'mu': mu}
    return out, faces, info


def main(argv=None):
    import argparse
    from .transfer import _ply_stores_doubles
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
    if os.path.splitext(args.out_file)[1].lower() != '.ply':
        ap.error('the output is a .ply file')
    if not torch.cuda.is_available():
        raise _lib.PpsError('python -m ppsurf_amd.smooth runs on the GPU only; there is no CPU fallback')
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
    out_v, _, info = smooth_mesh(local, torch.from_numpy(np.asarray(faces, dtype=np.int64).reshape(-1, 3)).to(dev), iters, lam, mu)
    out_v = out_v.cpu().numpy().astype(np.float64) + centre[None]
    if colors is not None:
        meshio.write_ply_mesh_colored(args.out_file, out_v, faces, colors, double=double)
    else:
        meshio.write_ply_mesh(args.out_file, out_v, faces, double=double)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
