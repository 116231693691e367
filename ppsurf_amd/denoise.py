"""Feature-preserving denoising of a mesh on the GPU: face-normal filtering, then a vertex update (csrc/pps_denoise.hip).

    python -m ppsurf_amd.denoise MESH OUT.ply [--threshold 0.5] [--normal_iters 5] [--vertex_iters 10]

Taubin's filter (smooth.py) is isotropic and rounds off every crease; CAD shapes are mostly creases.  This is the two-step filter of Sun,
Rosin, Martin and Langbein (TVCG 2007), the one MeshLab and CGAL ship for that case: every face normal becomes the normalised sum of the
normals of the faces that share a vertex with it, each weighted by (n_i . n_j - threshold)^2 and left out when the dot product does not
exceed the threshold, so a normal across a crease has no say; then every vertex moves along the filtered normals of its faces towards
their planes.  All sums run in fp64 in ascending face index.  The result is a pure function of (verts, faces, threshold, normal_iters,
vertex_iters); the topology is not changed.  The reference has no denoising, and the models have no switch for this stage: run the command
on the PLY that `pps.py rec` wrote.  The defaults come from the paper's range for CAD-like shapes and are not tuned on network output.
"""
import json
import math
import sys

import numpy as np
import torch

from . import _lib, mesh_cli, meshio, params, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_ITERS = 1000


def _checked_iters(name, value):
    return params.integer(name, value, 0, MAX_ITERS)


def _checked_threshold(threshold):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError('threshold must be a number in [0, 1), got {!r}'.format(threshold))
    threshold = float(threshold)
    if not (math.isfinite(threshold) and 0.0 <= threshold < 1.0):
        raise ValueError('threshold must be a finite number in [0, 1), got {}'.format(threshold))
    return threshold


def _checked_params(threshold, normal_iters, vertex_iters):
    """(threshold float, normal_iters int, vertex_iters int) or a ValueError: threshold finite in [0, 1), both counts integers in 0..1000."""
    return _checked_threshold(threshold), _checked_iters('normal_iters', normal_iters), _checked_iters('vertex_iters', vertex_iters)


def _filtered_normals(v, f, offsets, inc, threshold, normal_iters):
    """(filtered normals f64 [nf,3], valid faces whose first normal is zero) of a checked device mesh and its incidence rows."""
    nv, nf, ni = int(v.shape[0]), int(f.shape[0]), int(inc.shape[0])
    n = torch.empty(nf, 3, dtype=torch.float64, device=v.device)          # the kernels write every row
    _lib.call('ppsx_denoise_face_normals', v, nv, f, nf, n)
    degenerate = ni // 3 - int((n != 0).any(dim=1).sum().item())          # an invalid face has a zero normal and no corner in the rows
    if normal_iters > 0 and nf > 0:
        m = torch.empty_like(n)
        for _ in range(normal_iters):
            _lib.call('ppsx_denoise_filter_pass', f, nf, nv, offsets, inc, ni, n, threshold, m)
            n, m = m, n
    return n, degenerate


def filtered_face_normals(verts: torch.Tensor, faces: torch.Tensor, threshold: float = 0.5, normal_iters: int = 5) -> torch.Tensor:
    """f64 [nf,3]: the unit normals of the faces of the device mesh verts f32 [nv,3] / faces int64 [nf,3] after `normal_iters` passes of the
    filter (0: the plain face normals); zeros for an invalid face and for one without area.  The first stage of `denoise_mesh` on its own.
    ValueError as there."""
    threshold, normal_iters = _checked_threshold(threshold), _checked_iters('normal_iters', normal_iters)
    topology.need_device('filtered_face_normals', verts, faces)
    v, f = topology.checked_mesh('filtered_face_normals', verts, faces, limit=True)
    offsets, inc, _ = topology.incidence_rows(f, int(v.shape[0]))
    return _filtered_normals(v, f, offsets, inc, threshold, normal_iters)[0]


def denoise_mesh(verts: torch.Tensor, faces: torch.Tensor, threshold: float = 0.5, normal_iters: int = 5, vertex_iters: int = 10):
    """(verts f32 [nv,3], faces, info): `normal_iters` passes of the face-normal filter with `threshold`, then `vertex_iters` passes of the
    vertex update with those normals, over the device mesh verts f32 [nv,3] / faces int64 [nf,3].  The state is fp64 from the widened input
    to one rounding after the last pass; the passes ping-pong two buffers.  The faces are returned as given, an empty mesh comes back as
    given, and with vertex_iters = 0 the input bytes come back.  info: vertices, faces_valid, degenerate_faces (valid faces whose first
    normal is zero), moved_vertices (rows whose bytes changed), threshold, normal_iters, vertex_iters.  ValueError: threshold not finite in
    [0, 1), a count that is no integer in 0..1000, non-finite vertices, more than 2^31 - 1 vertices or faces, CPU tensors (CpuTensorError)."""
    threshold, normal_iters, vertex_iters = _checked_params(threshold, normal_iters, vertex_iters)
    topology.need_device('denoise_mesh', verts, faces)
    v, f = topology.checked_mesh('denoise_mesh', verts, faces, limit=True)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    offsets, inc, valid = topology.incidence_rows(f, nv)
    n, degenerate = _filtered_normals(v, f, offsets, inc, threshold, normal_iters)
    out = v
    if vertex_iters > 0 and nv > 0 and nf > 0:
        x, y = v.double(), torch.empty(nv, 3, dtype=torch.float64, device=v.device)
        for _ in range(vertex_iters):
            _lib.call('ppsx_denoise_vertex_pass', x, nv, f, nf, n, offsets, inc, int(inc.shape[0]), y)
            x, y = y, x
        out = x.float()
    info = {'vertices': nv, 'faces_valid': valid, 'degenerate_faces': degenerate,
            'moved_vertices': int((out.view(torch.int32) != v.view(torch.int32)).any(dim=1).sum().item()),
            'threshold': threshold, 'normal_iters': normal_iters, 'vertex_iters': vertex_iters}
    return out, faces, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.denoise',
                                 description='Denoise a mesh and keep its sharp edges: face-normal filtering, then a vertex update (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='denoised PLY mesh')
    ap.add_argument('--threshold', type=float, default=0.5, help='faces whose normals have a dot product <= this have no say; in [0, 1)')
    ap.add_argument('--normal_iters', type=int, default=5, help='passes of the face-normal filter')
    ap.add_argument('--vertex_iters', type=int, default=10, help='passes of the vertex update')
    args = ap.parse_args(argv)
    try:
        threshold, normal_iters, vertex_iters = _checked_params(args.threshold, args.normal_iters, args.vertex_iters)
    except ValueError as e:
        ap.error(str(e))
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.denoise')
    out_v, _, info = denoise_mesh(*mesh.to_device(), threshold, normal_iters, vertex_iters)
    mesh.write_moved(args.out_file, out_v)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
