"""Mesh queries on the GPU, the layer under evaluation, visualization and make_dataset: the face tables of a triangle mesh, area-weighted
surface samples, and the three brute-force queries of the triangle soup -- generalised winding number, exact closest point, first hit of a
ray.  Device tensors in, device tensors out; there is no CPU fallback.

The three queries are operations of one sliced face sweep (csrc/pps_sweep.h; the operations are in pps_eval.hip, pps_vis.hip and
pps_scan.hip); the sampler draws from the counter-based generator of csrc/pps_rng.h.
"""
import typing

import torch

from . import _lib


def _device():
    if not torch.cuda.is_available():
        raise _lib.PpsError('ppsurf_amd.geometry needs a GPU; there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


# ---- face tables and surface samples ------------------------------------------------------------------------------------------------------------
def face_stats(verts: torch.Tensor, faces: torch.Tensor):
    """verts f32 [nv,3], faces int32 [nf,3] on the device -> (area f32 [nf], unit normal f32 [nf,3], corners f32 [nf,9])."""
    _lib.need_device('geometry', verts, faces)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_contiguous() and faces.is_contiguous()
    nf = faces.shape[0]
    area = torch.empty(nf, dtype=torch.float32, device=verts.device)
    normal = torch.empty((nf, 3), dtype=torch.float32, device=verts.device)
    corners = torch.empty((nf, 9), dtype=torch.float32, device=verts.device)
    _lib.call('pps_eval_face_stats', verts, verts.shape[0], faces, nf, area, normal, corners)
    return area, normal, corners


def area_prefix(area: torch.Tensor) -> torch.Tensor:
    """fp64 inclusive prefix of the face areas (the sampler's face table)."""
    return torch.cumsum(area.to(torch.float64), 0)


def sample_surface(corners: torch.Tensor, prefix: torch.Tensor, n: int, seed: int = 0, stream_id: int = 0):
    """n area-weighted surface samples -> (points f32 [n,3], face ids int32 [n]).  prefix = area_prefix(area), its last entry > 0."""
    _lib.need_device('geometry', corners, prefix)
    assert corners.dtype == torch.float32 and prefix.dtype == torch.float64 and corners.is_contiguous() and prefix.is_contiguous()
    pts = torch.empty((n, 3), dtype=torch.float32, device=corners.device)
    face = torch.empty(n, dtype=torch.int32, device=corners.device)
    _lib.call('pps_eval_sample_surface', corners, prefix, corners.shape[0], int(n), int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), pts, face)
    return pts, face


# ---- the sliced face sweeps ---------------------------------------------------------------------------------------------------------------------
def _sweep(entry: str, planner: str, corners, items, part_dtypes, outputs, slices=None):
    """One two-pass query `entry(corners, nf, *items, m, slices, *partials, *outputs, stream)` of the m rows of `items` against the faces of
    corners: the slice count from `planner` unless forced, [slices, m] partials of `part_dtypes` for pass 1, call and check."""
    m, nf = items[0].shape[0], corners.shape[0]
    s = getattr(_lib.lib(), planner)(m, nf) if slices is None else int(slices)
    partials = [torch.empty((s, m), dtype=dt, device=items[0].device) for dt in part_dtypes]
    _lib.call(entry, corners, nf, *items, m, s, *partials, *outputs)


def winding_number(corners: torch.Tensor, query: torch.Tensor) -> torch.Tensor:
    """Generalised winding number f64 [m] of query f32 [m,3] with respect to the mesh of corners [nf,9] (0 for a mesh without faces).  The
    slice count is always the planner's: the fp32 partial sums depend on it."""
    _lib.need_device('geometry', corners, query)
    query = query.contiguous().float()
    w = torch.zeros(query.shape[0], dtype=torch.float64, device=query.device)
    if query.shape[0] > 0 and corners.shape[0] > 0:
        _sweep('pps_eval_winding', 'pps_eval_winding_slices', corners, [query], [torch.float32], [w])
    return w


def closest_point_on_corners(corners: torch.Tensor, query: torch.Tensor, slices: typing.Optional[int] = None):
    """Exact closest point on the triangle soup corners f32 [nf,9] (face_stats) of query [m,3], device tensors -> (closest points f32 [m,3],
    distances f32 [m], face ids int32 [m]), ties to the lowest face id.  `slices` forces the number of face slices (any value gives the same
    result; default pps_vis_closest_slices)."""
    _lib.need_device('geometry', corners, query)
    query = query.to(torch.float32).contiguous()
    m, dev = query.shape[0], query.device
    pt = torch.empty((m, 3), dtype=torch.float32, device=dev)
    d = torch.empty(m, dtype=torch.float32, device=dev)
    face = torch.empty(m, dtype=torch.int32, device=dev)
    if m > 0:
        _sweep('pps_vis_closest_point', 'pps_vis_closest_slices', corners, [query], [torch.float32, torch.int32], [d, face, pt], slices)
    return pt, d, face


def closest_point_on_mesh(verts: torch.Tensor, faces: torch.Tensor, query: torch.Tensor, slices: typing.Optional[int] = None):
    """closest_point_on_corners for a mesh (verts f32 [nv,3], faces int [nf,3]); a mesh without faces raises ValueError."""
    _lib.need_device('geometry', verts, faces, query)
    verts = verts.to(torch.float32).contiguous()
    faces = faces.to(torch.int32).contiguous()
    if faces.shape[0] == 0:
        raise ValueError('closest_point_on_mesh: the mesh has no faces')
    return closest_point_on_corners(face_stats(verts, faces)[2], query, slices)


def first_hit(corners: torch.Tensor, orig: torch.Tensor, dirs: torch.Tensor, slices: typing.Optional[int] = None):
    """First hit of the rays (orig, dirs f32 [m,3]) on the triangle soup corners f32 [nf,9], device tensors -> (t f64 [m], face int32 [m]),
    -1 for a miss.  `slices` forces the number of face slices (any value gives the same result; default pps_scan_hit_slices)."""
    _lib.need_device('geometry', corners, orig, dirs)
    orig, dirs = orig.to(torch.float32).contiguous(), dirs.to(torch.float32).contiguous()
    corners = corners.to(torch.float32).contiguous()
    m, dev = orig.shape[0], orig.device
    t = torch.full((m,), -1.0, dtype=torch.float64, device=dev)
    face = torch.full((m,), -1, dtype=torch.int32, device=dev)
    if m > 0 and corners.shape[0] > 0:
        _sweep('pps_scan_first_hit', 'pps_scan_hit_slices', corners, [orig, dirs], [torch.float64, torch.int32], [t, face], slices)
    return t, face
