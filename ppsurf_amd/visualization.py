"""Distance-coloured meshes and renders on the GPU: the qualitative half of the comparison (source/base/visualization.py, proximity.py).

Replaces trimesh (subdivision, closest point, PLY export) and pyrender / pyglet (renders), which are not available and need an OpenGL
context.  The distances are geometry.closest_point_on_mesh (exact point-to-triangle closest point, ties to the lowest face id);
`render_scene` is a deterministic z-buffer rasteriser (64-bit atomicMin of depth bits and id per pixel) and a shading pass, both in
csrc/pps_vis.hip.

Camera of `render_scene` (the reference's `scene.set_camera(angles=(pi/4, pi/4, 0), distance=2.2, fov=(45, 45))`; trimesh is not
installed, so this definition is the specification):
  * c = centre of the axis-aligned bounding box of the vertices;
  * R = Rz(0) Ry(pi/4) Rx(pi/4) (static 'sxyz' Euler angles);
  * eye = c + R (0, 0, 2.2); the camera looks along -R z, its up vector is R y; world -> view is Rt (v - eye), view depth = -z_view;
  * vertical field of view 45 degrees, 1024 x 1024 pixels, focal length f = (H / 2) / tan(22.5 degrees) pixels, principal point at the
    image centre, y down (row 0 at the top).
Triangles with a vertex nearer than 0.01 are dropped; no back-face culling.  A mesh is grey (102, 102, 102) unless its PLY carries vertex
colours, shaded by 0.3 + 0.7 |n . v| (two-sided headlight).  A vertex-only PLY or a .npy renders as points: discs of radius 2 px at 1024^2
(scaled with the width), unshaded.  The background is white.  The PNG is written with zlib alone (8-bit RGB, one IDAT chunk).

Colour map: `distances_to_vertex_colors` indexes a 256-entry parula-like table built here by linear interpolation between eight anchor
colours sampled at equal steps along the published MATLAB parula map (dark blue at 0, yellow at 1; `PARULA_ANCHORS`).
"""
import math
import os
import struct
import typing
import zlib

import numpy as np
import torch

from . import _lib, meshio
from .geometry import _device, closest_point_on_mesh
from .meshio import call_necessary, load_mesh_any

NEAR = 0.01
RENDER_SIZE = 1024
GREY = (102, 102, 102)
POINT_RADIUS_PX = 2.0                       # at 1024 px width

# Anchor colours of the parula map at t = 0, 1/7, ..., 1 (sRGB in [0, 1], three decimals); linear interpolation between them.
PARULA_ANCHORS = np.array([
    [0.208, 0.166, 0.529],
    [0.012, 0.388, 0.882],
    [0.078, 0.522, 0.831],
    [0.024, 0.651, 0.753],
    [0.220, 0.725, 0.620],
    [0.592, 0.749, 0.439],
    [0.973, 0.729, 0.235],
    [0.976, 0.983, 0.054],
], dtype=np.float64)


def parula_table(levels: int = 256) -> np.ndarray:
    """uint8 [levels, 3]: PARULA_ANCHORS interpolated linearly at `levels` equally spaced positions, rounded to 0..255."""
    t = np.linspace(0.0, 1.0, levels)
    xs = np.linspace(0.0, 1.0, PARULA_ANCHORS.shape[0])
    rgb = np.stack([np.interp(t, xs, PARULA_ANCHORS[:, c]) for c in range(3)], axis=1)
    return np.rint(rgb * 255.0).astype(np.uint8)


PARULA = parula_table()


def distance_color_indices(dist_per_vertex, cut_off: float) -> np.ndarray:
    """int(min(d, cut_off) / cut_off * (L - 1)) clamped to L - 1, in fp32 as the reference computes it (visualization.py:66-78)."""
    d = np.array(dist_per_vertex, dtype=np.float32)
    d[d > cut_off] = cut_off
    d /= np.float32(cut_off)
    idx = (d * np.float32(PARULA.shape[0] - 1)).astype(np.int32)
    idx[idx >= PARULA.shape[0]] = PARULA.shape[0] - 1
    return idx


def distances_to_vertex_colors(dist_per_vertex, cut_off=0.3) -> np.ndarray:
    """uint8 [n,3] parula colours of the distances: 0 -> blue, cut_off / 2 -> green, >= cut_off -> yellow."""
    return PARULA[distance_color_indices(dist_per_vertex, cut_off)]


# ---- closest point ------------------------------------------------------------------------------------------------------------------------------
def get_closest_point_on_mesh(mesh, query_pts, batch_size=1000):
    """proximity.py:20 with numpy in and out: mesh = (verts [nv,3], faces [nf,3]) -> (closest points f32 [m,3], distances f32 [m],
    face ids int32 [m]).  batch_size is accepted and ignored (one launch)."""
    verts, faces = mesh
    dev = _device()
    v = torch.as_tensor(np.asarray(verts, dtype=np.float32), device=dev)
    f = torch.as_tensor(np.asarray(faces, dtype=np.int32), device=dev)
    q = torch.as_tensor(np.asarray(query_pts, dtype=np.float32), device=dev)
    pt, d, face = closest_point_on_mesh(v, f, q)
    return pt.cpu().numpy(), d.cpu().numpy(), face.cpu().numpy()


# ---- subdivision --------------------------------------------------------------------------------------------------------------------------------
def subdivide(verts: torch.Tensor, faces: torch.Tensor):
    """Midpoint subdivision (trimesh.remesh.subdivide's geometry): every face becomes four, one new vertex at the midpoint of every unique
    edge, the new vertices after the old ones (sorted by edge).  Runs on the tensors' device."""
    nv = verts.shape[0]
    f = faces.to(torch.int64)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], dim=0)
    lo, hi = torch.minimum(e[:, 0], e[:, 1]), torch.maximum(e[:, 0], e[:, 1])
    uniq, inv = torch.unique(lo * nv + hi, return_inverse=True)
    a, b = uniq // nv, uniq % nv
    mid = (verts[a] + verts[b]) * 0.5
    m = (inv + nv).view(3, -1)
    m01, m12, m20 = m[0], m[1], m[2]
    new_f = torch.cat([torch.stack([f[:, 0], m01, m20], 1), torch.stack([m01, f[:, 1], m12], 1), torch.stack([m20, m12, f[:, 2]], 1),
                       torch.stack([m01, m12, m20], 1)], dim=0)
    return torch.cat([verts, mid.to(verts.dtype)], dim=0), new_f.to(faces.dtype)


# ---- distance-coloured meshes -----------------------------------------------------------------------------------------------------------------
def visualize_chamfer_distance(input_mesh_file: str, reference_mesh_file: str, output_mesh_file: str, min_vertex_count: typing.Optional[int],
                               dist_cut_off=0.3, distance_batch_size=1000):
    """visualization.py:81-99: subdivide the input mesh until it has min_vertex_count vertices, colour every vertex by its exact distance
    to the reference mesh (parula, clipped at dist_cut_off) and write a vertex-coloured PLY.  distance_batch_size is ignored."""
    dev = _device()
    vi, fi = load_mesh_any(input_mesh_file)[:2]
    vr, fr = load_mesh_any(reference_mesh_file)[:2]
    v = torch.as_tensor(vi, device=dev)
    f = torch.as_tensor(fi, device=dev)
    if min_vertex_count is not None and f.shape[0] > 0:
        while v.shape[0] < min_vertex_count:
            v, f = subdivide(v, f)
    _, d, _ = closest_point_on_mesh(torch.as_tensor(vr, device=dev), torch.as_tensor(fr, device=dev), v)
    colors = distances_to_vertex_colors(d.cpu().numpy(), float(dist_cut_off))
    meshio.write_ply_mesh_colored(output_mesh_file, v.cpu().numpy(), f.cpu().numpy(), colors)


def visualize_chamfer_distance_pool(rec_meshes: typing.Sequence[str], gt_meshes: typing.Sequence[str], output_mesh_files: typing.Sequence[str],
                                    min_vertex_count=10000, dist_cut_off=0.3, distance_batch_size=1000, num_processes=0):
    """visualization.py:102-116 in one process (the work is on the GPU); pairs whose output is up to date or whose input is missing are
    skipped."""
    assert len(rec_meshes) == len(gt_meshes) == len(output_mesh_files)
    for rec, gt, out in zip(rec_meshes, gt_meshes, output_mesh_files):
        if call_necessary([rec, gt], out):
            visualize_chamfer_distance(rec, gt, out, min_vertex_count, dist_cut_off, distance_batch_size)


# ---- camera, rasteriser, PNG --------------------------------------------------------------------------------------------------------------------
def euler_sxyz(ai: float, aj: float, ak: float) -> np.ndarray:
    """Rotation matrix of static 'sxyz' Euler angles: Rz(ak) Ry(aj) Rx(ai)."""
    ca, sa, cb, sb, cc, sc = math.cos(ai), math.sin(ai), math.cos(aj), math.sin(aj), math.cos(ak), math.sin(ak)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], dtype=np.float64)
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], dtype=np.float64)
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]], dtype=np.float64)
    return rz @ ry @ rx


def camera(verts: np.ndarray, size: int = RENDER_SIZE, angles=(math.pi * 0.25, math.pi * 0.25, 0.0), distance: float = 2.2,
           fov_deg: float = 45.0):
    """(eye f64 [3], world -> view rotation f64 [3,3], focal length in pixels) of the module docstring's camera."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    c = 0.5 * (v.min(axis=0) + v.max(axis=0)) if v.shape[0] else np.zeros(3)
    R = euler_sxyz(*angles)
    eye = c + R @ np.array([0.0, 0.0, distance])
    focal = 0.5 * size / math.tan(math.radians(fov_deg) * 0.5)
    return eye, R.T, focal


def camera_array(eye, view_rot, focal) -> np.ndarray:
    """The 16 floats of the kernels' camera: world -> view rotation (row-major), eye, focal length, 3 unused."""
    cam = np.zeros(16, dtype=np.float32)
    cam[0:9] = np.asarray(view_rot, dtype=np.float64).reshape(9)
    cam[9:12] = eye
    cam[12] = focal
    return cam


def _clear_keys(h, w, dev):
    return torch.full((h, w), -1, dtype=torch.int64, device=dev)      # all ones: the background key


def raster_faces(verts: torch.Tensor, faces: torch.Tensor, cam: np.ndarray, width: int, height: int, keys: torch.Tensor = None) -> torch.Tensor:
    """Key buffer int64 [H,W] (bits of uint64 (depth bits << 32) | face id; -1 = empty) of the mesh on the device."""
    _lib.need_device('visualization', verts, faces)
    verts = verts.to(torch.float32).contiguous()
    faces = faces.to(torch.int32).contiguous()
    dev = verts.device
    keys = _clear_keys(height, width, dev) if keys is None else keys
    L = _lib.lib()
    ws_bytes = L.pps_vis_raster_ws_bytes(verts.shape[0], faces.shape[0])
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
    cam = np.ascontiguousarray(cam, dtype=np.float32)
    _lib.call('pps_vis_raster_faces', verts, verts.shape[0], faces, faces.shape[0], cam.ctypes.data, width, height, ws, ws_bytes, keys)
    return keys


def raster_points(pts: torch.Tensor, cam: np.ndarray, width: int, height: int, radius: float, keys: torch.Tensor = None) -> torch.Tensor:
    """Key buffer int64 [H,W] of points drawn as discs of `radius` pixels (key id = point index)."""
    _lib.need_device('visualization', pts)
    pts = pts.to(torch.float32).contiguous()
    keys = _clear_keys(height, width, pts.device) if keys is None else keys
    cam = np.ascontiguousarray(cam, dtype=np.float32)
    _lib.call('pps_vis_raster_points', pts, pts.shape[0], cam.ctypes.data, width, height, float(radius), keys)
    return keys


def shade(keys: torch.Tensor, verts: torch.Tensor, faces: typing.Optional[torch.Tensor], cam: np.ndarray, colors: torch.Tensor = None,
          rgb=GREY) -> torch.Tensor:
    """uint8 [H,W,3] image of a key buffer: faces given -> mesh shading, faces None -> points."""
    _lib.need_device('visualization', keys, verts)
    h, w = keys.shape
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=keys.device)
    verts = verts.to(torch.float32).contiguous()
    if faces is not None:
        faces = faces.to(torch.int32).contiguous()
    if colors is not None:
        colors = colors.to(torch.uint8).contiguous()
    packed = (int(rgb[0]) << 16) | (int(rgb[1]) << 8) | int(rgb[2])
    cam = np.ascontiguousarray(cam, dtype=np.float32)
    _lib.call('pps_vis_shade', keys, w, h, verts, faces, colors, packed, cam.ctypes.data, out)
    return out


def render(verts: np.ndarray, faces: np.ndarray, colors: typing.Optional[np.ndarray] = None, size: int = RENDER_SIZE) -> np.ndarray:
    """uint8 [size,size,3] image of a mesh (faces non-empty) or a point cloud (faces empty) with the module's camera."""
    dev = _device()
    cam = camera_array(*camera(verts, size))
    v = torch.as_tensor(np.asarray(verts, dtype=np.float32).reshape(-1, 3), device=dev)
    c = torch.as_tensor(np.asarray(colors, dtype=np.uint8), device=dev) if colors is not None else None
    if faces is not None and len(faces) > 0:
        f = torch.as_tensor(np.asarray(faces, dtype=np.int32), device=dev)
        img = shade(raster_faces(v, f, cam, size, size), v, f, cam, c)
    else:
        img = shade(raster_points(v, cam, size, size, POINT_RADIUS_PX * size / 1024.0), v, None, cam, c)
    return img.cpu().numpy()


def write_png(path: str, img: np.ndarray):
    """8-bit RGB PNG of img uint8 [H,W,3], one IDAT chunk, filter 0 on every row (zlib and struct only)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), img.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    png = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b'')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(png)


def read_png(path: str) -> np.ndarray:
    """uint8 [H,W,3] of an 8-bit RGB PNG with filter 0 rows (what write_png writes)."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError('not a PNG file: {}'.format(path))
    pos, idat, w, h = 8, b'', 0, 0
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b'IHDR':
            w, h, depth, ctype = struct.unpack('>IIBB', body[:10])
            if depth != 8 or ctype != 2:
                raise ValueError('only 8-bit RGB PNG is supported: {}'.format(path))
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if np.any(rows[:, 0] != 0):
        raise ValueError('only filter type 0 is supported: {}'.format(path))
    return rows[:, 1:].reshape(h, w, 3).copy()


def render_scene(mesh_file: str, rendering_file: str):
    """visualization.py:25-63: render a mesh or point cloud file to a 1024^2 PNG."""
    if not os.path.isfile(mesh_file):
        print('Rendering failed, file not found: ' + mesh_file)
        return
    verts, faces, colors = load_mesh_any(mesh_file)
    write_png(rendering_file, render(verts, faces, colors))


def render_meshes(all_meshes_in, all_renders_out, workers=1):
    """visualization.py:122-134 in one process; renders whose output is up to date or whose input is missing are skipped."""
    assert len(all_meshes_in) == len(all_renders_out)
    for mesh_in, out in zip(all_meshes_in, all_renders_out):
        if call_necessary(mesh_in, out):
            render_scene(mesh_in, out)
