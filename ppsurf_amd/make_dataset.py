"""Training / test datasets from triangle meshes on the GPU: virtual range scans and signed-distance labels.

    python -m ppsurf_amd.make_dataset --meshes_dir my_meshes --out_dir datasets/my_set [--settings settings.ini] [--num_query_pts 2000]
        [--scan_resolution 64] [--seed 42] [--test_fraction 0.3] [--no_normalize]

Writes the layout that `fit` and `test` read (data.py): `03_meshes/<name>.ply` (the mesh the labels refer to), `04_pts_vis/<name>.xyz.ply`
(the scanned cloud, xyz only), `05_query_pts/<name>.ply.npy` (float32 [n,3]), `05_query_dist/<name>.ply.npy` (float32 [n], signed
distance, positive inside), `trainset.txt` / `valset.txt` / `testset.txt` and a `settings.ini` with the values used.  The reference ships
only the result of its generator (abc_minimal and its settings.ini); BlenSor, trimesh and pysdf are not available, so this is a model of
its own (csrc/pps_scan.hip):
  * each shape has its own generator, seeded from (seed, crc32 of the shape name): a shape's files do not depend on the other shapes;
  * the number of scans is uniform in [num_scans_per_mesh_min, num_scans_per_mesh_max]; scan s looks from c + D u_s at c (u_s uniform on
    the sphere, c the bounding-box centre, rho half its diagonal, D = 3 rho) with a square image of scan_resolution^2 pixels whose field
    of view just holds the bounding sphere (tan(fov / 2) = rho / sqrt(D^2 - rho^2)); every pixel casts one ray, the first hit on the
    mesh (both faces, watertight) is a point, displaced along the ray by sigma_s g (g standard normal, sigma_s uniform in
    [scanner_noise_sigma_min, scanner_noise_sigma_max] x the longest bounding-box edge); misses are dropped;
  * the first floor(n / 2) queries are uniform in [-0.5, 0.5)^3, the others area-weighted surface samples moved along their face normal
    by u r, u uniform in [-1, 1), r = query_near_radius (3 / 128, the band of the reference's near-surface queries);
  * labels: exact distance to the mesh (geometry.closest_point_on_corners) with the sign of the generalised winding number
    (geometry.winding_number, |w| > 0.5 inside -> positive), the convention of the reference's 05_query_dist.
Meshes (PLY or OBJ) are normalised like a single-file input cloud (bounding-box centre to 0, longest edge x 1.05 to 1) unless
--no_normalize, which copies them unchanged (meshes already in a dataset's frame).  A shape whose outputs are newer than its mesh is skipped.
"""
import argparse
import configparser
import math
import os
import shutil
import typing
import zlib

import numpy as np
import torch

from . import _lib, meshio
from .geometry import (_device, area_prefix, closest_point_on_corners, face_stats, first_hit, sample_surface,
                       winding_number)

DEFAULTS = {'num_scans_per_mesh_min': 5, 'num_scans_per_mesh_max': 30, 'scanner_noise_sigma_min': 0.0, 'scanner_noise_sigma_max': 0.05,
            'scan_resolution': 64, 'num_query_pts': 2000, 'query_near_radius': 3.0 / 128.0, 'seed': 42, 'test_fraction': 0.3, 'normalize': 1}
PADDING = 0.05
CAM_FLOATS = 16
MESH_EXTS = ('.ply', '.obj')


# ---- settings, seeds, split ---------------------------------------------------------------------------------------------------------------------
def read_settings(path: str) -> dict:
    """DEFAULTS updated with the known keys of the [general] section of a settings.ini (other keys are ignored)."""
    cp = configparser.ConfigParser()
    if not cp.read(path):
        raise FileNotFoundError(path)
    s = dict(DEFAULTS)
    if cp.has_section('general'):
        for k, v in cp.items('general'):
            if k in DEFAULTS:
                s[k] = type(DEFAULTS[k])(float(v)) if isinstance(DEFAULTS[k], int) else float(v)
    return s


def write_settings(path: str, settings: dict):
    cp = configparser.ConfigParser()
    cp['general'] = {k: repr(settings[k]) for k in DEFAULTS}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        cp.write(f)


def resolve_settings(settings: typing.Optional[dict] = None, **overrides) -> dict:
    """DEFAULTS < settings < overrides that are not None; unknown keys raise."""
    s = dict(DEFAULTS)
    for src in (settings or {}), {k: v for k, v in overrides.items() if v is not None}:
        for k, v in src.items():
            if k not in DEFAULTS:
                raise KeyError('unknown make_dataset setting: {}'.format(k))
            s[k] = type(DEFAULTS[k])(v)
    if not 1 <= s['num_scans_per_mesh_min'] <= s['num_scans_per_mesh_max']:
        raise ValueError('need 1 <= num_scans_per_mesh_min <= num_scans_per_mesh_max')
    if not 0.0 <= s['scanner_noise_sigma_min'] <= s['scanner_noise_sigma_max']:
        raise ValueError('need 0 <= scanner_noise_sigma_min <= scanner_noise_sigma_max')
    if s['scan_resolution'] < 1 or s['num_query_pts'] < 0:
        raise ValueError('scan_resolution must be >= 1 and num_query_pts >= 0')
    return s


def shape_stream(name: str) -> int:
    """crc32 of the shape name: the per-shape part of every generator key."""
    return zlib.crc32(name.encode('utf-8'))


def shape_rng(seed: int, name: str) -> np.random.Generator:
    """The host generator of one shape (scan count, view directions, noise levels)."""
    return np.random.default_rng([int(seed), shape_stream(name)])


def split_names(names: typing.Sequence[str], test_fraction: float, seed: int):
    """(train, test) sorted: ceil(test_fraction n) shapes drawn by a seeded permutation for test (at least 1, at most n - 1), the rest for
    training; a single shape is listed in both."""
    names = sorted(names)
    n = len(names)
    if n <= 1:
        return list(names), list(names)
    n_test = min(max(math.ceil(round(test_fraction * n, 9)), 1), n - 1)
    perm = np.random.default_rng(int(seed)).permutation(n)
    test = sorted(names[i] for i in perm[:n_test])
    train = sorted(names[i] for i in perm[n_test:])
    return train, test


# ---- scanner ------------------------------------------------------------------------------------------------------------------------------------
def scan_cameras(bb_min, bb_max, settings: dict, rng: np.random.Generator) -> np.ndarray:
    """Cameras f32 [n_scans,16] of the scanner model (layout at the top of csrc/pps_scan.hip), fp64 on the host.  Draws, in this order:
    the scan count, n_scans standard-normal 3-vectors (view directions), n_scans noise levels."""
    bb_min, bb_max = np.asarray(bb_min, dtype=np.float64), np.asarray(bb_max, dtype=np.float64)
    c = (bb_min + bb_max) * 0.5
    ext = bb_max - bb_min
    rho = 0.5 * float(np.linalg.norm(ext))
    dist = 3.0 * rho
    n = int(rng.integers(settings['num_scans_per_mesh_min'], settings['num_scans_per_mesh_max'] + 1))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sigma = rng.uniform(settings['scanner_noise_sigma_min'], settings['scanner_noise_sigma_max'], size=n) * float(ext.max())
    eye = c[None] + dist * u
    fwd = -u
    ref = np.where((np.abs(fwd[:, 2]) < 0.9)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    right = np.cross(fwd, ref)
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    up = np.cross(right, fwd)
    cams = np.zeros((n, CAM_FLOATS), dtype=np.float64)
    cams[:, 0:3], cams[:, 3:6], cams[:, 6:9], cams[:, 9:12] = eye, right, up, fwd
    cams[:, 12] = rho / math.sqrt(dist * dist - rho * rho) if rho > 0 else 1.0
    cams[:, 13] = sigma
    return cams.astype(np.float32)


def scan_rays(cams: torch.Tensor, res: int):
    """One ray per pixel of every camera (device f32 [n_scans,16]) -> (orig, dirs f32 [n_scans res^2, 3])."""
    _lib.need_device('make_dataset', cams)
    cams = cams.to(torch.float32).contiguous()
    m = cams.shape[0] * res * res
    orig = torch.empty((m, 3), dtype=torch.float32, device=cams.device)
    dirs = torch.empty((m, 3), dtype=torch.float32, device=cams.device)
    _lib.call('pps_scan_rays', cams, cams.shape[0], int(res), orig, dirs)
    return orig, dirs


def scan_points(corners: torch.Tensor, cams: torch.Tensor, res: int, seed: int, stream_id: int, slices: typing.Optional[int] = None,
                keep_misses: bool = False) -> torch.Tensor:
    """The scans of the cameras cams (device f32 [n_scans,16]) of the mesh corners [nf,9] -> points f32 [k,3] of the hits in (scan, pixel)
    order (keep_misses: every pixel, NaN for a miss)."""
    _lib.need_device('make_dataset', corners, cams)
    cams = cams.to(torch.float32).contiguous()
    orig, dirs = scan_rays(cams, res)
    t, face = first_hit(corners, orig, dirs, slices)
    pts = torch.empty_like(orig)
    _lib.call('pps_scan_points', orig, dirs, t, face, cams, cams.shape[0], int(res), int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), pts)
    return pts if keep_misses else pts[face >= 0]


def _mesh_tables(verts: torch.Tensor, faces: torch.Tensor):
    _lib.need_device('make_dataset', verts, faces)
    v = verts.to(torch.float32).contiguous()
    f = faces.to(torch.int32).contiguous()
    return face_stats(v, f)


def scan_mesh(verts: torch.Tensor, faces: torch.Tensor, name: str, settings: typing.Optional[dict] = None, seed: int = DEFAULTS['seed']) -> torch.Tensor:
    """The virtual scans of one mesh (device verts f32 [nv,3], faces int [nf,3]) -> device point cloud f32 [k,3]."""
    s = resolve_settings(settings)
    _, _, corners = _mesh_tables(verts, faces)
    bb = torch.stack([verts.amin(0), verts.amax(0)]).double().cpu().numpy()
    cams = scan_cameras(bb[0], bb[1], s, shape_rng(seed, name))
    cams_d = torch.from_numpy(cams).to(verts.device)
    return scan_points(corners, cams_d, s['scan_resolution'], seed, shape_stream(name) << 2)


def query_points(verts: torch.Tensor, faces: torch.Tensor, name: str, n: int = DEFAULTS['num_query_pts'], seed: int = DEFAULTS['seed'],
                 radius: float = DEFAULTS['query_near_radius']) -> torch.Tensor:
    """Query points f32 [n,3] of one mesh: floor(n / 2) uniform in [-0.5, 0.5)^3 (stream crc << 2 | 1), then area-weighted surface samples
    (stream crc << 2 | 2) moved along their unit face normal by u radius, u uniform in [-1, 1).  Raises ValueError for a mesh without
    samplable area."""
    area, normal, corners = _mesh_tables(verts, faces)
    n_far = int(n) // 2
    n_near = int(n) - n_far
    out = torch.empty((n_far + n_near, 3), dtype=torch.float32, device=verts.device)
    pts = face = None
    if n_near > 0:
        prefix = area_prefix(area)
        if corners.shape[0] == 0 or not float(prefix[-1]) > 0.0:
            raise ValueError('the mesh has no samplable area')
        pts, face = sample_surface(corners, prefix, n_near, seed, (shape_stream(name) << 2) | 2)
    _lib.call('pps_scan_queries', pts, face, normal, n_far, n_near, int(seed) & (2 ** 64 - 1), (shape_stream(name) << 2) | 1, float(radius), out)
    return out


def signed_distance(verts: torch.Tensor, faces: torch.Tensor, query: torch.Tensor) -> torch.Tensor:
    """Signed distance f32 [m] of query [m,3] to the mesh, all device tensors: the exact distance, positive inside (|winding number| > 0.5)."""
    _lib.need_device('make_dataset', verts, faces, query)
    _, _, corners = _mesh_tables(verts, faces)
    query = query.to(torch.float32).contiguous()
    _, d, _ = closest_point_on_corners(corners, query)
    w = winding_number(corners, query)
    return torch.where(w.abs() > 0.5, d, -d)


# ---- files --------------------------------------------------------------------------------------------------------------------------------------
def normalize_mesh(verts: np.ndarray) -> np.ndarray:
    """data.load_shape_data_pc(normalize=True) for mesh vertices: bounding-box centre to 0, longest edge x 1.05 to 1 (fp64, then f32)."""
    v = np.asarray(verts, dtype=np.float64)
    bb_min, bb_max = v.min(axis=0), v.max(axis=0)
    return ((v - (bb_min + bb_max) * 0.5) / (np.max(bb_max - bb_min) * (1.0 + PADDING))).astype(np.float32)


def mesh_files(meshes_dir: str):
    """{shape name: path} of the PLY / OBJ meshes of a directory (a name found twice raises)."""
    out = {}
    for fn in sorted(os.listdir(meshes_dir)):
        base, ext = os.path.splitext(fn)
        if ext.lower() in MESH_EXTS and os.path.isfile(os.path.join(meshes_dir, fn)):
            if base in out:
                raise ValueError('two meshes named {} in {}'.format(base, meshes_dir))
            out[base] = os.path.join(meshes_dir, fn)
    return out


def output_files(out_dir: str, name: str):
    return [os.path.join(out_dir, '03_meshes', name + '.ply'), os.path.join(out_dir, '04_pts_vis', name + '.xyz.ply'),
            os.path.join(out_dir, '05_query_pts', name + '.ply.npy'), os.path.join(out_dir, '05_query_dist', name + '.ply.npy')]


def make_shape(mesh_file: str, out_dir: str, name: str, settings: dict, device) -> int:
    """All files of one shape; returns its point count."""
    f_mesh, f_pts, f_q, f_d = output_files(out_dir, name)
    verts, faces, _ = meshio.load_mesh_any(mesh_file)
    if settings['normalize']:
        verts = normalize_mesh(verts)
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(device)
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(device)
    area = face_stats(v, f)[0] if faces.shape[0] else torch.zeros(0, device=device)
    if not float(area.double().sum()) > 0.0:
        raise ValueError('{}: the mesh has no samplable area'.format(mesh_file))
    seed = settings['seed']
    pts = scan_mesh(v, f, name, settings, seed)
    q = query_points(v, f, name, settings['num_query_pts'], seed, settings['query_near_radius'])
    d = signed_distance(v, f, q)
    if settings['normalize'] or os.path.splitext(mesh_file)[1].lower() != '.ply':
        meshio.write_ply_mesh(f_mesh, verts, faces)
    else:
        os.makedirs(os.path.dirname(f_mesh), exist_ok=True)
        shutil.copyfile(mesh_file, f_mesh)
    meshio.write_ply_points(f_pts, pts.cpu().numpy())
    for fn, arr in ((f_q, q), (f_d, d)):
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        np.save(fn, arr.cpu().numpy().astype(np.float32))
    return int(pts.shape[0])


def make_dataset(meshes_dir: str, out_dir: str, settings: typing.Optional[dict] = None, verbose: bool = True, **overrides) -> typing.List[str]:
    """Builds the dataset of every PLY / OBJ mesh in meshes_dir into out_dir; returns the names of the shapes built (the others were up to
    date).  settings: a dict of DEFAULTS keys (read_settings), overrides: the same keys, None meaning unset."""
    s = resolve_settings(settings, **overrides)
    meshes = mesh_files(meshes_dir)
    if not meshes:
        raise ValueError('no PLY or OBJ meshes in {}'.format(meshes_dir))
    device = _device()
    built = []
    for name, path in meshes.items():
        if not meshio.call_necessary(path, output_files(out_dir, name)):
            continue
        n = make_shape(path, out_dir, name, s, device)
        built.append(name)
        if verbose:
            print('{}: {} points'.format(name, n), flush=True)
    train, test = split_names(list(meshes), s['test_fraction'], s['seed'])
    for fn, names in (('trainset.txt', train), ('valset.txt', test), ('testset.txt', test)):
        with open(os.path.join(out_dir, fn), 'w') as f:
            f.write(''.join(n + '\n' for n in names))
    write_settings(os.path.join(out_dir, 'settings.ini'), s)
    return built


def parse_arguments(args=None):
    ap = argparse.ArgumentParser(description='Virtual scans and signed-distance labels of a directory of meshes (GPU).')
    ap.add_argument('--meshes_dir', required=True, help='directory of PLY / OBJ meshes')
    ap.add_argument('--out_dir', required=True, help='dataset root to write')
    ap.add_argument('--settings', default=None, help='settings.ini whose [general] keys are honoured')
    ap.add_argument('--num_query_pts', type=int, default=None, help='queries per shape (default {})'.format(DEFAULTS['num_query_pts']))
    ap.add_argument('--scan_resolution', type=int, default=None, help='pixels per scan side (default {})'.format(DEFAULTS['scan_resolution']))
    ap.add_argument('--seed', type=int, default=None, help='default {}'.format(DEFAULTS['seed']))
    ap.add_argument('--test_fraction', type=float, default=None, help='share of shapes in testset / valset (default 0.3)')
    ap.add_argument('--no_normalize', action='store_true', help='copy the meshes unchanged instead of normalising them')
    return ap.parse_args(args)


def main(argv=None):
    a = parse_arguments(argv)
    settings = read_settings(a.settings) if a.settings else None
    built = make_dataset(a.meshes_dir, a.out_dir, settings, num_query_pts=a.num_query_pts, scan_resolution=a.scan_resolution, seed=a.seed,
                         test_fraction=a.test_fraction, normalize=0 if a.no_normalize else None)
    print('built {} shape(s) into {}'.format(len(built), a.out_dir))
    return built


if __name__ == '__main__':
    main()
