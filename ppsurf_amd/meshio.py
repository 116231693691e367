"""Minimal PLY / XYZ / NPY / LAS / STL / OFF / OBJ / PCD IO for the predict path and the mesh evaluation (the reference uses trimesh, absent here);
`load_pts_colors` is the colour half of `load_pts`.

Point clouds of datasets/abc_minimal are binary little-endian PLY written by trimesh
(`element vertex n`, `property float x/y/z`, optional normals, `element face 0`); meshes are written the same way
(source/poco_model.py:269 `mesh.export`).  Replaces the IO part of source/occupancy_data_module.py:174-225.
"""
import os

import numpy as np

_PLY_TYPES = {'char': 'i1', 'uchar': 'u1', 'short': 'i2', 'ushort': 'u2', 'int': 'i4', 'uint': 'u4', 'float': 'f4', 'double': 'f8',
              'int8': 'i1', 'uint8': 'u1', 'int16': 'i2', 'uint16': 'u2', 'int32': 'i4', 'uint32': 'u4', 'float32': 'f4', 'float64': 'f8'}


def read_ply_vertices(path):
    """Vertex x,y,z (+ nx,ny,nz if present) of an ascii or binary PLY -> float array [n, 3|6]."""
    cols = _ply_vertex_columns(path)
    names = ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if all(k in cols for k in ('nx', 'ny', 'nz')) else [])
    return np.stack([np.asarray(cols[k], dtype=np.float64) for k in names], axis=1)


def read_ply_vertex_colors(path):
    """Vertex colours uint8 [n,3] (red, green, blue) of an ascii or binary PLY, or None when the vertices carry no colour.  Float colour
    properties in [0, 1] are scaled to [0, 255]."""
    cols = _ply_vertex_columns(path)
    if not all(k in cols for k in ('red', 'green', 'blue')):
        return None
    rgb = np.stack([np.asarray(cols[k]) for k in ('red', 'green', 'blue')], axis=1)
    if rgb.dtype.kind == 'f':
        rgb = np.rint(np.clip(rgb, 0.0, 1.0) * 255.0)
    return rgb.astype(np.uint8)


def _ply_vertex_columns(path):
    """{property name: array [n]} of the vertex element of an ascii or binary PLY (the vertex element must come first)."""
    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError('not a PLY file: {}'.format(path))
        fmt, nvert, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError('unterminated PLY header: {}'.format(path))
            tok = line.decode('ascii', 'replace').split()
            if not tok:
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                in_vertex = tok[1] == 'vertex'
                if in_vertex:
                    nvert = int(tok[2])
            elif tok[0] == 'property' and in_vertex:
                if tok[1] == 'list':
                    raise ValueError('list property on vertices is not supported')
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == 'end_header':
                break
        if fmt == 'ascii':
            data = np.loadtxt(f, max_rows=nvert, ndmin=2)
            cols = {name: data[:, i] for i, (name, _) in enumerate(props)}
        else:
            end = '<' if fmt == 'binary_little_endian' else '>'
            rec = np.frombuffer(f.read(nvert * sum(np.dtype(t).itemsize for _, t in props)),
                                dtype=np.dtype([(n, end + t) for n, t in props]), count=nvert)
            cols = {name: rec[name] for name, _ in props}
    return cols


def _fan(polys):
    """Triangles of polygons fanned from their first corner (trimesh's triangulation of n-gons): [v0, vi, vi+1]."""
    tris = []
    for p in polys:
        p = np.asarray(p, dtype=np.int64)
        if p.shape[0] >= 3:
            tris.append(np.stack([np.full(p.shape[0] - 2, p[0]), p[1:-1], p[2:]], axis=1))
    return np.concatenate(tris, axis=0) if tris else np.zeros((0, 3), dtype=np.int64)


def read_ply_mesh(path, dtype=np.float32):
    """Vertices float32 [nv,3] (`dtype=np.float64` keeps the doubles of a `write_ply_mesh(..., double=True)` file) and triangles int32 [nf,3] of an ascii or binary PLY mesh (trimesh-written `03_meshes` files and
    write_ply_mesh): float or double x/y/z (other vertex properties skipped), face list `vertex_indices` (or `vertex_index`) of
    uchar/int/uint counts and int/uint indices, polygons fan-triangulated.  Other face properties and elements after `face` are skipped
    (binary: fixed-size ones only).  Raises ValueError on anything else or on an index outside [0, nv)."""
    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError('not a PLY file: {}'.format(path))
        fmt, elements = None, []                          # [name, count, [(prop, dtype) | (prop, (count_dtype, item_dtype))]]
        while True:
            line = f.readline()
            if not line:
                raise ValueError('unterminated PLY header: {}'.format(path))
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] in ('comment', 'obj_info'):
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == 'property':
                if not elements:
                    raise ValueError('PLY property before any element: {}'.format(path))
                if tok[1] == 'list':
                    elements[-1][2].append((tok[4], (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
                else:
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == 'end_header':
                break
        if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            raise ValueError('unknown PLY format {!r}: {}'.format(fmt, path))
        body = f.read()
    verts, faces = None, None
    end = '>' if fmt == 'binary_big_endian' else '<'
    pos = 0
    lines = body.decode('ascii', 'replace').split('\n') if fmt == 'ascii' else None
    for name, count, props in elements:
        if name == 'vertex':
            if any(isinstance(t, tuple) for _, t in props):
                raise ValueError('list property on vertices is not supported: {}'.format(path))
            names = [n for n, _ in props]
            if not all(k in names for k in 'xyz'):
                raise ValueError('PLY vertices without x/y/z: {}'.format(path))
            if fmt == 'ascii':
                data = np.array([lines[pos + i].split()[:len(props)] for i in range(count)], dtype=np.float64).reshape(count, len(props))
                pos += count
                verts = np.stack([data[:, names.index(k)] for k in 'xyz'], axis=1)
            else:
                dt = np.dtype([(n, end + t) for n, t in props])
                rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                verts = np.stack([rec[k].astype(np.float64) for k in 'xyz'], axis=1)
        elif name == 'face':
            lists = [i for i, (_, t) in enumerate(props) if isinstance(t, tuple)]
            idx_prop = [i for i in lists if props[i][0] in ('vertex_indices', 'vertex_index')]
            if not idx_prop:
                raise ValueError('PLY faces without vertex_indices: {}'.format(path))
            ip = idx_prop[0]
            if fmt == 'ascii':
                polys = []
                for i in range(count):
                    vals = lines[pos + i].split()
                    at = 0
                    for j, (_, t) in enumerate(props):
                        if isinstance(t, tuple):
                            k = int(vals[at])
                            if j == ip:
                                polys.append([int(v) for v in vals[at + 1:at + 1 + k]])
                            at += 1 + k
                        else:
                            at += 1
                pos += count
                faces = _fan(polys)
            elif len(props) == 1:
                cdt, idt = np.dtype(end + props[0][1][0]), np.dtype(end + props[0][1][1])
                if count > 0:
                    k0 = int(np.frombuffer(body, dtype=cdt, count=1, offset=pos)[0])
                    dt = np.dtype([('n', cdt), ('v', idt, (k0,))])
                    rec = np.frombuffer(body, dtype=dt, count=count, offset=pos) if pos + count * dt.itemsize <= len(body) else None
                    if rec is not None and np.all(rec['n'] == k0):            # every face has the same corner count: one view
                        pos += count * dt.itemsize
                        faces = _fan([]) if k0 < 3 else _fan_uniform(rec['v'].astype(np.int64))
                        continue
                polys = []
                for _ in range(count):
                    k = int(np.frombuffer(body, dtype=cdt, count=1, offset=pos)[0])
                    polys.append(np.frombuffer(body, dtype=idt, count=k, offset=pos + cdt.itemsize))
                    pos += cdt.itemsize + k * idt.itemsize
                faces = _fan(polys)
            else:
                polys = []
                for _ in range(count):
                    for j, (_, t) in enumerate(props):
                        if isinstance(t, tuple):
                            cdt, idt = np.dtype(end + t[0]), np.dtype(end + t[1])
                            k = int(np.frombuffer(body, dtype=cdt, count=1, offset=pos)[0])
                            if j == ip:
                                polys.append(np.frombuffer(body, dtype=idt, count=k, offset=pos + cdt.itemsize))
                            pos += cdt.itemsize + k * idt.itemsize
                        else:
                            pos += np.dtype(t).itemsize
                faces = _fan(polys)
        else:                                             # other elements: skipped (fixed-size records only in binary files)
            if fmt == 'ascii':
                pos += count
            elif any(isinstance(t, tuple) for _, t in props):
                if count > 0:
                    raise ValueError('list property on PLY element {!r} is not supported: {}'.format(name, path))
            else:
                pos += count * sum(np.dtype(t).itemsize for _, t in props)
    if verts is None:
        raise ValueError('PLY file without vertices: {}'.format(path))
    if faces is None:
        faces = np.zeros((0, 3), dtype=np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= verts.shape[0]):
        raise ValueError('PLY face index out of range: {}'.format(path))
    return verts.astype(dtype), faces.astype(np.int32)


def _fan_uniform(v):
    """_fan for polygons that all have the same corner count k >= 3, v int [n, k] -> [n * (k - 2), 3] (polygon-major)."""
    k = v.shape[1]
    return np.stack([np.repeat(v[:, :1], k - 2, axis=1), v[:, 1:-1], v[:, 2:]], axis=2).reshape(-1, 3)


def _las_records(path):
    """(point format, record length, number of records, the records' bytes, scale, offset) of an uncompressed LAS 1.0-1.4 file."""
    import struct
    with open(path, 'rb') as f:
        head = f.read(375)
        if len(head) < 227 or head[:4] != b'LASF':
            raise ValueError('not a LAS file: {}'.format(path))
        major, minor = head[24], head[25]
        header_size, data_offset = struct.unpack_from('<HI', head, 94)
        fmt, rec_len, n = struct.unpack_from('<BHI', head, 104)
        if fmt & 0xC0:
            raise ValueError('compressed LAS (LAZ) is not supported: {}: decompress it to .las or convert it to .npy first'.format(path))
        if (major, minor) >= (1, 4) and n == 0 and len(head) >= 255:
            n = struct.unpack_from('<Q', head, 247)[0]
        if major != 1 or minor > 4 or fmt > 10 or rec_len < 12:
            raise ValueError('unsupported LAS {}.{} point format {}: {}'.format(major, minor, fmt, path))
        scale = np.array(struct.unpack_from('<3d', head, 131), dtype=np.float64)
        offset = np.array(struct.unpack_from('<3d', head, 155), dtype=np.float64)
        f.seek(data_offset)
        raw = f.read(n * rec_len)
    if len(raw) < n * rec_len:
        raise ValueError('LAS file ends before its {} point records: {}'.format(n, path))
    return fmt, rec_len, n, raw, scale, offset


def read_las_points(path):
    """x, y, z float64 [n,3] of an uncompressed LAS 1.0-1.4 file, point formats 0-10 (ASPRS LAS specification, public header block):
    offset to point data (byte 96), point format (104), record length (105), legacy number of points (107; for 1.4 the 64-bit field at 247
    when the legacy one is 0), scale (131) and offset (155).  Every record starts with int32 X, Y, Z; xyz = int32 * scale + offset in float64,
    as laspy's `las.xyz`.  Colours and intensity are read by read_las_colors; classification is not read."""
    fmt, rec_len, n, raw, scale, offset = _las_records(path)
    ints = np.ndarray((n, 3), dtype='<i4', buffer=raw, strides=(rec_len, 4)) if n else np.zeros((0, 3), dtype='<i4')
    return ints.astype(np.float64) * scale[None] + offset[None]


_LAS_RGB_AT = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}          # format 0 is 20 bytes, GPS time adds 8, format 6 is 30 (ASPRS record layouts)


def read_las_colors(path):
    """Colours uint8 [n,3] of the records read_las_points returns, or None.  RGB: three uint16 at record offset 20 (format 2), 28 (3, 5) or 30
    (7, 8, 10), `v >> 8` when the file's largest value exceeds 255 and `v` itself otherwise (many writers store 0..255).  A format without
    RGB, or RGB that is 0 everywhere, falls back to a grey from the intensity I (uint16 at offset 12): (I * 255 + Imax // 2) // Imax in
    integers, Imax the file's maximum; None when that is 0.  A record too short for the field raises ValueError."""
    fmt, rec_len, n, raw, _, _ = _las_records(path)
    if n == 0:
        return None
    at = _LAS_RGB_AT.get(fmt)
    if at is not None:
        if rec_len < at + 6:
            raise ValueError('LAS point format {} with records of {} bytes, too short for RGB at offset {}: {}'.format(fmt, rec_len, at, path))
        rgb = np.ndarray((n, 3), dtype='<u2', buffer=raw, offset=at, strides=(rec_len, 2)).astype(np.uint16)
        top = int(rgb.max())
        if top > 0:
            return (rgb >> 8 if top > 255 else rgb).astype(np.uint8)
    if rec_len < 14:
        raise ValueError('LAS records of {} bytes, too short for the intensity at offset 12: {}'.format(rec_len, path))
    inten = np.ndarray((n,), dtype='<u2', buffer=raw, offset=12, strides=(rec_len,)).astype(np.int64)
    imax = int(inten.max())
    if imax == 0:
        return None
    g = ((inten * 255 + imax // 2) // imax).astype(np.uint8)
    return np.stack([g, g, g], axis=1)


def read_stl_vertices(path):
    """Facet corners float64 [3 nf, 3] of a binary or ascii STL as they are stored (three per facet, duplicates kept)."""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) >= 84:
        nf = int(np.frombuffer(data, dtype='<u4', count=1, offset=80)[0])
        if len(data) == 84 + 50 * nf:                      # the size test tells binary from ascii (binary headers may start with `solid` too)
            rec = np.frombuffer(data, dtype=np.dtype([('n', '<f4', (3,)), ('v', '<f4', (3, 3)), ('a', '<u2')]), count=nf, offset=84)
            return rec['v'].reshape(-1, 3).astype(np.float64)
    if not data.lstrip()[:5].lower() == b'solid':
        raise ValueError('neither a binary nor an ascii STL: {}'.format(path))
    verts = [line.split()[1:4] for line in data.decode('ascii', 'replace').split('\n') if line.split()[:1] == ['vertex']]
    v = np.array(verts, dtype=np.float64).reshape(-1, 3)
    if v.shape[0] % 3:
        raise ValueError('ascii STL with a vertex count that is no multiple of 3: {}'.format(path))
    return v


def _off_vertex_lines(path):
    """(keyword, token lists of the nv vertex lines) of an OFF / COFF / NOFF file."""
    with open(path, 'r') as f:
        lines = [t for t in (line.split('#', 1)[0].split() for line in f) if t]
    if not lines or not lines[0][0].upper().endswith('OFF'):
        raise ValueError('not an OFF file: {}'.format(path))
    counts = lines[0][1:] if len(lines[0]) > 1 else (lines[1] if len(lines) > 1 else [])
    first = 1 if len(lines[0]) > 1 else 2
    try:
        nv = int(counts[0])
    except (IndexError, ValueError):
        raise ValueError('malformed OFF file: {}'.format(path))
    rows = lines[first:first + nv]
    if len(rows) != nv:
        raise ValueError('OFF file ends before its {} vertices: {}'.format(nv, path))
    return lines[0][0].upper(), rows


def read_off_vertices(path):
    """Vertices float64 [nv,3] of an OFF / COFF / NOFF file: the `OFF` keyword (the counts `nv nf ne` on the same or the next line), then nv
    lines that start with x y z (normals after them are skipped, colours are read by read_off_colors); `#` comments and empty lines anywhere."""
    _, rows = _off_vertex_lines(path)
    try:
        v = np.array([t[:3] for t in rows], dtype=np.float64).reshape(-1, 3)
    except ValueError:
        raise ValueError('malformed OFF file: {}'.format(path))
    return v


def read_off_colors(path):
    """Colours uint8 [nv,3] of the vertices of an OFF file whose keyword contains `C` (COFF, CNOFF, ...), or None.  The colour columns follow
    x y z, and the normal where the keyword contains `N`; an alpha column is ignored.  Tokens with `.`, `e` or `E` anywhere make the file's
    colours floats in [0, 1], converted with rint(clip * 255); otherwise they are integers 0..255."""
    keyword, rows = _off_vertex_lines(path)
    word = keyword[:-3]
    if 'C' not in word or not rows:
        return None
    at = 6 if 'N' in word else 3
    try:
        tok = [t[at:at + 3] for t in rows]
        if any(len(t) != 3 for t in tok):
            raise ValueError
        if any(ch in c for t in tok for c in t for ch in '.eE'):
            return np.rint(np.clip(np.array(tok, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        return np.clip(np.array(tok, dtype=np.int64), 0, 255).astype(np.uint8)
    except ValueError:
        raise ValueError('malformed colours in OFF file: {}'.format(path))


_PCD_TYPES = {('F', 4): 'f4', ('F', 8): 'f8', ('I', 1): 'i1', ('I', 2): 'i2', ('I', 4): 'i4', ('I', 8): 'i8',
              ('U', 1): 'u1', ('U', 2): 'u2', ('U', 4): 'u4', ('U', 8): 'u8'}


def _pcd_parts(path):
    """(fields, sizes, types, counts, n, mode, body) of a PCD 0.7 file."""
    with open(path, 'rb') as f:
        head = {}
        while True:
            line = f.readline()
            if not line:
                raise ValueError('unterminated PCD header: {}'.format(path))
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0].startswith('#'):
                continue
            head[tok[0].upper()] = tok[1:]
            if tok[0].upper() == 'DATA':
                break
        body = f.read()
    try:
        fields, sizes, types = head['FIELDS'], [int(v) for v in head['SIZE']], head['TYPE']
        counts = [int(v) for v in head.get('COUNT', ['1'] * len(fields))]
        n = int(head['POINTS'][0]) if 'POINTS' in head else int(head['WIDTH'][0]) * int(head['HEIGHT'][0])
        mode = head['DATA'][0].lower()
    except (KeyError, IndexError, ValueError):
        raise ValueError('incomplete PCD header: {}'.format(path))
    return fields, sizes, types, counts, n, mode, body


def _pcd_ascii_rows(body, n, path):
    rows = [line.split() for line in body.decode('ascii', 'replace').split('\n') if line.strip()][:n]
    if len(rows) < n:
        raise ValueError('PCD file ends before its {} points: {}'.format(n, path))
    return rows


def _pcd_records(fields, sizes, types, counts, n, body, path):
    dt = np.dtype([(name, '<' + _PCD_TYPES[(t.upper(), s)], (c,)) for name, s, t, c in zip(fields, sizes, types, counts)])
    if len(body) < n * dt.itemsize:
        raise ValueError('PCD file ends before its {} points: {}'.format(n, path))
    return np.frombuffer(body, dtype=dt, count=n)


def read_pcd_points(path):
    """x, y, z [n,3] of a PCD 0.7 file (Point Cloud Library), `DATA ascii` or `DATA binary`, any field list that holds x y z as 4- or 8-byte
    floats (float64 out when they are 8-byte, float32 otherwise)."""
    fields, sizes, types, counts, n, mode, body = _pcd_parts(path)
    for k in 'xyz':
        if k not in fields or types[fields.index(k)].upper() != 'F' or sizes[fields.index(k)] not in (4, 8) or counts[fields.index(k)] != 1:
            raise ValueError('PCD without float x y z fields: {}'.format(path))
    out_type = np.float64 if any(sizes[fields.index(k)] == 8 for k in 'xyz') else np.float32
    if mode == 'ascii':
        starts = np.concatenate([[0], np.cumsum(counts)])
        rows = _pcd_ascii_rows(body, n, path)
        return np.array([[r[starts[fields.index(k)]] for k in 'xyz'] for r in rows], dtype=out_type).reshape(n, 3)
    if mode != 'binary':
        raise ValueError('PCD DATA {} is not supported (ascii and binary are): {}'.format(mode, path))
    rec = _pcd_records(fields, sizes, types, counts, n, body, path)
    return np.stack([rec[k][:, 0].astype(out_type) for k in 'xyz'], axis=1)


def read_pcd_colors(path):
    """Colours uint8 [n,3] of a PCD file with a 4-byte field `rgb` or `rgba` of TYPE F, U or I (COUNT 1), or None.  The field's four bytes are
    the uint32 0x..RRGGBB (PCL's packing); an ascii value of TYPE F is parsed as float32 and its bits are taken."""
    fields, sizes, types, counts, n, mode, body = _pcd_parts(path)
    name = 'rgb' if 'rgb' in fields else 'rgba' if 'rgba' in fields else None
    if name is None:
        return None
    at = fields.index(name)
    if sizes[at] != 4 or counts[at] != 1 or types[at].upper() not in ('F', 'U', 'I'):
        return None
    if mode not in ('ascii', 'binary'):
        raise ValueError('PCD DATA {} is not supported (ascii and binary are): {}'.format(mode, path))
    if mode == 'ascii':
        col = int(np.sum(counts[:at]))
        tok = [r[col] for r in _pcd_ascii_rows(body, n, path)]
        if types[at].upper() == 'F':
            packed = np.array(tok, dtype=np.float32).view(np.uint32)
        else:
            packed = (np.array([int(t) for t in tok], dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    else:
        packed = np.ascontiguousarray(_pcd_records(fields, sizes, types, counts, n, body, path)[name][:, 0]).view(np.uint32)
    packed = packed.reshape(n)
    return np.stack([(packed >> 16) & 0xFF, (packed >> 8) & 0xFF, packed & 0xFF], axis=1).astype(np.uint8)


def load_pts(pts_file: str) -> np.ndarray:
    """source/occupancy_data_module.py:174-225 without a third-party package: the reference's formats (trimesh for STL / OBJ / OFF, laspy for
    LAS) are read here from their published layouts.  LAS and 8-byte PCD coordinates stay float64."""
    ext = os.path.splitext(pts_file)[1].lower()
    if ext == '.npy':
        return np.load(pts_file)
    if ext == '.npz':
        return np.load(pts_file)['arr_0']
    if ext == '.xyz':
        return np.loadtxt(pts_file, ndmin=2)
    if ext == '.ply':
        return read_ply_vertices(pts_file)
    if ext == '.las':
        return read_las_points(pts_file)
    if ext in ('.laz', '.copc', '.crs'):
        raise ValueError('compressed LAS is not supported ({}): decompress it to .las or convert it to .npy first'.format(pts_file))
    if ext == '.stl':
        return read_stl_vertices(pts_file)
    if ext == '.off':
        return read_off_vertices(pts_file)
    if ext == '.obj':
        return read_obj_mesh(pts_file)[0]
    if ext == '.pcd':
        return read_pcd_points(pts_file)
    raise ValueError('Unknown point cloud type: {}'.format(pts_file))


def load_pts_colors(pts_file: str):
    """Colours uint8 [n,3] of the rows `load_pts(pts_file)` returns, one to one, or None when the file carries none.  PLY red/green/blue, LAS
    RGB (or a grey from the intensity), PCD packed rgb / rgba, COFF and `v x y z r g b` of an OBJ; .xyz / .npy columns 3-5 are normals."""
    ext = os.path.splitext(pts_file)[1].lower()
    if ext == '.ply':
        return read_ply_vertex_colors(pts_file)
    if ext == '.las':
        return read_las_colors(pts_file)
    if ext == '.pcd':
        return read_pcd_colors(pts_file)
    if ext == '.off':
        return read_off_colors(pts_file)
    if ext == '.obj':
        return read_obj_mesh(pts_file, colors=True)[2]
    return None


def _write_ply(path, pos, double, normals, colors_u8, faces):
    """The one layout of every writer below, binary little-endian: `x y z` float or double, then `nx ny nz` float when given, then `red green
    blue alpha` uchar when given (three columns get alpha 255), then the faces; faces=None is `element face 0`."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ftype, name = ('<f8', 'double') if double else ('<f4', 'float')
    pos = np.asarray(pos, dtype=ftype).reshape(-1, 3)
    n = pos.shape[0]
    fields, cols = [('p', ftype, (3,))], {'p': pos}
    header = 'ply\nformat binary_little_endian 1.0\ncomment ppsurf_amd\nelement vertex {0}\nproperty {1} x\nproperty {1} y\nproperty {1} z\n'.format(n, name)
    if normals is not None:
        fields.append(('n', '<f4', (3,)))
        cols['n'] = np.asarray(normals, dtype='<f4').reshape(n, 3)
        header += 'property float nx\nproperty float ny\nproperty float nz\n'
    if colors_u8 is not None:
        colors = np.asarray(colors_u8, dtype=np.uint8).reshape(n, -1)
        if colors.shape[1] == 3:
            colors = np.concatenate([colors, np.full((n, 1), 255, dtype=np.uint8)], axis=1)
        fields.append(('c', 'u1', (4,)))
        cols['c'] = colors[:, :4]
        header += 'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n'
    faces = np.zeros((0, 3), dtype='<i4') if faces is None else np.asarray(faces, dtype='<i4').reshape(-1, 3)
    header += 'element face {}\nproperty list uchar int vertex_indices\nend_header\n'.format(faces.shape[0])
    vrec = np.empty(n, dtype=fields)
    for k, col in cols.items():
        vrec[k] = col
    frec = np.empty(faces.shape[0], dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    frec['n'] = 3
    frec['v'] = faces
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def write_ply_mesh(path, verts: np.ndarray, faces: np.ndarray, double=False, normals: np.ndarray = None, colors_u8: np.ndarray = None):
    """Binary little-endian PLY mesh `x y z [nx ny nz] [red green blue alpha]`; double=True stores `property double x/y/z` (geo-referenced
    coordinates lose centimetres in float32).  The normals are always `float`; colors_u8 uint8 [nv,3] (alpha 255) or
    [nv,4], the layout trimesh exports for vertex colours."""
    _write_ply(path, verts, double, normals, colors_u8, faces)


def write_ply_points(path, pts: np.ndarray):
    """Binary little-endian PLY with float x/y/z vertices and zero faces (layout of datasets/*/04_pts_vis/*.xyz.ply)."""
    _write_ply(path, pts, False, None, None, None)


def write_ply_mesh_colored(path, verts: np.ndarray, faces: np.ndarray, colors_u8: np.ndarray, double=False):
    """write_ply_mesh with per-vertex colours."""
    _write_ply(path, verts, double, None, colors_u8, faces)


def write_ply_mesh_normals(path, verts: np.ndarray, faces: np.ndarray, normals: np.ndarray, colors_u8: np.ndarray = None, double=False):
    """write_ply_mesh with per-vertex normals, and colours when given."""
    _write_ply(path, verts, double, normals, colors_u8, faces)


def write_ply_points_normals(path, pts: np.ndarray, normals: np.ndarray, double=False):
    """Binary little-endian PLY point cloud `x y z nx ny nz` with zero faces: the layout read_ply_vertices returns as [n,6].  The normals are
    always `float`; double=True stores `property double x/y/z`."""
    _write_ply(path, pts, double, normals, None, None)


def read_obj_mesh(path, colors=False):
    """Vertices float32 [nv,3] and triangles int32 [nf,3] of a Wavefront OBJ: `v x y z` and `f` lines only (`a`, `a/b`, `a//c`, `a/b/c`
    corners, 1-based or negative (relative) indices, polygons fan-triangulated).  Raises ValueError on an index outside the vertices.
    colors=True: a third result, uint8 [nv,3] from `v x y z r g b` with r g b floats in [0, 1] (rint(clip * 255)) when EVERY `v` line has
    them, else None."""
    verts, polys, rgb = [], [], []
    with open(path, 'r') as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == 'v':
                verts.append([float(t) for t in tok[1:4]])
                if colors and len(tok) >= 7:
                    rgb.append(tok[4:7])
            elif tok[0] == 'f':
                poly = []
                for c in tok[1:]:
                    i = int(c.split('/')[0])
                    poly.append(i - 1 if i > 0 else len(verts) + i)
                polys.append(poly)
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = _fan(polys)
    if faces.size and (faces.min() < 0 or faces.max() >= v.shape[0]):
        raise ValueError('OBJ face index out of range: {}'.format(path))
    if colors:
        col = None
        if rgb and len(rgb) == len(verts):
            col = np.rint(np.clip(np.array(rgb, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        return v, faces.astype(np.int32), col
    return v, faces.astype(np.int32)


def load_mesh_any(path: str):
    """(verts f32 [nv,3], faces int32 [nf,3], colours uint8 [nv,3] or None) of a PLY, OBJ or .npy (points) file."""
    ext = os.path.splitext(path)[1].lower()
    if ext == '.npy':
        pts = np.load(path)
        return np.asarray(pts, dtype=np.float32)[:, :3], np.zeros((0, 3), dtype=np.int32), None
    if ext == '.obj':
        return read_obj_mesh(path, colors=True)
    if ext == '.ply':
        v, f = read_ply_mesh(path)
        return v, f, read_ply_vertex_colors(path)
    raise ValueError('unsupported mesh file: {}'.format(path))


def ply_stores_doubles(path) -> bool:
    """True when the PLY file's header declares `property double x`: a file that write_ply_mesh(..., double=True) or a geo-referenced export wrote."""
    with open(path, 'rb') as f:
        head = f.read(4096)
    return b'property double x' in head.split(b'end_header')[0]


def read_mesh_file(path: str):
    """(verts float64 [nv,3], faces int32 [nf,3], colours uint8 [nv,3] or None, double) of the mesh file of a command line: a PLY is read as
    float64 with its colours and whether it stores doubles (a writer's `double=`); OBJ and .npy go through load_mesh_any."""
    if os.path.splitext(path)[1].lower() == '.ply':
        verts, faces = read_ply_mesh(path, dtype=np.float64)
        return verts, faces, read_ply_vertex_colors(path), ply_stores_doubles(path)
    verts, faces, colors = load_mesh_any(path)
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), faces, colors, False


def box_centre(pts):
    """The float64 centre of the box of pts [n,3] (zeros for no points)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return (pts.min(axis=0) + pts.max(axis=0)) * 0.5 if pts.shape[0] else np.zeros(3)


def centred_f32(pts, centre):
    """float32 [n,3]: pts - centre in float64 on the host and only then the cast to float32 (geo-referenced coordinates)."""
    return (np.asarray(pts, dtype=np.float64).reshape(-1, 3) - np.asarray(centre, dtype=np.float64)[None]).astype(np.float32)


def need_ply_output(ap, *names, plural=False):
    """ap.error (exit code 2) unless every given output name of an argparse front end ends in .ply; None is skipped."""
    for name in names:
        if name is not None and os.path.splitext(name)[1].lower() != '.ply':
            ap.error('the outputs are .ply files' if plural else 'the output is a .ply file')


def call_necessary(file_in, file_out) -> bool:
    """source/base/fs.py `call_necessary`: False when an input is missing; True when an output is missing or not newer than every input."""
    file_in = [file_in] if isinstance(file_in, str) else list(file_in)
    file_out = [file_out] if isinstance(file_out, str) else list(file_out)
    if not file_out:
        return True
    if any(not os.path.isfile(f) for f in file_in):
        return False
    if any(not os.path.isfile(f) for f in file_out):
        return True
    return max(os.path.getmtime(f) for f in file_in) >= min(os.path.getmtime(f) for f in file_out)
