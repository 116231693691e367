"""The frame of the commands that work on a mesh in its own box: smooth, denoise, fill, pieces, decimate, orient, weld, manifold, flip, subdivide, intersect, remesh and normals
(DESIGN.md section 18).  `load` reads and checks the file and centres it, `Mesh.to_device` uploads it, and four writers put the result
back: as read, gathered through rows, moved positions on the centre, or -- for decimate, subdivide and remesh, which drop, move and add
vertices -- every vertex through the row it came from (`write_origin`).  The stages work on row numbers and on the centred float32 copy,
so whatever they do not move is written from the file's own float64 values and colours.  trim and transfer centre on the scan's box and
simplify has its own reader: they are not served here.
"""
import numpy as np
import torch

from . import _lib, meshio, topology

LIMITS = {'faces': 1, 'corners': 3}            # what to_device counts against 2^31 - 1 next to the vertices: nf, or the 3 nf corners


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


class Mesh:
    """The record of `load`: path, verts float64 [nv,3] as read, faces int64 [nf,3], colors uint8 [nv,c] or None, double (the file stores
    doubles), centre float64 [3] of the mesh's own box and local32, the centred float32 host copy."""

    def __init__(self, path, verts, faces, colors, double):
        self.path, self.verts, self.colors, self.double = path, verts, colors, double
        self.centre = meshio.box_centre(verts)
        self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        self.local32 = meshio.centred_f32(verts, self.centre)

    def to_device(self, limit=None):
        """(local f32 [nv,3], f int64 [nf,3]) on the GPU.  limit 'faces' / 'corners': SystemExit when the vertices or the faces / the
        3 nf corners do not fit an int32."""
        dev = torch.device('cuda')
        local, f = torch.from_numpy(self.local32).to(dev), torch.from_numpy(self.faces).to(dev)
        if limit is not None and (local.shape[0] > topology.MAX_COUNT or LIMITS[limit] * f.shape[0] > topology.MAX_COUNT):
            raise SystemExit('{} has more than 2^31 - 1 vertices or {}'.format(self.path, limit))
        return local, f

    def _colors(self, rows):
        return None if self.colors is None else np.asarray(self.colors)[rows]

    def write_as_read(self, out_file, faces=None, normals=None):
        """The vertices and colours as read, with other faces (re-wound ones) or with normals when given."""
        meshio.write_ply_mesh(out_file, self.verts, self.faces if faces is None else _host(faces), double=self.double,
                              normals=None if normals is None else _host(normals), colors_u8=self.colors)

    def write_rows(self, out_file, rows, out_f):
        """The vertices and colours as read, gathered through `rows` (kept rows, or source rows with repeats), with the faces out_f."""
        rows = _host(rows)
        meshio.write_ply_mesh(out_file, self.verts[rows], _host(out_f), double=self.double, colors_u8=self._colors(rows))

    def write_moved(self, out_file, out_v):
        """The positions out_v f32 [nv,3] of the centred frame put back on the centre in float64; faces and colours as read."""
        meshio.write_ply_mesh(out_file, _host(out_v).astype(np.float64) + self.centre[None], self.faces, double=self.double,
                              colors_u8=self.colors)

    def write_origin(self, out_file, origin, out_v, out_f, colors):
        """The mesh out_v f32 / out_f of a stage that drops, moves and adds vertices: origin int64 [nv out] is the row as read of every
        output vertex, -1 for one the stage made.  A vertex whose float32 bytes equal those of its origin row is written as read, every
        other one from its float32 position put back on the centre; colors (uint8 [nv out, c] or None) are the caller's."""
        origin, out_v = _host(origin), _host(out_v)
        same = origin >= 0
        same[same] = (out_v[same].view(np.int32) == self.local32[origin[same]].view(np.int32)).all(axis=1)
        pos = out_v.astype(np.float64) + self.centre[None]
        pos[same] = np.asarray(self.verts, dtype=np.float64)[origin[same]]
        meshio.write_ply_mesh(out_file, pos, _host(out_f), double=self.double, colors_u8=colors)


def load(path, prog, reader=None):
    """The Mesh of a command's input: need_gpu(prog), the read (meshio.read_mesh_file unless a reader is given), the finite check."""
    _lib.need_gpu(prog)
    verts, faces, colors, double = (reader or meshio.read_mesh_file)(path)
    if not np.isfinite(verts).all():
        raise SystemExit('{} has non-finite vertices'.format(path))
    return Mesh(path, verts, faces, colors, double)
