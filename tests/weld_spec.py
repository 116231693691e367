"""numpy restatement of the weld stage (ppsurf_amd/csrc/pps_weld.hip, ppsurf_amd/weld.py): the specification the GPU
is held to, byte for byte, and the fixtures of its tests.  Nothing here comes from the device, and nothing here knows a grid.

Rule: on the f32 vertices widened to fp64, rows i != j are linked when ((dx dx + dy dy) + dz dz) <= eps2, d* = p_i* - p_j*, eps2 = eps * eps,
every operation one rounded fp64 operation.  The clusters are the connected components of the links (single linkage), the leader of a cluster
is its smallest row.  Vertices out: the leaders in ascending row, byte for byte.  Every face gets a code: 1 invalid as given (an index outside
[0, nv) or two equal indices), 2 valid as given with two corners in one cluster, 0 kept; the kept faces come in their given order, corners
renumbered, winding untouched.  With drop_duplicates the kept faces with one set of three new indices collapse to the first of them.  The
mesh comes back as given when no two rows are linked and either no face is valid or every face is valid and no duplicate is dropped.
"""
import struct

import numpy as np

from topology_spec import valid_faces

D = np.float64
BLOCK = 512                                                             # rows per block of the all-pairs distance table


def linked_pairs(verts, eps):
    """(i, j int64 [nl]), i > j: every linked pair, by brute force over all pairs."""
    p = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(D)
    eps2 = D(eps) * D(eps)
    hi, lo = [], []
    for at in range(0, p.shape[0], BLOCK):
        d = p[at:at + BLOCK, None, :] - p[None, :at + BLOCK, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i, j = np.nonzero(d2 <= eps2)
        i = i + at
        hi.append(i[i > j])
        lo.append(j[i > j])
    none = np.zeros(0, dtype=np.int64)
    return np.concatenate(hi + [none]).astype(np.int64), np.concatenate(lo + [none]).astype(np.int64)


def clusters_of_pairs(nv, hi, lo):
    """leader int32 [nv] of the given links between the rows 0 .. nv - 1: a union by smallest row."""
    parent = list(range(nv))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(np.asarray(hi).tolist(), np.asarray(lo).tolist()):
        a, b = root(i), root(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([root(x) for x in range(nv)], dtype=np.int32).reshape(nv)


def clusters_spec(verts, eps=0.0):
    """leader int32 [nv]: the smallest row of every row's cluster."""
    return clusters_of_pairs(np.asarray(verts).reshape(-1, 3).shape[0], *linked_pairs(verts, eps))


def faces_spec(faces, nv, newrow):
    """(out int64 [nf,3], code uint8 [nf]) of ppsx_weld_faces: code 1 for a face that is invalid as given or has a newrow entry outside
    [0, nv), 2 for a valid one with two equal new indices, 0 for a kept one; only the kept rows are renumbered."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    newrow = np.asarray(newrow, dtype=np.int64).reshape(-1)
    ok = valid_faces(f, nv)
    new = np.where(ok[:, None], newrow[np.where(ok[:, None], f, 0)], -1) if nv > 0 else np.full(f.shape, -1, dtype=np.int64)
    ok = ok & ((new >= 0) & (new < nv)).all(axis=1)
    flat = (new[:, 0] == new[:, 1]) | (new[:, 1] == new[:, 2]) | (new[:, 2] == new[:, 0])
    code = np.where(~ok, 1, np.where(flat, 2, 0)).astype(np.uint8)
    return np.where((code == 0)[:, None], new, f), code


def weld_spec(verts, faces, eps=0.0, drop_duplicates=False):
    """(verts f32, faces int64, info, parts): weld.weld_mesh, and parts = {leader int32 [nv], rows int64 (the leaders ascending), code uint8
    [nf], same (the mesh comes back as given)}."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    leader = clusters_spec(v, eps)
    leads = leader == np.arange(nv)
    rows = np.nonzero(leads)[0].astype(np.int64)
    sizes = np.bincount(leader, minlength=nv)
    newrow = (np.cumsum(leads) - 1)[leader]
    out, code = faces_spec(f, nv, newrow)
    kept = out[code == 0]
    valid, duplicate = kept.shape[0], 0
    if drop_duplicates:
        seen, first = set(), np.ones(valid, dtype=bool)
        for k, row in enumerate(np.sort(kept, axis=1).tolist()):
            first[k] = tuple(row) not in seen
            seen.add(tuple(row))
        kept = kept[first]
        duplicate = valid - kept.shape[0]
    invalid = int((code == 1).sum())
    info = {'vertices_in': int(nv), 'vertices_out': int(rows.shape[0]), 'clusters_merged': int((sizes >= 2).sum()),
            'largest_cluster': int(sizes.max()) if nv else 0, 'faces_in': int(nf), 'faces_invalid': invalid,
            'faces_collapsed': int((code == 2).sum()), 'faces_duplicate': int(duplicate), 'faces_out': int(kept.shape[0]), 'eps': float(eps),
            'drop_duplicates': bool(drop_duplicates)}
    same = rows.shape[0] == nv and (valid == 0 or (invalid == 0 and duplicate == 0))
    parts = {'leader': leader, 'rows': rows, 'code': code, 'same': bool(same)}
    if same:
        info['faces_out'] = int(nf)
        return v, f, info, parts
    return v[rows], kept, info, parts


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------

INVALID = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 1 << 40]], dtype=np.int64)
CHAIN_EPS = 0.125                                                       # the chains are spaced 0.9 of it


def soup(verts, faces, seed):
    """(verts f32 [3 nf,3], faces [nf,3], first int64 [nv]): every face gets private copies of its corners and the rows are shuffled
    (default_rng(seed)); first[u] is the smallest soup row that copies vertex u (3 nf for a vertex no face holds)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = 3 * f.shape[0]
    place = np.random.default_rng(seed).permutation(n)                  # corner k lives in row place[k]
    out = np.empty((n, 3), dtype=np.float32)
    out[place] = v[f.reshape(-1)]
    first = np.full(v.shape[0], n, dtype=np.int64)
    np.minimum.at(first, f.reshape(-1), place)
    return out, place.reshape(-1, 3).astype(np.int64), first


def welded_soup(verts, faces, first):
    """(verts, faces) that the weld at eps = 0 must give for soup(verts, faces, seed) of a mesh whose vertices are pairwise distinct and
    all referenced: the vertices in the order of their first copy, the faces renumbered to it."""
    order = np.argsort(first, kind='stable')
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return np.asarray(verts, dtype=np.float32)[order], rank[np.asarray(faces, dtype=np.int64)]


def chain(n, order='ascending'):
    """verts f32 [n,3]: points on a line spaced 0.9 CHAIN_EPS (dyadic steps would tie; these do not), as given, reversed or shuffled."""
    x = (np.arange(n, dtype=D) * (0.9 * CHAIN_EPS)).astype(np.float32)
    if order == 'reversed':
        x = x[::-1]
    elif order == 'shuffled':
        x = x[np.random.default_rng(61).permutation(n)]
    else:
        assert order == 'ascending'
    return np.stack([x, np.full_like(x, 0.5), np.full_like(x, -0.25)], axis=1).astype(np.float32)


def tetra_soup():
    """(verts f32 [12,3], faces [4,3]): the tetrahedron of orient_spec as an STL stores it, three private corners per facet."""
    import orient_spec
    verts, faces = orient_spec.tetra()
    return verts[faces.reshape(-1)].copy(), np.arange(12, dtype=np.int64).reshape(4, 3)


def tetra_stl(path, ascii_):
    """Writes the outward tetrahedron as an STL and returns its corners float32 [12,3] in file order."""
    import orient_spec
    verts, faces = orient_spec.tetra()
    corners = verts[faces]                                             # [4,3,3]
    if ascii_:
        with open(path, 'w') as f:
            f.write('solid tetra\n')
            for tri in corners:
                f.write(' facet normal 0 0 0\n  outer loop\n')
                for p in tri:
                    f.write('   vertex {:.9g} {:.9g} {:.9g}\n'.format(*p.tolist()))
                f.write('  endloop\n endfacet\n')
            f.write('endsolid tetra\n')
    else:
        with open(path, 'wb') as f:
            f.write(b'solid binary all the same'.ljust(80, b' ') + struct.pack('<I', 4))
            for tri in corners:
                f.write(struct.pack('<12fH', 0.0, 0.0, 0.0, *tri.reshape(-1).tolist(), 0))
    return corners.reshape(12, 3)


def twins():
    """(verts f32 [9,3], faces [3,3]): a triangle three times over private corners: as given, rotated (same winding), mirrored."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    return np.concatenate([tri, tri[[1, 2, 0]], tri[[0, 2, 1]]]), np.arange(9, dtype=np.int64).reshape(3, 3)


def case(name):
    """(verts f32, faces int64, eps) of a named test mesh."""
    import orient_spec
    none = np.zeros((0, 3), dtype=np.int64)
    if name in ('sphere soup', 'cube soup', 'torus soup'):
        verts, faces = orient_spec.case(name.split(' ')[0])              # the scrambled winding: the weld must leave it alone
        return soup(verts, faces, SEEDS[name])[:2] + (0.0,)
    if name == 'sphere soup jitter':                                   # the copies moved by less than eps, eps far below the shortest edge
        verts, faces, _ = case('sphere soup')
        move = np.random.default_rng(62).uniform(-1.0, 1.0, verts.shape) * 1.0e-4
        return (verts.astype(D) + move).astype(np.float32), faces, 1.0e-3
    if name == 'tetra soup':
        return tetra_soup() + (0.0,)
    if name == 'tetra soup invalid':
        verts, faces = tetra_soup()
        return verts, np.concatenate([INVALID[:1], faces[:2], INVALID[1:2], faces[2:], INVALID[2:]]), 0.0
    if name == 'signed zeros':
        return np.array([[0.0, 0.0, 1.0], [-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [1.0, 0.0, 0.0]], dtype=np.float32), none, 0.0
    if name == '3-4-5 linked':
        return np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float32), none, 5.0
    if name == '3-4-5 apart':
        return np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float32), none, float(np.nextafter(5.0, 0.0))
    if name == 'chain 5':
        return chain(5), np.array([[0, 1, 4]], dtype=np.int64), CHAIN_EPS
    if name in ('chain 1025', 'chain 1025 reversed', 'chain 1025 shuffled'):
        return chain(1025, (name.split(' ') + ['ascending'])[2]), none, CHAIN_EPS
    if name == 'collapsed':                                              # rows 1 and 4 are one point: face 1 loses an edge, face 0 does not
        verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float32)
        return verts, np.array([[0, 1, 2], [1, 4, 3], [0, 4, 3]], dtype=np.int64), 0.0
    if name in ('twins', 'twins dropped'):
        return twins() + (0.0,)
    if name == 'unreferenced':                                           # rows 3 and 5 are one point that no face holds; row 4 is alone
        verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [7, 7, 7], [8, 8, 8], [7, 7, 7], [0, 0, 0]], dtype=np.float32)
        return verts, np.array([[0, 1, 2], [6, 2, 1]], dtype=np.int64), 0.0
    if name == 'crowd':                                                  # 300 copies of one point: one cell, an extent of 0
        return np.tile(np.array([[0.3, -1.7, 2.5]], dtype=np.float32), (300, 1)), none, 0.0
    if name == 'crowd eps':
        return case('crowd')[0], none, 0.01
    if name == 'single':
        return np.array([[1.0, 2.0, 3.0]], dtype=np.float32), none, 0.5
    if name == 'welded sphere':                                          # nothing to do
        return orient_spec.sphere() + (0.0,)
    if name == 'welded sphere invalid':
        verts, faces = orient_spec.sphere()
        return verts, orient_spec.with_invalid(faces), 0.0
    if name == 'all invalid':
        return orient_spec.tetra()[0], INVALID.copy(), 0.0
    if name == 'all invalid merged':
        return np.zeros((4, 3), dtype=np.float32), INVALID.copy(), 0.0
    if name == 'cloud':
        pts = np.random.default_rng(63).integers(0, 6, size=(700, 3)).astype(np.float32)          # a lattice: many coincident rows
        return pts, none, 0.0
    if name == 'cloud eps':                                              # eps = 1: the lattice neighbours chain into one cluster
        return case('cloud')[0], none, 1.0
    assert name == 'empty'
    return np.zeros((0, 3), dtype=np.float32), none, 0.0


SEEDS = {'sphere soup': 71, 'cube soup': 72, 'torus soup': 73}
DROP = ('twins dropped',)                                               # the cases that run with drop_duplicates
CASES = ('sphere soup', 'cube soup', 'torus soup', 'sphere soup jitter', 'tetra soup', 'tetra soup invalid', 'signed zeros', '3-4-5 linked',
         '3-4-5 apart', 'chain 5', 'chain 1025', 'chain 1025 reversed', 'chain 1025 shuffled', 'collapsed', 'twins', 'twins dropped',
         'unreferenced', 'crowd', 'crowd eps', 'single', 'welded sphere', 'welded sphere invalid', 'all invalid', 'all invalid merged', 'cloud',
         'cloud eps', 'empty')
