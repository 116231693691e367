"""numpy restatement of the manifold split (ppsurf_amd/csrc/pps_manifold.hip, ppsurf_amd/manifold.py): the specification
the GPU is held to, byte for byte, and the fixtures of its tests.  Nothing here comes from the device and nothing from the module: the
pairs come from a dictionary of edge owners and the fans from a plain sequential union-find over corners.

Rule: corner c = 3 f + k of a valid face f (indices in [0, nv), pairwise distinct) names the vertex faces[f, k]; the corners of an invalid
face have the label -1 and take no part.  For every undirected edge that exactly two valid faces hold, with its slot in each (slot k is
corner k -> corner k + 1 mod 3), the corner of the one face and the corner of the other that name the same end of the edge are linked, for
both ends.  A fan is a connected component of the links, its leader its smallest corner, label[c] the leader of c's fan.  At vertex v the
fan with the smallest leader keeps row v; every other fan gets a new row after the nv given ones, in ascending order of fan leader, with
v's position; source is the given row of every output row.  Every corner of a valid face is renamed to its fan's row; an invalid face is
copied; order and winding stay.  When no vertex has a second fan the arrays come back as given.
"""
import numpy as np

import decimate_spec
import orient_spec
import pieces_spec
import simplify_spec
from topology_spec import valid_faces


def pair_list(faces, nv):
    """(fa, fb, ea, eb int64 [np]): the two owners of every undirected edge that exactly two valid faces hold and the slot of the edge in
    each.  The order of the pairs and which owner comes first mean nothing."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    owners = {}
    for t in np.nonzero(valid_faces(f, nv))[0].tolist():
        row = f[t].tolist()
        for k in range(3):
            u, w = row[k], row[(k + 1) % 3]
            owners.setdefault((min(u, w), max(u, w)), []).append((t, k))
    two = [held for held in owners.values() if len(held) == 2]
    cols = [[held[i][j] for held in two] for i, j in ((0, 0), (1, 0), (0, 1), (1, 1))]
    return tuple(np.array(c, dtype=np.int64) for c in cols)


def owner_counts(faces, nv):
    """int64 [ne]: the number of valid faces on every distinct undirected edge of the valid faces."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, nv)]
    if f.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1].astype(np.int64)


def start_labels(faces, nv):
    """int32 [3 nf]: c for the corners of the valid faces, -1 for the others."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = np.repeat(valid_faces(f, nv), 3)
    return np.where(ok, np.arange(3 * f.shape[0]), -1).astype(np.int32)


def fans_of_pairs(faces, nv, fa, fb, ea, eb, start=None):
    """int32 [3 nf]: the fixed point of the hooking rounds over a given pair list from the labels `start` (each its own index or
    negative; start_labels when None).  A pair with a face outside [0, nf), a slot outside [0, 3), a corner vertex outside [0, nv) or
    slots that name no common edge is skipped, and so is a link onto a corner with a negative label.  The smaller root wins a union, so
    a root is the smallest corner of its class."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nf = f.shape[0]
    start = start_labels(f, nv) if start is None else np.asarray(start, dtype=np.int32)
    live = start >= 0
    assert (start[live] == np.arange(3 * nf)[live]).all()
    parent = list(range(3 * nf))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, sa, sb in zip(np.asarray(fa).tolist(), np.asarray(fb).tolist(), np.asarray(ea).tolist(), np.asarray(eb).tolist()):
        if not (0 <= a < nf and 0 <= b < nf and 0 <= sa < 3 and 0 <= sb < 3):
            continue
        ta, tb = (sa + 1) % 3, (sb + 1) % 3
        a0, a1, b0, b1 = int(f[a, sa]), int(f[a, ta]), int(f[b, sb]), int(f[b, tb])
        if not all(0 <= i < nv for i in (a0, a1, b0, b1)):
            continue
        if a0 == b0 and a1 == b1:
            links = ((3 * a + sa, 3 * b + sb), (3 * a + ta, 3 * b + tb))
        elif a0 == b1 and a1 == b0:
            links = ((3 * a + sa, 3 * b + tb), (3 * a + ta, 3 * b + sb))
        else:
            continue
        for x, y in links:
            if live[x] and live[y]:
                rx, ry = find(x), find(y)
                if rx != ry:
                    parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(c) if live[c] else start[c] for c in range(3 * nf)], dtype=np.int32).reshape(-1)


def fans_spec(faces, nv):
    """int32 [3 nf]: the leader of every corner's fan, -1 for the corners of an invalid face."""
    return fans_of_pairs(faces, nv, *pair_list(faces, nv))


def rows_spec(faces, nv, label):
    """(newrow int64 [3 nf], source int64 [nv_out], fans int64 [nv]): the leaders in ascending order; the first at a vertex keeps its
    row, every later one gets the next new row.  newrow is the identity away from the leaders (never read)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1)
    newrow = np.arange(label.shape[0], dtype=np.int64)
    source, fans = list(range(nv)), np.zeros(nv, dtype=np.int64)
    for l in np.nonzero(label == np.arange(label.shape[0]))[0].tolist():
        v = int(f[l])
        newrow[l] = v if fans[v] == 0 else len(source)
        if fans[v] > 0:
            source.append(v)
        fans[v] += 1
    return newrow, np.array(source, dtype=np.int64), fans


def faces_spec(faces, nv, label, newrow, nv_out):
    """int64 [nf,3]: the face kernel's table.  Corner c of a face that is valid as given becomes newrow[label[c]] when label[c] >= 0 and
    keeps its entry when it is negative; a face that is invalid as given, has a label >= 3 nf or a new entry outside [0, nv_out) is
    copied."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out = f.copy()
    for t in np.nonzero(valid_faces(f, nv))[0].tolist():
        row = f[t].tolist()
        for k in range(3):
            l = int(label[3 * t + k])
            if l >= 3 * f.shape[0]:
                row = None
                break
            if l >= 0:
                row[k] = int(newrow[l])
        if row is not None and all(0 <= i < nv_out for i in row):
            out[t] = row
    return out


def split_spec(verts, faces):
    """(verts out, faces out, info, parts): the split.  parts: `label`, `newrow`, `source`, `fans` and `same`, whether the arrays come
    back as given."""
    v, f = np.asarray(verts), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    label = fans_spec(f, nv)
    newrow, source, fans = rows_spec(f, nv, label)
    same = source.shape[0] == nv
    out_f = f if same else faces_spec(f, nv, label, newrow, source.shape[0])
    before, after = owner_counts(f, nv), owner_counts(out_f, source.shape[0])
    valid = int(valid_faces(f, nv).sum())
    info = {'vertices_in': nv, 'vertices_out': int(source.shape[0]), 'vertices_split': int((fans >= 2).sum()),
            'max_fans': int(fans.max()) if nv else 0, 'faces_in': nf, 'faces_valid': valid,
            'edges_border_in': int((before == 1).sum()), 'edges_border_out': int((after == 1).sum()),
            'edges_manifold_in': int((before == 2).sum()), 'edges_manifold_out': int((after == 2).sum()),
            'edges_nonmanifold_in': int((before >= 3).sum()), 'closed_out': bool(2 * int((after == 2).sum()) == 3 * valid)}
    return (v if same else v[source]), out_f, info, {'label': label, 'newrow': newrow, 'source': source, 'fans': fans, 'same': same}


def check(verts, faces, out):
    """The postconditions of out = (verts out, faces out, source) for the mesh (verts, faces)."""
    v, f = np.asarray(verts), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out_v, out_f, source = out
    ok = valid_faces(f, v.shape[0])
    assert out_f.shape == f.shape and out_f.dtype == np.int64 and out_v.dtype == v.dtype and out_v.shape == (source.shape[0], 3)
    assert source[:v.shape[0]].tolist() == list(range(v.shape[0])) and out_v.tobytes() == v[source].tobytes()
    after = owner_counts(out_f, out_v.shape[0])
    assert after.shape[0] == 0 or after.max() <= 2                                            # no edge with more than two valid owners
    assert np.array_equal(valid_faces(out_f, out_v.shape[0]), ok) and np.array_equal(out_f[~ok], f[~ok])
    assert np.array_equal(source[out_f[ok]], f[ok])                                           # the faces, mapped back, are the given ones
    assert out_v[out_f[ok]].tobytes() == v[f[ok]].tobytes()                                   # no corner moved
    again_v, again_f, info, parts = split_spec(out_v, out_f)                                  # idempotent: one fan per vertex now
    assert parts['same'] and again_v.tobytes() == out_v.tobytes() and again_f.tobytes() == out_f.tobytes()
    assert info['vertices_split'] == 0 and info['max_fans'] <= 1 and info['vertices_out'] == out_v.shape[0]
    assert info['edges_nonmanifold_in'] == 0


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------

INVALID = orient_spec.INVALID
SHUFFLE_SEED = 41


def bow_tie():
    """Two triangles that share vertex 0 and nothing else."""
    verts = np.array([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]], dtype=np.float32)
    return verts, np.array([[0, 1, 2], [0, 3, 4]], dtype=np.int64)


def three_tetrahedra():
    """Three tetrahedra that share vertex 0 and nothing else: a vertex with three closed fans."""
    tv, tf = orient_spec.tetra()
    verts, faces = [np.zeros((1, 3), dtype=np.float32)], []
    for i, axis in enumerate(np.eye(3, dtype=np.float32)):
        verts.append(tv[1:] * 0.25 + axis[None] - 0.1)                                       # three private corners per tetrahedron
        rename = np.array([0, 3 * i + 1, 3 * i + 2, 3 * i + 3], dtype=np.int64)
        faces.append(rename[tf])
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces)


def book():
    """Three pages on the spine (0, 1), every page running it the same way."""
    verts = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 1, 0.5], [-0.5, -1, 0.5]], dtype=np.float32)
    return verts, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], dtype=np.int64)


def simplified(name, G):
    """(verts f32, faces) of the vertex clustering of a closed mesh on a coarse grid, by simplify_spec: it has many-owner edges."""
    verts, faces = orient_spec.sphere() if name == 'sphere' else decimate_spec.torus(32, 16)
    out = simplify_spec.simplify(verts, faces, G)
    return out['verts'].astype(np.float32), np.ascontiguousarray(out['faces'], dtype=np.int64)


def base(name):
    """(verts f32, faces int64) of a named mesh as built."""
    if name in pieces_spec.SMALL:
        return pieces_spec.small(name)[:2]
    if name in ('moebius', 'klein', 'sphere', 'torus'):
        return orient_spec.case(name)
    if name == 'bow-tie':
        return bow_tie()
    if name == 'three tetrahedra':
        return three_tetrahedra()
    if name == 'book':
        return book()
    if name == 'simplified sphere 6':
        return simplified('sphere', 6)
    if name == 'simplified torus 4':
        return simplified('torus', 4)
    assert name == 'simplified torus 8'
    return simplified('torus', 8)


BASES = pieces_spec.SMALL + ('bow-tie', 'three tetrahedra', 'book', 'moebius', 'klein', 'sphere', 'torus', 'simplified sphere 6',
                             'simplified torus 4', 'simplified torus 8')
CLOSED = ('klein', 'sphere', 'torus')                                   # closed manifolds: the same arrays come back
_built = {}


def case(name):
    """(verts f32, faces int64) of a named case: a base mesh, `NAME invalid` (the rows of INVALID interleaved), `NAME shuffled` (the faces
    permuted by a seed: which copy keeps row v follows the face order), the empty mesh, a mesh of invalid faces only, and a strip of
    1 025 faces in three orders."""
    if name not in _built:
        if name == 'empty':
            got = orient_spec.tetra()[0], np.zeros((0, 3), dtype=np.int64)
        elif name == 'all invalid':
            got = orient_spec.tetra()[0], INVALID.copy()
        elif name.startswith('strip '):
            got = pieces_spec.strip(1025, name[len('strip '):])
        elif name.endswith(' invalid'):
            verts, faces = case(name[:-len(' invalid')])
            n = faces.shape[0]
            got = verts, orient_spec.with_invalid(faces, at=(0, n // 2 + 1, n + 2))              # in front, in the middle, at the end
        elif name.endswith(' shuffled'):
            verts, faces = case(name[:-len(' shuffled')])
            got = verts, faces[np.random.default_rng(SHUFFLE_SEED).permutation(faces.shape[0])]
        else:
            got = base(name)
        _built[name] = (np.ascontiguousarray(got[0], dtype=np.float32), np.ascontiguousarray(got[1], dtype=np.int64))
    return _built[name]


CASES = tuple(n + tail for n in BASES for tail in ('', ' invalid', ' shuffled')) + ('empty', 'all invalid', 'strip ascending', 'strip reversed',
                                                                                 'strip permuted')
