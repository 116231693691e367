"""numpy restatement of the removal of isolated pieces (ppsurf_amd/csrc/pps_pieces.hip, ppsurf_amd/pieces.py): the
specification the GPU is held to, byte for byte, and the fixtures of its tests.  Nothing here comes from the device.

Rule: a face is valid when its three indices lie in [0, nv) and are pairwise distinct; an invalid face has the label -1, belongs to no
component and is always dropped.  Two valid faces are adjacent when they share an undirected edge that exactly two valid faces hold (one
owner, or three and more, joins nothing; a duplicated face is two faces).  A component is a class of the transitive closure; its leader is
its smallest face index; label[f] is the leader of f's component; components are numbered in ascending leader.  The table: faces (the
count), lo and hi (the f32 box of the corners, every coordinate taken as x + 0.0f), diag2 = (dx dx + dy dy) + dz dz in fp64 on the widened
box, and D2, the same over the box of all components (0 without one).  Rules, each optional, all that are given must pass: min_faces = N,
faces >= N; min_diag_frac = F, diag2 >= (F F) D2; keep_largest = K, rank < K by faces descending, then leader ascending, over all
components.  Output: the kept faces in their order, the vertices no kept face references dropped, the faces re-indexed.  A mesh without a
valid face comes back as given.
"""
import numpy as np

import denoise_spec
import smooth_spec
from topology_spec import SENTINEL, valid_faces

D = np.float64


def edge_keys(faces, nv):
    """int64 [3 nf]: (min << 32) | max of ab, bc, ca per face (a, b, c), in that order; INT64_MAX three times for an invalid face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    keys = np.stack([(np.minimum(a, b) << 32) | np.maximum(a, b), (np.minimum(b, c) << 32) | np.maximum(b, c),
                     (np.minimum(c, a) << 32) | np.maximum(c, a)], axis=1)
    keys[~valid_faces(f, nv)] = SENTINEL
    return keys.reshape(-1)


def pairs(faces, nv):
    """A set of (smaller face, larger face): the owners of every edge that exactly two valid faces hold."""
    keys = edge_keys(faces, nv)
    order = np.argsort(keys, kind='stable')
    uniq, first, counts = np.unique(keys[order], return_index=True, return_counts=True)
    first = first[(counts == 2) & (uniq != SENTINEL)]
    a, b = order[first] // 3, order[first + 1] // 3
    return set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))


def labels_spec(faces, nv):
    """int32 [nf]: the leader of every valid face's component, -1 for an invalid face.  A sequential union-find over the owners of every
    edge; the smaller root wins a union, so a root is the smallest index of its class."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(f, nv)
    parent = list(range(f.shape[0]))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    owners = {}
    for t in np.nonzero(ok)[0].tolist():
        a, b, c = f[t].tolist()
        for u, w in ((a, b), (b, c), (c, a)):
            owners.setdefault((min(u, w), max(u, w)), []).append(t)
    for held in owners.values():
        if len(held) == 2:
            ra, rb = find(held[0]), find(held[1])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(t) if ok[t] else -1 for t in range(f.shape[0])], dtype=np.int32).reshape(-1)


def diag2_of(lo, hi):
    d = np.asarray(hi, dtype=np.float32).astype(D) - np.asarray(lo, dtype=np.float32).astype(D)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def table_spec(verts, faces):
    """{label int32 [nf], leader int64 [nc], faces int64 [nc], lo, hi f32 [nc,3], diag2 f64 [nc], box_diag2 float, cid int64 [nf]}."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = labels_spec(f, v.shape[0])
    leader = np.unique(label[label >= 0]).astype(np.int64)
    nc = leader.shape[0]
    cid = np.where(label >= 0, np.searchsorted(leader, label), -1).astype(np.int64)
    live = np.nonzero(label >= 0)[0]
    count = np.bincount(cid[live], minlength=nc).astype(np.int64)
    lo, hi = np.full((nc, 3), np.inf, dtype=np.float32), np.full((nc, 3), -np.inf, dtype=np.float32)
    corners = v[f[live]] + np.float32(0.0)                            # [live,3,3]; -0.0 becomes +0.0
    np.minimum.at(lo, cid[live], corners.min(axis=1))
    np.maximum.at(hi, cid[live], corners.max(axis=1))
    box = float(diag2_of(lo.min(axis=0), hi.max(axis=0))) if nc else 0.0
    return {'label': label, 'leader': leader, 'faces': count, 'lo': lo, 'hi': hi, 'diag2': diag2_of(lo, hi).reshape(-1), 'box_diag2': box, 'cid': cid}


def rank_spec(count):
    """int64 [nc]: the place by faces descending, then leader ascending."""
    order = np.argsort(-np.asarray(count, dtype=np.int64), kind='stable')
    rank = np.empty(order.shape[0], dtype=np.int64)
    rank[order] = np.arange(order.shape[0])
    return rank


def select_spec(table, min_faces=None, min_diag_frac=None, keep_largest=None):
    """bool [nc]: the components that pass every rule given."""
    assert not (min_faces is None and min_diag_frac is None and keep_largest is None)
    keep = np.ones(table['leader'].shape[0], dtype=bool)
    if min_faces is not None:
        keep &= table['faces'] >= int(min_faces)
    if min_diag_frac is not None:
        keep &= table['diag2'] >= (D(min_diag_frac) * D(min_diag_frac)) * D(table['box_diag2'])
    if keep_largest is not None:
        keep &= rank_spec(table['faces']) < int(keep_largest)
    return keep


def remove_spec(verts, faces, min_faces=None, min_diag_frac=None, keep_largest=None):
    """(verts f32, faces int64, info, kept leaders): pieces.remove_pieces and the leaders of the components it keeps."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    table = table_spec(v, f)
    nc = table['leader'].shape[0]
    info = {'faces_in': int(f.shape[0]), 'faces_valid': int((table['label'] >= 0).sum()), 'faces_out': int(f.shape[0]),
            'vertices_in': int(v.shape[0]), 'vertices_out': int(v.shape[0]), 'components': int(nc), 'components_kept': 0, 'largest_faces': 0,
            'box_diag2': table['box_diag2'], 'min_faces': min_faces, 'min_diag_frac': min_diag_frac, 'keep_largest': keep_largest}
    if nc == 0:
        return v, f, info, []
    keep = select_spec(table, min_faces, min_diag_frac, keep_largest)
    cid = table['cid']
    kept = f[(cid >= 0) & keep[np.maximum(cid, 0)]]
    used = np.zeros(v.shape[0], dtype=bool)
    used[kept.reshape(-1)] = True
    out_f = (np.cumsum(used) - 1)[kept].reshape(-1, 3).astype(np.int64)
    info.update(faces_out=int(out_f.shape[0]), vertices_out=int(used.sum()), components_kept=int(keep.sum()), largest_faces=int(table['faces'].max()))
    return v[used], out_f, info, table['leader'][keep].tolist()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------

def moved(n, off, s=1.0):
    """(verts f32, faces): denoise_spec.cube(n) scaled by s and shifted by off."""
    verts, faces, _ = denoise_spec.cube(n)
    return (verts * s + np.asarray(off, dtype=D)[None]).astype(np.float32), faces


def joined(parts):
    """(verts, faces) of meshes put one after another."""
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + base)
        base += v.shape[0]
    return np.concatenate(verts), np.concatenate(faces)


SCENE_PARTS = ((8, (0, 0, 0), 1.0), (4, (12, 12, 12), 1.0), (2, (12, 0, 0), 1.0), (2, (0, 12, 0), 1.0), (1, (0, 0, 12), 1.0), (4, (12, 0, 12), 0.5))
SCENE_FACES = {0: 768, 768: 192, 960: 48, 1008: 48, 1056: 12, 1068: 192}          # leader: faces, as built
SCENE_DIAG2 = {0: 192.0, 768: 48.0, 960: 12.0, 1008: 12.0, 1056: 3.0, 1068: 12.0}
# (rules, the leaders kept, as built)
SCENE_GRID = (
    ((None, 0.5, None), [0]),
    ((None, float(np.nextafter(0.5, 1.0)), None), []),
    ((None, 0.25, None), [0, 768]),
    ((None, 0.125, None), [0, 768, 960, 1008, 1068]),
    ((None, 0.0, None), [0, 768, 960, 1008, 1056, 1068]),
    ((None, 1.0, None), []),
    ((48, None, None), [0, 768, 960, 1008, 1068]),
    ((49, None, None), [0, 768, 1068]),
    ((None, None, 2), [0, 768]),
    ((None, None, 3), [0, 768, 1068]),
    ((None, None, 6), [0, 768, 960, 1008, 1056, 1068]),
    ((None, None, 7), [0, 768, 960, 1008, 1056, 1068]),
    ((13, 0.125, 3), [0, 768, 1068]),
)
SCENE_INVALID = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 642]], dtype=np.int64)


def scene(order='built'):
    """(verts f32 [642,3], faces int64): six cubes apart from one another.  order: 'built', 'robin' (round-robin across the six pieces, so
    that the leaders are 0..5 and every wave mixes components), 'permuted' (default_rng(11)) or 'invalid' (as built with the three rows of
    SCENE_INVALID after face 300)."""
    parts = [moved(n, off, s) for n, off, s in SCENE_PARTS]
    verts, faces = joined(parts)
    if order == 'robin':
        starts = np.cumsum([0] + [f.shape[0] for _, f in parts])
        turn = [starts[p] + i for i in range(768) for p in range(6) if i < parts[p][1].shape[0]]
        faces = faces[np.array(turn)]
    elif order == 'permuted':
        faces = faces[np.random.default_rng(11).permutation(faces.shape[0])]
    elif order == 'invalid':
        faces = np.concatenate([faces[:301], SCENE_INVALID, faces[301:]])
    else:
        assert order == 'built'
    return verts, faces


def cube8(prefix=768):
    verts, faces = moved(8, (0, 0, 0))
    return verts, faces[:prefix]


def strip(n, order='ascending'):
    """(verts f32 [n + 2,3], faces (i, i + 1, i + 2)): one chain of n faces, ascending, reversed or permuted (default_rng(3))."""
    i = np.arange(n, dtype=np.int64)
    faces = np.stack([i, i + 1, i + 2], axis=1)
    j = np.arange(n + 2)
    verts = np.stack([j * 0.5, j % 2, np.zeros(n + 2)], axis=1).astype(np.float32)
    if order == 'reversed':
        faces = faces[::-1].copy()
    elif order == 'permuted':
        faces = faces[np.random.default_rng(3).permutation(n)]
    else:
        assert order == 'ascending'
    return verts, faces


def debris():
    """(verts, faces): about half the faces of smooth_spec.noisy_sphere(): 672 faces in 158 components."""
    verts, faces = smooth_spec.noisy_sphere()
    return verts, faces[np.random.default_rng(5).random(faces.shape[0]) < 0.5]


def fins():
    """Three faces on one edge: the edge has three owners and joins nothing."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0.1], [0.5, -1, 0.2], [0.5, 0.1, 1]], dtype=np.float32)
    return verts, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)


def cube2_duplicated():
    """cube(2) with face 5 once more at the end: every edge of the two copies has three owners."""
    verts, faces = moved(2, (0, 0, 0))
    return verts, np.concatenate([faces, faces[5:6]])


def welded(off):
    """Two unit cubes, the second shifted by off, with the vertices at one position made one."""
    verts, faces = joined([moved(1, (0, 0, 0)), moved(1, off)])
    uniq, inverse = np.unique(verts, axis=0, return_inverse=True)
    return uniq.astype(np.float32), inverse.reshape(-1)[faces].astype(np.int64)


def small(name):
    """(verts, faces, the face counts of the components in ascending leader) of a small topology."""
    if name == 'fins':
        return fins() + ([1, 1, 1],)
    if name == 'cube2 duplicated':
        return cube2_duplicated() + ([47, 1, 1],)
    if name == 'welded vertex':
        return welded((1, 1, 1)) + ([12, 12],)
    if name == 'welded edge':
        return welded((1, 1, 0)) + ([12, 12],)
    assert name == 'fan300'
    return smooth_spec.fan(300) + ([300],)


SMALL = ('fins', 'cube2 duplicated', 'welded vertex', 'welded edge', 'fan300')
