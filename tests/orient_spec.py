"""numpy restatement of the orientation stage (ppsurf_amd/csrc/pps_orient.hip, ppsurf_amd/orient.py): the specification
the GPU is held to, byte for byte, and the fixtures of its tests.  Nothing here comes from the device.

Rule: validity, adjacency, components and leaders are those of pieces_spec (a face is valid when its indices lie in [0, nv) and are pairwise
distinct; two valid faces are adjacent across an undirected edge that exactly two valid faces hold; the leader is the smallest face index).
Slot k of a face is the directed edge corner k -> corner k + 1 mod 3.  A pair (fa, fb) with its edge in the slots (ea, eb) -- the sort
positions % 3 -- has s = 1 when faces[fa][ea] == faces[fb][eb] (both run the edge the same way: one must turn), else 0.  In an orientable
component flip[f] is the XOR of s along any path from the leader; a component where some pair has flip[a] ^ flip[b] != s is not orientable and
comes back byte for byte.  Per orientable component, T = the faces with flip 1, U = those with flip 0: `majority` turns the smaller, T on a
tie; `outward` (`inward`) turns T when V > 0 (V < 0) and U when V < 0 (V > 0) for a closed component (2 pairs == 3 faces), and takes the
majority for V == 0 and for an open one.  V is six times the signed volume with the flips applied, fp64, in the order of `ordered_sum`.  A
turned face (a, b, c) becomes (a, c, b); every other row is kept.
"""
import numpy as np

import denoise_spec
import pieces_spec
import smooth_spec
from topology_spec import SENTINEL, valid_faces

D = np.float64
MODES = ('outward', 'inward', 'majority')
BLOCK = 256


def pair_list(faces, nv):
    """(fa, fb, ea, eb int64 [np], s uint8 [np]): the owners of every edge that exactly two valid faces hold, the slot of the edge in each
    (the position of its key % 3) and the sign of the pair.  The order of the pairs and which owner comes first mean nothing."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keys = pieces_spec.edge_keys(f, nv)
    order = np.argsort(keys, kind='stable')
    uniq, first, counts = np.unique(keys[order], return_index=True, return_counts=True)
    first = first[(counts == 2) & (uniq != SENTINEL)]
    one, two = order[first], order[first + 1]
    fa, fb, ea, eb = one // 3, two // 3, one % 3, two % 3
    s = (f[fa, ea] == f[fb, eb]).astype(np.uint8) if fa.shape[0] else np.zeros(0, dtype=np.uint8)
    return fa, fb, ea, eb, s


def flips_spec(faces, nv):
    """(label int32 [nf], flip uint8 [nf], bad uint8 [nf]): a breadth-first walk over the pair list from every unvisited valid face in
    ascending index, so the start is the leader; flip[n] = flip[f] ^ s along the tree; bad[leader] = 1 when a pair of the component
    contradicts the flips (they then depend on the tree and mean nothing).  label -1 and flip 0 for an invalid face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fa, fb, _, _, s = pair_list(f, nv)
    return flips_of_pairs(valid_faces(f, nv), fa, fb, s)


def flips_of_pairs(ok, fa, fb, s):
    """flips_spec on a given pair list (every entry a valid face) over the faces with `ok` set."""
    nf = ok.shape[0]
    around = [[] for _ in range(nf)]
    for a, b, sign in zip(fa.tolist(), fb.tolist(), s.tolist()):
        around[a].append((b, sign))
        around[b].append((a, sign))
    label, flip, bad = np.full(nf, -1, dtype=np.int32), np.zeros(nf, dtype=np.uint8), np.zeros(nf, dtype=np.uint8)
    for start in range(nf):
        if not ok[start] or label[start] >= 0:
            continue
        label[start] = start
        queue = [start]
        while queue:
            nxt = []
            for t in queue:
                for n, sign in around[t]:
                    if label[n] < 0:
                        label[n], flip[n] = start, flip[t] ^ sign
                        nxt.append(n)
            queue = nxt
    wrong = (flip[fa] ^ flip[fb]) != s
    bad[label[fa[wrong]]] = 1
    return label, flip, bad


def ordered_sum(t):
    """The sum of fp64 terms in the stated order: position j lies in block j // 256; lane (j % 256) // 4 adds its four terms in order from
    +0.0 (absent: +0.0); S[l] = S[l] + S[l + stride] for stride 1, 2, 4, 8, 16, 32 and l a multiple of 2 stride; the block sums are added
    in ascending order from +0.0.  Every operation is one rounded fp64 addition."""
    t = np.asarray(t, dtype=D).reshape(-1)
    blocks = (t.shape[0] + BLOCK - 1) // BLOCK
    padded = np.zeros(blocks * BLOCK, dtype=D)
    padded[:t.shape[0]] = t
    x = padded.reshape(blocks, 64, 4)
    S = np.zeros((blocks, 64), dtype=D)
    for j in range(4):
        S = S + x[:, :, j]
    for stride in (1, 2, 4, 8, 16, 32):
        at = np.arange(0, 64, 2 * stride)
        S[:, at] = S[:, at] + S[:, at + stride]
    total = D(0.0)
    for b in range(blocks):
        total = total + S[b, 0]
    return total


def block_sums(t):
    """f64 [blocks]: the block sums of `ordered_sum`."""
    t = np.asarray(t, dtype=D).reshape(-1)
    return np.array([ordered_sum(t[i:i + BLOCK]) for i in range(0, t.shape[0], BLOCK)], dtype=D)


def volume_terms(verts, faces, members, flip, leader):
    """f64 [len(members)]: the term of every listed face about R, the first corner of the leader as given, negated where flip is 1."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    R = v[f[leader, 0]].astype(D)
    q = v[f[members]].astype(D) - R[None, None]
    q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
    t = ((q0[:, 0] * (q1[:, 1] * q2[:, 2] - q1[:, 2] * q2[:, 1])) + (q0[:, 1] * (q1[:, 2] * q2[:, 0] - q1[:, 0] * q2[:, 2]))) \
        + (q0[:, 2] * (q1[:, 0] * q2[:, 1] - q1[:, 1] * q2[:, 0]))
    return np.where(np.asarray(flip)[members] == 1, -t, t)


def orient_spec(verts, faces, mode='outward'):
    """(verts f32, faces int64, info, table): orient.orient_mesh, and per component in ascending leader {leader, faces, pairs, ones,
    closed, bad, turn (0 nothing, 1 the faces with flip 1, 2 those with flip 0), vol (None where it is not computed)}."""
    assert mode in MODES
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    label, flip, bad = flips_spec(f, nv)
    fa = pair_list(f, nv)[0]
    out = f.copy()
    info = {'faces_in': int(nf), 'faces_valid': int((label >= 0).sum()), 'faces_flipped': 0, 'components': 0, 'components_closed': 0,
            'components_open': 0, 'components_non_orientable': 0, 'faces_non_orientable': 0, 'components_flipped': 0, 'zero_volume': 0,
            'mode': mode}
    table = []
    for leader in np.unique(label[label >= 0]).tolist():
        members = np.nonzero(label == leader)[0]                                    # ascending
        n, pairs, ones = int(members.shape[0]), int((label[fa] == leader).sum()), int(flip[members].sum())
        closed, broken = 2 * pairs == 3 * n, bool(bad[leader])
        row = {'leader': leader, 'faces': n, 'pairs': pairs, 'ones': ones, 'closed': closed, 'bad': broken, 'turn': 0, 'vol': None}
        table.append(row)
        info['components'] += 1
        info['components_closed' if closed else 'components_open'] += 1
        if broken:
            info['components_non_orientable'] += 1
            info['faces_non_orientable'] += n
            continue
        turn = 1 if 2 * ones <= n else 2
        if mode != 'majority' and closed:
            vol = ordered_sum(volume_terms(v, f, members, flip, leader))
            row['vol'] = float(vol)
            if vol > 0:
                turn = 1 if mode == 'outward' else 2
            elif vol < 0:
                turn = 2 if mode == 'outward' else 1
            else:
                info['zero_volume'] += 1
        row['turn'] = turn
        which = members[flip[members] == (1 if turn == 1 else 0)]
        out[which] = f[which][:, [0, 2, 1]]
        info['faces_flipped'] += int(which.shape[0])
        info['components_flipped'] += int(turn == 2)
    return v, out, info, table


def signed_volumes(verts, faces):
    """{leader: six times the signed volume of the component as wound, by ordered_sum}, for checks on oriented meshes."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = pieces_spec.labels_spec(f, v.shape[0])
    none = np.zeros(f.shape[0], dtype=np.uint8)
    return {l: float(ordered_sum(volume_terms(v, f, np.nonzero(label == l)[0], none, l))) for l in np.unique(label[label >= 0]).tolist()}


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------

INVALID = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 1 << 40]], dtype=np.int64)


def turned(faces, which=None):
    """The faces with the rows `which` (a mask or indices; all rows when None) as (a, c, b)."""
    out = np.array(faces, dtype=np.int64).reshape(-1, 3)
    rows = np.arange(out.shape[0]) if which is None else which
    out[rows] = out[rows][:, [0, 2, 1]]
    return out


def scramble(faces, seed, frac=0.5):
    """(faces with a seeded random subset turned, the mask of that subset)."""
    mask = np.random.default_rng(seed).random(np.asarray(faces).shape[0]) < frac
    return turned(faces, mask), mask


def tetra():
    """(verts f32 [4,3], faces [4,3]): a tetrahedron wound outward."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    return verts, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)


def lattice(nu, nw, wrap_u=None, wrap_w=False):
    """(faces int64 [2 nu nw,3], columns, rows): nu x nw quads over the vertices (u, w) -> u * rows + w, every quad (A, B, C, D) =
    ((u, w), (u + 1, w), (u + 1, w + 1), (u, w + 1)) split into (A, B, C), (A, C, D).  wrap_w: w is taken mod nw.  wrap_u 'plain': column
    nu is column 0; 'reversed': column nu is column 0 with w mirrored (-w mod nw with wrap_w, else nw - w), the seam of a Moebius strip or
    of a Klein bottle."""
    rows = nw if wrap_w else nw + 1
    cols = nu if wrap_u else nu + 1

    def at(u, w):
        if wrap_w:
            w %= nw
        if u == nu and wrap_u:
            u = 0
            if wrap_u == 'reversed':
                w = (-w) % nw if wrap_w else nw - w
        return u * rows + w

    faces = []
    for u in range(nu):
        for w in range(nw):
            A, B, C, Dq = at(u, w), at(u + 1, w), at(u + 1, w + 1), at(u, w + 1)
            faces += [[A, B, C], [A, C, Dq]]
    return np.array(faces, dtype=np.int64), cols, rows


def torus(nu=16, nw=8, seam='plain'):
    """(verts f32 [nu nw,3], faces [2 nu nw,3]): a torus lattice (radii 2 and 0.7) wound outward; seam 'reversed' joins the last column to
    the first mirrored: a Klein bottle on the same vertices (its surface crosses itself, which no rule here looks at)."""
    faces, cols, rows = lattice(nu, nw, seam, True)
    u, w = np.meshgrid(np.arange(cols), np.arange(rows), indexing='ij')
    a, b = 2.0 * np.pi * u.reshape(-1) / nu, 2.0 * np.pi * w.reshape(-1) / nw
    verts = np.stack([(2.0 + 0.7 * np.cos(b)) * np.cos(a), (2.0 + 0.7 * np.cos(b)) * np.sin(a), 0.7 * np.sin(b)], axis=1).astype(np.float32)
    return verts, faces


def moebius(nu=16, nw=3):
    """(verts f32, faces): a Moebius strip lattice of nu x nw quads (open, not orientable)."""
    faces, cols, rows = lattice(nu, nw, 'reversed', False)
    u, w = np.meshgrid(np.arange(cols), np.arange(rows), indexing='ij')
    a, t = 2.0 * np.pi * u.reshape(-1) / nu, (w.reshape(-1) / nw - 0.5)
    verts = np.stack([(2.0 + t * np.cos(a / 2)) * np.cos(a), (2.0 + t * np.cos(a / 2)) * np.sin(a), t * np.sin(a / 2)], axis=1).astype(np.float32)
    return verts, faces


def flat(n=12):
    """(verts f32, faces): a flat n x n lattice in the plane z = 0 (open, wound towards +z)."""
    faces, cols, rows = lattice(n, n)
    u, w = np.meshgrid(np.arange(cols), np.arange(rows), indexing='ij')
    return np.stack([u.reshape(-1), w.reshape(-1), 0 * u.reshape(-1)], axis=1).astype(np.float32), faces


def sphere():
    return smooth_spec.noisy_sphere(3)


def cube():
    verts, faces, _ = denoise_spec.cube(8)
    return verts.astype(np.float32), faces


def closed_mesh(name):
    """(verts, faces) of a closed mesh wound outward: 'sphere', 'cube', 'torus' or 'scene'."""
    return {'sphere': sphere, 'cube': cube, 'torus': torus, 'scene': pieces_spec.scene}[name]()


CLOSED = ('sphere', 'cube', 'torus', 'scene')
SEEDS = {'sphere': 21, 'cube': 22, 'torus': 23, 'scene': 24}


def with_invalid(faces, at=(3, 300, 301)):
    """The faces with the rows of INVALID put in before the given positions (of the growing array)."""
    out = np.asarray(faces, dtype=np.int64)
    for row, k in zip(INVALID, at):
        out = np.concatenate([out[:k], row[None], out[k:]])
    return out


def flat_tie(leader_turned):
    """The flat lattice with exactly half of its 288 faces turned (default_rng(31)), face 0 among them or not."""
    verts, faces = flat()
    rows = np.random.default_rng(31).permutation(faces.shape[0])[:faces.shape[0] // 2]
    if (0 in rows.tolist()) != leader_turned:
        mask = np.ones(faces.shape[0], dtype=bool)
        mask[rows] = False
        rows = np.nonzero(mask)[0]
    return verts, turned(faces, rows)


def case(name):
    """(verts f32, faces int64) of a named test mesh."""
    if name in CLOSED:                                                 # scrambled: half of the faces turned
        verts, faces = closed_mesh(name)
        return verts, scramble(faces, SEEDS[name])[0]
    if name == 'tetra':
        return tetra()
    if name == 'tetra one turned':
        return tetra()[0], turned(tetra()[1], [2])
    if name == 'twins same':
        return tetra()[0], np.array([[0, 1, 2], [0, 1, 2]], dtype=np.int64)
    if name == 'twins opposite':
        return tetra()[0], np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64)
    if name == 'moebius':
        return moebius()
    if name == 'klein':
        return torus(seam='reversed')
    if name in ('klein and sphere', 'moebius and sphere'):
        sv, sf = case('sphere')
        return pieces_spec.joined([torus(seam='reversed') if name.startswith('klein') else moebius(), (sv, sf)])
    if name == 'flat 30':
        return flat()[0], scramble(flat()[1], 25, 0.3)[0]
    if name == 'flat tie':
        return flat_tie(False)
    if name == 'flat tie leader':
        return flat_tie(True)
    if name == 'sphere invalid':
        verts, faces = case('sphere')
        return verts, with_invalid(faces)
    if name == 'sphere coherent':
        return sphere()
    if name == 'sphere inside out':
        return sphere()[0], turned(sphere()[1])
    if name == 'strip reversed':
        return pieces_spec.strip(1025, 'reversed')
    if name == 'strip permuted':
        return pieces_spec.strip(1025, 'permuted')
    if name == 'fins':
        return pieces_spec.fins()
    if name == 'empty':
        return tetra()[0], np.zeros((0, 3), dtype=np.int64)
    assert name == 'all invalid'
    return tetra()[0], INVALID.copy()


CASES = CLOSED + ('tetra', 'tetra one turned', 'twins same', 'twins opposite', 'moebius', 'klein', 'klein and sphere', 'moebius and sphere', 'flat 30',
                  'flat tie', 'flat tie leader', 'sphere invalid', 'sphere coherent', 'sphere inside out', 'strip reversed', 'strip permuted', 'fins',
                  'empty', 'all invalid')
