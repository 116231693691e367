"""numpy restatement of the longest-edge bisection (ppsurf_amd/csrc/pps_subdivide.hip, ppsurf_amd/subdivide.py): the
specification the GPU is held to, byte for byte, and the fixtures and measures of its tests.  Every fp64 step is one numpy float64 operation
in the order the kernel uses; nothing here comes from the device.

Rule, per round, on the vertices V (f32; P is V widened to fp64) and the working faces F; a face that is invalid for the INPUT vertex count
holds (-1, -1, -1) in F, takes no part in any round and comes back as given:
  edges      the distinct undirected edges of the valid faces in ascending key (min << 32) | max with their owners; the ends a < b of run e
             are the halves of its key and its rank is e.
  candidate  len2 = (dx dx + dy dy) + dz dz of d = P_b - P_a exceeds max2, and M = f32((P_a + P_b) 0.5) differs from V[a] and from V[b].
  priority   ((0x7FF00000 - (bits(f64 len2) >> 32)) << 32) | fmix32(e), a u64, the smallest first; NONE = 2^64 - 1 for every other run.
  choice     every valid face takes the slot k of the smallest priority among its three edges (none when all are NONE) and votes for it.
  winners    a candidate whose votes equal its owners.
  apply      the winners in ascending key get the rows nv + i at M; a face whose chosen edge won keeps its row with entry k + 1 replaced by
             the new row m, and the old row with entry k replaced by m is appended at nf + (its rank among such faces in ascending f).
The rounds stop when an evaluation has no candidate (converged), after max_rounds rounds, or before a round that would take the faces above
max_faces or the vertices above 2^31 - 1 (limited; nothing of that round is applied).
"""
import math

import numpy as np

import pieces_spec
from topology_spec import SENTINEL, valid_faces

D = np.float64
U = np.uint64
NONE = U(0xFFFFFFFFFFFFFFFF)
INF_HIGH = 0x7FF00000
MAX_FACES = (2 ** 32 - 1) // 3
MAX_VERTS = 2 ** 31 - 1


def fmix32(h):
    """uint32: murmur3's 32-bit finaliser, a bijection of the 32-bit words."""
    h = np.asarray(h, dtype=np.uint64) & U(0xFFFFFFFF)
    h = h ^ (h >> U(16))
    h = (h * U(0x85EBCA6B)) & U(0xFFFFFFFF)
    h = h ^ (h >> U(13))
    h = (h * U(0xC2B2AE35)) & U(0xFFFFFFFF)
    h = h ^ (h >> U(16))
    return h.astype(np.uint32)


def edge_table(F, nv):
    """(keys int64 [ne] ascending and distinct, owners int64 [ne], run_of int64 [nf,3]): the edges of the valid faces and the run of every
    slot, -1 in the rows of an invalid face."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    all_keys = pieces_spec.edge_keys(F, nv)
    keys, inverse, owners = np.unique(all_keys, return_inverse=True, return_counts=True)
    run_of = inverse.reshape(-1).astype(np.int64)
    run_of[all_keys == SENTINEL] = -1
    live = keys != SENTINEL
    return keys[live], owners[live].astype(np.int64), run_of.reshape(-1, 3)


def midpoints(V, a, b):
    """f32 [n,3]: f32((P_a + P_b) 0.5), the one fp64 sum and product per component rounded to nearest."""
    P = np.asarray(V, dtype=np.float32).astype(D)
    return ((P[a] + P[b]) * D(0.5)).astype(np.float32)


def edge_priorities(keys, V, max2):
    """(len2 f64 [ne], prio uint64 [ne]) of any key list: a key that is negative or whose halves are no a < b < nv (the sentinel is one) has
    len2 0 and NONE; the rank is the position in the list."""
    keys = np.asarray(keys, dtype=np.int64)
    V = np.asarray(V, dtype=np.float32).reshape(-1, 3)
    nv = V.shape[0]
    a, b = keys >> 32, keys & 0xFFFFFFFF
    ok = (keys >= 0) & (a < b) & (b < nv)
    a, b = np.where(ok, a, 0), np.where(ok, b, 0)
    P = V.astype(D)
    with np.errstate(all='ignore'):
        d = P[b] - P[a] if nv else np.zeros((keys.shape[0], 3))
        len2 = np.where(ok, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], D(0.0))
        M = midpoints(V, a, b) if nv else np.zeros((keys.shape[0], 3), dtype=np.float32)
        cand = ok & (len2 > D(max2)) & (M != V[a]).any(axis=1) & (M != V[b]).any(axis=1) if nv else np.zeros(keys.shape[0], dtype=bool)
    high = U(INF_HIGH) - (np.where(cand, len2, D(1.0)).view(U) >> U(32))
    prio = np.where(cand, (high << U(32)) | fmix32(np.arange(keys.shape[0])).astype(U), NONE)
    return len2, prio


def choices(run_of, prio):
    """(choice int64 [nf] in -1..2, votes int64 [ne]): the first slot of the smallest priority per face; a run outside [0, ne) counts as NONE."""
    run_of = np.asarray(run_of, dtype=np.int64).reshape(-1, 3)
    ne = prio.shape[0]
    inside = (run_of >= 0) & (run_of < ne)
    p = np.where(inside, prio[np.where(inside, run_of, 0)] if ne else NONE, NONE)
    k = np.argmin(p, axis=1) if p.shape[0] else np.zeros(0, dtype=np.int64)
    choice = np.where(p[np.arange(p.shape[0]), k] != NONE, k, -1).astype(np.int64)
    votes = np.zeros(ne, dtype=np.int64)
    has = choice >= 0
    np.add.at(votes, run_of[has, choice[has]], 1)
    return choice, votes


def hits_of(run_of, choice, win):
    """bool [nf]: the face chose a slot in 0..2 whose run lies in range and won."""
    run_of = np.asarray(run_of, dtype=np.int64).reshape(-1, 3)
    ok = (choice >= 0) & (choice <= 2)
    r = np.where(ok, run_of[np.arange(run_of.shape[0]), np.where(ok, choice, 0)], -1)
    ok &= (r >= 0) & (r < win.shape[0])
    return ok & (win[np.where(ok, r, 0)] != 0 if win.shape[0] else False)


def evaluate(V, F, max2):
    """Everything an evaluation computes, by name: keys, owners, run_of, len2, prio, cand, choice, votes, win (bool [ne]), hit (bool [nf])."""
    keys, owners, run_of = edge_table(F, V.shape[0])
    len2, prio = edge_priorities(keys, V, max2)
    choice, votes = choices(run_of, prio)
    win = (prio != NONE) & (votes == owners)
    return {'keys': keys, 'owners': owners, 'run_of': run_of, 'len2': len2, 'prio': prio, 'cand': prio != NONE, 'choice': choice, 'votes': votes,
            'win': win, 'hit': hits_of(run_of, choice, win)}


def emit(V, F, ev):
    """(verts f32, faces int64, ends int64 [winners,2]) after the winners of an evaluation split."""
    nv, nf = V.shape[0], F.shape[0]
    w = np.nonzero(ev['win'])[0]
    a, b = ev['keys'][w] >> 32, ev['keys'][w] & 0xFFFFFFFF
    new_row = np.full(ev['keys'].shape[0], -1, dtype=np.int64)
    new_row[w] = nv + np.arange(w.shape[0])
    h = np.nonzero(ev['hit'])[0]
    k = ev['choice'][h]
    m = new_row[ev['run_of'][h, k]]
    out = np.concatenate([F, F[h]])
    out[h, (k + 1) % 3] = m
    out[nf + np.arange(h.shape[0]), k] = m
    return np.concatenate([V, midpoints(V, a, b)]), out, np.stack([a, b], axis=1).astype(np.int64).reshape(-1, 2)


def median_edge(V, F):
    """The max_edge of factor 1: the square root of the lower median of the squared lengths of the distinct edges, 0.0 without an edge."""
    len2 = edge_priorities(edge_table(F, V.shape[0])[0], V, np.inf)[0]
    return math.sqrt(float(np.sort(len2)[(len2.shape[0] - 1) // 2])) if len2.shape[0] else 0.0


def subdivide_spec(verts, faces, max_edge=None, factor=None, max_rounds=100, max_faces=None, trace=None):
    """(verts f32, faces int64, ends int64, info) of subdivide.split_long_edges(..., return_ends=True).  trace, a list, receives
    (V, F, evaluation) of every round that split."""
    assert (max_edge is None) != (factor is None)
    V = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    given = np.array(faces, dtype=np.int64).reshape(-1, 3)
    nv0, nf0 = V.shape[0], given.shape[0]
    ok = valid_faces(given, nv0)
    F = np.where(ok[:, None], given, -1)
    max_faces = MAX_FACES if max_faces is None else int(max_faces)
    info = {'vertices_in': nv0, 'vertices_out': nv0, 'faces_in': nf0, 'faces_valid': int(ok.sum()), 'faces_out': nf0, 'edges_in': 0,
            'max_edge': 0.0 if max_edge is None else float(max_edge), 'candidates_in': 0, 'candidates_out': 0, 'splits': 0, 'rounds': 0,
            'converged': True, 'limited': False, 'max_rounds': int(max_rounds), 'max_faces': max_faces, 'added': []}
    ends = [np.zeros((0, 2), dtype=np.int64)]
    if not ok.any():
        return V, given, ends[0], info
    if max_edge is None:
        info['max_edge'] = float(factor) * median_edge(V, F)
    max2 = info['max_edge'] * info['max_edge']
    first = True
    while True:
        ev = evaluate(V, F, max2)
        count = int(ev['cand'].sum())
        if first:
            info['edges_in'], info['candidates_in'], first = int(ev['keys'].shape[0]), count, False
        winners, hits = int(ev['win'].sum()), int(ev['hit'].sum())
        limited = count > 0 and info['rounds'] < max_rounds and (F.shape[0] + hits > max_faces or V.shape[0] + winners > MAX_VERTS)
        if count == 0 or info['rounds'] == max_rounds or limited:
            info.update(candidates_out=count, converged=count == 0, limited=limited)
            break
        assert winners > 0
        if trace is not None:
            trace.append((V, F, ev))
        V, F, e = emit(V, F, ev)
        ends.append(e)
        info['rounds'] += 1
        info['splits'] += winners
        info['added'].append(winners)
    info.update(vertices_out=int(V.shape[0]), faces_out=int(F.shape[0]))
    if info['splits'] == 0:
        return V, given, ends[0], info
    F[:nf0][~ok] = given[~ok]
    return V, F, np.concatenate(ends), info


# ---- measures ------------------------------------------------------------------------------------------------------------------------------------
def live(faces, nv):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return f[valid_faces(f, nv)]


def edge_lengths2(verts, faces):
    """(keys, owners, squared length f64) of the distinct edges of valid faces, computed on its own: np.unique over sorted pairs."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(e, axis=0, return_counts=True)
    P = np.asarray(verts, dtype=D)
    d = P[uniq[:, 1]] - P[uniq[:, 0]]
    return (uniq[:, 0] << 32) | uniq[:, 1], counts, (d * d).sum(axis=1)


def min_angle(verts, faces):
    """The smallest corner angle in degrees of the faces given."""
    p = np.asarray(verts, dtype=D)[np.asarray(faces, dtype=np.int64)]
    best = np.inf
    for i in range(3):
        u, w = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        best = min(best, float(np.degrees(np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(axis=1))).min()))
    return best


def incoherent_pairs(faces):
    """How many two-owner edges both owners run the same way (valid faces given)."""
    f = np.asarray(faces, dtype=np.int64)
    src = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    dst = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    key = (np.minimum(src, dst) << 32) | np.maximum(src, dst)
    order = np.argsort(key, kind='stable')
    uniq, first, counts = np.unique(key[order], return_index=True, return_counts=True)
    first = first[counts == 2]
    return int((src[order[first]] == src[order[first + 1]]).sum())


def interpolate_colors(colors, ends, added):
    """uint8 [nv + new, c]: the specification of subdivide.midpoint_colors, one new vertex at a time."""
    out = [np.asarray(row, dtype=np.int64) for row in np.asarray(colors)]
    assert sum(added) == len(ends)
    for a, b in np.asarray(ends).tolist():
        out.append((out[a] + out[b] + 1) >> 1)
    return np.array(out, dtype=np.uint8).reshape(len(out), -1)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
INVALID = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 1 << 40]], dtype=np.int64)
FACTORS = (1.0, 0.5, 0.26)
BASES = ('cube', 'torus', 'sphere', 'patch', 'lattice', 'tetrahedron', 'torus scrambled', 'sphere scrambled', 'cube decimated', 'sphere decimated',
         'cubes welded')
VARIANTS = ('', ' invalid', ' shuffled')
CASES = tuple(b + v for b in BASES for v in VARIANTS) + ('empty', 'all invalid')
_base = {}


def base(name):
    """(verts f32, faces int64) of the named meshes, computed once."""
    if name not in _base:
        import decimate_spec
        import denoise_spec
        import flip_spec
        import smooth_spec
        if name == 'cube':
            mesh = denoise_spec.cube(8)[:2]
        elif name == 'torus':
            mesh = decimate_spec.torus(32, 16)
        elif name == 'sphere':
            mesh = smooth_spec.noisy_sphere(3)
        elif name == 'patch':
            mesh = decimate_spec.patch(12)
        elif name == 'lattice':
            mesh = flip_spec.jittered_lattice(12)
        elif name == 'tetrahedron':
            mesh = decimate_spec.tetrahedron()
        else:
            mesh = flip_spec.base(name)
        _base[name] = (np.ascontiguousarray(mesh[0], dtype=np.float32), np.ascontiguousarray(mesh[1], dtype=np.int64))
    return _base[name]


def with_invalid(faces):
    """The faces with the rows of INVALID put in before rows 3, 10 and 11 (of the growing array), as far as there are rows."""
    out = np.asarray(faces, dtype=np.int64)
    for row, k in zip(INVALID, (3, 10, 11)):
        k = min(k, out.shape[0])
        out = np.concatenate([out[:k], row[None], out[k:]])
    return out


def shuffled(faces, seed):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int64)[np.random.default_rng(seed).permutation(np.asarray(faces).shape[0])])


def case(name):
    """(verts f32, faces int64) of a named test mesh."""
    if name == 'empty':
        return base('patch')[0], np.zeros((0, 3), dtype=np.int64)
    if name == 'all invalid':
        return base('patch')[0], INVALID.copy()
    for k, variant in enumerate(VARIANTS[1:]):
        if name.endswith(variant):
            verts, faces = base(name[:-len(variant)])
            return verts, with_invalid(faces) if k == 0 else shuffled(faces, 80 + BASES.index(name[:-len(variant)]))
    return base(name)


def hostile(scale=1.0):
    """(verts f32, faces int64): the 12 x 12 jittered lattice stretched, bent and shifted so that no coordinate is a short binary fraction,
    built here from the generator alone; `scale` multiplies the f32 coordinates in fp64 (1e38 keeps them finite)."""
    import flip_spec
    verts, faces = flip_spec.jittered_lattice(12)
    rng = np.random.default_rng(12)
    verts = (verts.astype(D) * [1.37, 0.73, 1.0] + [0.1, -0.3, 0.0]
             + np.stack([0 * verts[:, 0], 0 * verts[:, 0], 0.15 * rng.standard_normal(verts.shape[0])], axis=1)).astype(np.float32)
    if scale != 1.0:
        verts = (verts.astype(D) * (scale / float(np.abs(verts).max()))).astype(np.float32)
    return verts, faces


def hand_cases():
    """[(name, verts f32, faces int64, max_edge, max_rounds)]: the meshes written out by hand that both tiers run."""
    tri = np.array([[0, 0, 0], [4, 0, 0], [1, 1, 0]], dtype=np.float32)
    quad = np.array([[0, 0, 0], [4, 0, 0], [2, 1, 0], [2, -1, 0]], dtype=np.float32)
    book = np.array([[0, 0, 0], [4, 0, 0], [2, 1, 0], [2, -1, 0], [2, 0, 1]], dtype=np.float32)
    wait = np.array([[0, 0, 0], [4, 0, 0], [1, 3, 0], [2, -0.5, 0]], dtype=np.float32)
    eq = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]], dtype=np.float32)[[1, 2, 3]]
    one = np.float32(1.0)
    near = np.array([[1, 0, 0], [np.nextafter(one, np.float32(2)), 0, 0], [1, 3, 0]], dtype=np.float32)
    late = np.array([[0, 0, 0], [4, 0, 0], [1, 1, 0], [9, 9, 9], [8, 8, 8], [7, 7, 7], [6, 6, 6]], dtype=np.float32)
    I = lambda rows: np.array(rows, dtype=np.int64)
    return [('slot 0', tri, I([[0, 1, 2]]), 3.5, 100), ('slot 1', tri, I([[2, 0, 1]]), 3.5, 100), ('slot 2', tri, I([[1, 2, 0]]), 3.5, 100),
            ('two faces', quad, I([[0, 1, 2], [1, 0, 3]]), 3.0, 100), ('waits', wait, I([[0, 1, 2], [1, 0, 3]]), 3.1, 100),
            ('equilateral', eq, I([[0, 1, 2]]), 2.0, 100), ('three on an edge', book, I([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), 3.0, 100),
            ('two copies', tri, I([[0, 1, 2], [0, 1, 2]]), 3.5, 100), ('neighbouring floats', near, I([[0, 1, 2]]), 1e-30, 4),
            ('rows out of play', late, I([[7, 1, 2], [0, 1, 2], [5, 6, 5]]), 1.5, 100)]
