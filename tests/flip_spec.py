"""numpy restatement of the Delaunay edge flips (ppsurf_amd/csrc/pps_flip.hip, ppsurf_amd/flip.py): the specification the
GPU is held to, byte for byte, and the fixtures and measures of its tests.  Every fp64 step is one numpy float64 operation in the order the
kernel uses; nothing here comes from the device.

Rule, per round, on the vertices P (the f32 vertices widened to fp64) and the current faces F, a working copy; invalid faces take no part:
  edges      the distinct undirected edges of the valid faces in ascending key (min << 32) | max with their owners; only an edge with exactly
             two owners can be a candidate, and its rank r is its position among the two-owner edges in ascending key.
  quad       f < g the two owners, k and l the slot of the edge in each: a = F[f][k], b = F[f][k + 1], c = F[f][k + 2]; the pair takes part
             only when F[g][l] == b and F[g][l + 1] == a (the faces run the edge in opposite ways); d = F[g][l + 2].
  topology   c != d and the edge {c, d} is no edge of F (a binary search in the ascending distinct keys).
  geometry   n1 = (P_b - P_a) x (P_c - P_a), n2 = (P_a - P_b) x (P_d - P_b), m1 = (P_d - P_a) x (P_c - P_a), m2 = (P_c - P_b) x (P_d - P_b),
             N = n1 + n2; fold guard m1.N > 0 and m2.N > 0; crease guard t = n1.n2, A = n1.n1, B = n2.n2: t >= 0 and t t >= cos2 (A B).
  criterion  p = (P_a - P_c).(P_b - P_c), q = (P_a - P_d).(P_b - P_d), s = p / sqrt(A) + q / sqrt(B); a candidate iff s < -min_gain.
  priority   ((0x7F800000 - bits(f32(-s))) << 32) | fmix32(r), a u64, the smallest first; NONE = 2^64 - 1 for every other pair.
  winners    vmin[v] = the minimum priority over the candidates whose quad holds v; an edge wins iff vmin equals its priority at a, b, c, d.
  apply      F[f] = (a, d, c), F[g] = (b, c, d).
The rounds stop when an evaluation has no candidate, or after max_rounds rounds.  A cross is written out component by component, every
component p*q - r*s; a dot is (x x' + y y') + z z'; a comparison with a NaN is false.
"""
import math

import numpy as np

import pieces_spec
from topology_spec import SENTINEL, valid_faces

D = np.float64
U = np.uint64
NONE = U(0xFFFFFFFFFFFFFFFF)
INF_BITS = 0x7F800000


def fmix32(h):
    """uint32: murmur3's 32-bit finaliser, a bijection of the 32-bit words."""
    h = np.asarray(h, dtype=np.uint64) & U(0xFFFFFFFF)
    h = h ^ (h >> U(16))
    h = (h * U(0x85EBCA6B)) & U(0xFFFFFFFF)
    h = h ^ (h >> U(13))
    h = (h * U(0xC2B2AE35)) & U(0xFFFFFFFF)
    h = h ^ (h >> U(16))
    return h.astype(np.uint32)


def cos2_of(max_angle):
    """The one host computation both sides take their threshold from."""
    return math.cos(math.radians(max_angle)) ** 2


def edge_table(F, nv):
    """(keys int64 [ne] ascending and distinct, owners int64 [ne], f, g, k, l int64 [np]): the edges of the valid faces, and for those with
    two owners in ascending key the owners f < g and the slot of the edge in each."""
    all_keys = pieces_spec.edge_keys(F, nv)
    order = np.argsort(all_keys, kind='stable')
    uniq, first, counts = np.unique(all_keys[order], return_index=True, return_counts=True)
    live = uniq != SENTINEL
    uniq, first, counts = uniq[live], first[live], counts[live]
    first = first[counts == 2]
    one, two = order[first], order[first + 1]
    swap = one // 3 > two // 3
    one, two = np.where(swap, two, one), np.where(swap, one, two)
    return uniq, counts, one // 3, two // 3, one % 3, two % 3


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def _dot(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]


def evaluate(P, F, nv, cos2, min_gain):
    """Everything an evaluation computes, by name: keys, owners, f, g (the pairs), quad int64 [np,4] (zeros for a non-candidate), s f64 [np]
    (NaN where the pair never reached the criterion), prio uint64 [np], cand bool [np], vmin uint64 [nv], win bool [np]."""
    keys, owners, f, g, k, l = edge_table(F, nv)
    n = f.shape[0]
    a, b, c = F[f, k], F[f, (k + 1) % 3], F[f, (k + 2) % 3]
    coherent = (F[g, l] == b) & (F[g, (l + 1) % 3] == a)
    d = F[g, (l + 2) % 3]
    new_key = (np.minimum(c, d) << 32) | np.maximum(c, d)
    at = np.searchsorted(keys, new_key)
    exists = keys[np.minimum(at, max(keys.shape[0] - 1, 0))] == new_key if keys.shape[0] else np.zeros(n, dtype=bool)
    ok = coherent & (c != d) & ~exists
    d = np.where(coherent, d, 0)                                     # (never read through where the pair is incoherent)
    Pa, Pb, Pc, Pd = P[a], P[b], P[c], P[d]
    with np.errstate(all='ignore'):
        n1, n2 = _cross(Pb - Pa, Pc - Pa), _cross(Pa - Pb, Pd - Pb)
        m1, m2 = _cross(Pd - Pa, Pc - Pa), _cross(Pc - Pb, Pd - Pb)
        N = n1 + n2
        fold = (_dot(m1, N) > 0) & (_dot(m2, N) > 0)
        t, A, B = _dot(n1, n2), _dot(n1, n1), _dot(n2, n2)
        crease = (t >= 0) & (t * t >= D(cos2) * (A * B))
        p, q = _dot(Pa - Pc, Pb - Pc), _dot(Pa - Pd, Pb - Pd)
        s = p / np.sqrt(A) + q / np.sqrt(B)
        cand = ok & fold & crease & (s < -D(min_gain))
        high = U(INF_BITS) - np.where(cand, -s, D(1.0)).astype(np.float32).view(np.uint32).astype(U)
    prio = np.where(cand, (high << U(32)) | fmix32(np.arange(n)).astype(U), NONE)
    quad = np.where(cand[:, None], np.stack([a, b, c, d], axis=1), 0).astype(np.int64).reshape(-1, 4)
    vmin = np.full(nv, NONE, dtype=U)
    for j in range(4):
        np.minimum.at(vmin, quad[cand, j], prio[cand])
    win = cand & (vmin[quad] == prio[:, None]).all(axis=1)
    return {'keys': keys, 'owners': owners, 'f': f, 'g': g, 'quad': quad, 's': np.where(ok, s, np.nan), 'prio': prio, 'cand': cand, 'vmin': vmin,
            'win': win}


def apply_spec(F, ev):
    """The faces after the winners of an evaluation flipped."""
    out = F.copy()
    w = np.nonzero(ev['win'])[0]
    a, b, c, d = (ev['quad'][w, j] for j in range(4))
    out[ev['f'][w]] = np.stack([a, d, c], axis=1)
    out[ev['g'][w]] = np.stack([b, c, d], axis=1)
    return out


def flip_spec(verts, faces, max_angle=10.0, min_gain=1e-6, max_rounds=100, trace=None):
    """(verts f32, faces int64, info) of flip.flip_edges.  trace, a list, receives the evaluation of every round that flipped."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    F = np.array(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    P, cos2 = v.astype(D), cos2_of(max_angle)
    info = {'faces_in': int(F.shape[0]), 'faces_valid': int(valid_faces(F, nv).sum()), 'edges_manifold': 0, 'candidates_in': 0, 'candidates_out': 0,
            'flips': 0, 'rounds': 0, 'converged': True, 'max_angle': float(max_angle), 'min_gain': float(min_gain), 'max_rounds': int(max_rounds)}
    first = True
    while True:
        ev = evaluate(P, F, nv, cos2, min_gain)
        count = int(ev['cand'].sum())
        if first:
            info['edges_manifold'], info['candidates_in'], first = int(ev['f'].shape[0]), count, False
        if count == 0 or info['rounds'] == max_rounds:
            info['candidates_out'], info['converged'] = count, count == 0
            break
        assert ev['win'].any()
        if trace is not None:
            trace.append(ev)
        F = apply_spec(F, ev)
        info['rounds'] += 1
        info['flips'] += int(ev['win'].sum())
    return v, F, info


# ---- measures ------------------------------------------------------------------------------------------------------------------------------------
def edge_sets(faces, nv):
    """(border keys, many-owner keys, all keys with their owners): sorted int64 arrays of the valid faces' edges."""
    keys = pieces_spec.edge_keys(faces, nv)
    uniq, counts = np.unique(keys[keys != SENTINEL], return_counts=True)
    return uniq[counts == 1], uniq[counts > 2], uniq, counts


def incoherent_pairs(faces, nv):
    """How many two-owner edges both owners run the same way."""
    F = np.asarray(faces, dtype=np.int64)
    _, _, f, g, k, l = edge_table(F, nv)
    return int((F[f, k] == F[g, l]).sum())


def angles(verts, faces):
    """f64 [nf,3]: the corner angles in degrees of the valid faces given (0 at the ends and 180 at the middle of a face without area)."""
    p = np.asarray(verts, dtype=D)[np.asarray(faces, dtype=np.int64)]
    out = np.zeros(p.shape[:2], dtype=D)
    for i in range(3):
        u, w = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        out[:, i] = np.degrees(np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), (u * w).sum(axis=1)))
    return out


def min_angle(verts, faces):
    f = np.asarray(faces, dtype=np.int64)
    return float(angles(verts, f[valid_faces(f, np.asarray(verts).shape[0])]).min())


def delaunay_violations(verts, faces, slack=1e-6):
    """How many (face, vertex) pairs of a flat mesh in the plane z = 0 have the vertex strictly inside the face's circumcircle: brute force,
    with the relative slack on the squared radius, and independent of the rule above."""
    p = np.asarray(verts, dtype=D)[:, :2]
    t = p[np.asarray(faces, dtype=np.int64)]
    ax, ay, bx, by, cx, cy = t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1], t[:, 2, 0], t[:, 2, 1]
    det = 2.0 * (ax * (by - cy) + bx * (cy - ay) + cx * (ay - by))
    a2, b2, c2 = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
    ux = (a2 * (by - cy) + b2 * (cy - ay) + c2 * (ay - by)) / det
    uy = (a2 * (cx - bx) + b2 * (ax - cx) + c2 * (bx - ax)) / det
    r2 = (ax - ux) ** 2 + (ay - uy) ** 2
    d2 = (p[None, :, 0] - ux[:, None]) ** 2 + (p[None, :, 1] - uy[:, None]) ** 2
    return int((d2 < r2[:, None] * (1.0 - slack)).sum())


def areas2(verts, faces):
    """f64 [nf]: twice the signed area of every face of a flat mesh in the plane z = 0."""
    t = np.asarray(verts, dtype=D)[np.asarray(faces, dtype=np.int64)][:, :, :2]
    u, w = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
INVALID = np.array([[0, 0, 1], [-1, 2, 3], [5, 6, 1 << 40]], dtype=np.int64)
ANGLES = (10.0, 30.0, 90.0)
LATTICES = (4, 12, 24)


def jittered_lattice(n, seed=None):
    """(verts f32 [(n + 1)^2,3], faces int64 [2 n^2,3]): a flat lattice of n x n unit quads in z = 0, every quad split alike and wound towards
    +z.  Interior vertices are moved by up to 0.2 of a cell in x and y, border vertices only along their side and corners not at all
    (default_rng(seed), seed = n when None): the domain stays the convex square and every triangle keeps its orientation."""
    rng = np.random.default_rng(n if seed is None else seed)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    jit = rng.uniform(-0.2, 0.2, size=(i.shape[0], 2))
    jit[(i == 0) | (i == n), 0] = 0.0
    jit[(j == 0) | (j == n), 1] = 0.0
    verts = np.stack([i + jit[:, 0], j + jit[:, 1], 0.0 * i], axis=1).astype(np.float32)
    qi, qj = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    qi, qj = qi.reshape(-1), qj.reshape(-1)
    at = lambda p, r: p * (n + 1) + r
    quad = np.stack([at(qi, qj), at(qi + 1, qj), at(qi + 1, qj + 1), at(qi, qj + 1)], axis=1)
    return verts, np.ascontiguousarray(np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]), dtype=np.int64)


def scrambled(verts, faces, seed, steps=None):
    """The faces after a seeded sequence of legal flips (steps of them tried, one per face by default): a random two-owner edge whose owners
    run it in opposite ways, with c != d and no edge {c, d} yet, is flipped as the rule's apply does, whatever the geometry."""
    F = np.array(faces, dtype=np.int64)
    nv = np.asarray(verts).shape[0]
    rng = np.random.default_rng(seed)
    for _ in range(F.shape[0] if steps is None else steps):
        keys, _, f, g, k, l = edge_table(F, nv)
        e = int(rng.integers(f.shape[0]))
        fe, ge, ke, le = int(f[e]), int(g[e]), int(k[e]), int(l[e])
        a, b, c = (int(F[fe, (ke + j) % 3]) for j in range(3))
        d = int(F[ge, (le + 2) % 3])
        if F[ge, le] != b or F[ge, (le + 1) % 3] != a or c == d or ((min(c, d) << 32) | max(c, d)) in set(keys.tolist()):
            continue
        F[fe], F[ge] = (a, d, c), (b, c, d)
    return F


def with_invalid(faces):
    """The faces with the rows of INVALID put in before rows 3, 10 and 11 (of the growing array)."""
    out = np.asarray(faces, dtype=np.int64)
    for row, k in zip(INVALID, (3, 10, 11)):
        out = np.concatenate([out[:k], row[None], out[k:]])
    return out


def shuffled(faces, seed):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int64)[np.random.default_rng(seed).permutation(np.asarray(faces).shape[0])])


_base = {}


def base(name):
    """(verts f32, faces int64) of the curved and repaired meshes, computed once."""
    if name not in _base:
        import decimate_spec
        import denoise_spec
        import smooth_spec
        if name == 'torus scrambled':
            verts, faces = decimate_spec.torus(32, 16)
            mesh = verts, scrambled(verts, faces, 61, 300)
        elif name == 'sphere scrambled':
            verts, faces = smooth_spec.noisy_sphere(3)
            mesh = verts, scrambled(verts, faces, 62, 300)
        elif name == 'cube decimated':
            mesh = decimate_spec.decimate_spec(denoise_spec.cube(8)[0].astype(np.float32), denoise_spec.cube(8)[1], 192)[:2]
        elif name == 'sphere decimated':
            mesh = decimate_spec.decimate_spec(*smooth_spec.noisy_sphere(3), 600)[:2]
        elif name == 'patch':
            mesh = decimate_spec.patch(12)
        else:
            assert name == 'cubes welded'
            mesh = pieces_spec.welded((1, 1, 0))
        _base[name] = (np.ascontiguousarray(mesh[0], dtype=np.float32), np.ascontiguousarray(mesh[1], dtype=np.int64))
    return _base[name]


BASES = ('torus scrambled', 'sphere scrambled', 'cube decimated', 'sphere decimated', 'patch', 'cubes welded')
VARIANTS = ('', ' invalid', ' shuffled')
CASES = tuple(b + v for b in BASES for v in VARIANTS) + tuple('lattice {}'.format(n) for n in LATTICES) + ('empty', 'all invalid')


def case(name):
    """(verts f32, faces int64) of a named test mesh."""
    if name == 'empty':
        return base('patch')[0], np.zeros((0, 3), dtype=np.int64)
    if name == 'all invalid':
        return base('patch')[0], INVALID.copy()
    if name.startswith('lattice '):
        return jittered_lattice(int(name.split(' ')[1]))
    for k, variant in enumerate(VARIANTS[1:]):
        if name.endswith(variant):
            verts, faces = base(name[:-len(variant)])
            return verts, with_invalid(faces) if k == 0 else shuffled(faces, 70 + BASES.index(name[:-len(variant)]))
    return base(name)


def hand_cases():
    """[(name, verts f32 [4,3], faces int64 [2,3], max_angle, min_gain)]: the quads written out by hand that both tiers run."""
    quad = lambda pts, second=(1, 0, 3): (np.array(pts, dtype=np.float32), np.array([[0, 1, 2], list(second)], dtype=np.int64))
    long_diagonal = [(-2, 0, 0), (2, 0, 0), (0, 0.5, 0), (0, -0.5, 0)]
    return [('long diagonal',) + quad(long_diagonal) + (10.0, 1e-6),
            ('long diagonal, other slots',) + (quad(long_diagonal)[0], np.array([[2, 0, 1], [3, 1, 0]], dtype=np.int64)) + (10.0, 1e-6),
            ('long diagonal, other order',) + (quad(long_diagonal)[0], quad(long_diagonal)[1][::-1].copy()) + (10.0, 1e-6),
            ('square',) + quad([(0, 0, 0), (1, 1, 0), (0, 1, 0), (1, 0, 0)]) + (10.0, 0.0),
            ('non-convex',) + quad([(0, 0, 0), (2, 0, 0), (3, 1, 0), (3, -1, 0)]) + (90.0, 0.0),
            ('cap',) + quad([(-1, 0, 0), (1, 0, 0), (0, 0, 0), (0, -1, 0)]) + (10.0, 1e-6),
            ('two caps',) + quad([(-1, 0, 0), (1, 0, 0), (0, 0, 0), (0.5, 0, 0)]) + (10.0, 1e-6),
            ('crease 90',) + quad([(0, 0, 0), (1, 0, 0), (0.5, 0.1, 0), (0.5, 0, 0.1)]) + (10.0, 1e-6),
            ('crease 16.7 at 10',) + quad([(0, 0, 0), (1, 0, 0), (0.5, 0.1, 0), (0.5, -0.1, 0.03)]) + (10.0, 1e-6),
            ('crease 16.7 at 30',) + quad([(0, 0, 0), (1, 0, 0), (0.5, 0.1, 0), (0.5, -0.1, 0.03)]) + (30.0, 1e-6),
            ('twins',) + quad(long_diagonal, (0, 1, 2)) + (90.0, 0.0),
            ('mirror',) + quad(long_diagonal, (0, 2, 1)) + (90.0, 0.0),
            ('incoherent',) + quad(long_diagonal, (0, 1, 3)) + (90.0, 0.0)]
