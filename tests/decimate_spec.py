"""numpy restatement of the edge-collapse decimation (ppsurf_amd/csrc/pps_decimate.hip, ppsurf_amd/decimate.py): the
specification the GPU is held to, byte for byte.  Every fp64 step is one numpy float64 operation in the order the kernels use; nothing here
comes from the device.  The sequential sums over an edge's face list run in turns -- "the k-th face of every list" -- so that every edge adds
its faces in list order, one rounding per addition.

Rule, per round, on the positions P float64 [nv,3] and the current faces F (all valid), with the adjacency rows (nbr ascending, mult) and the
incidence rows (faces ascending) of F:
  regular vertex  it has a face, every entry of its adjacency row has mult == 2, and its faces are as many as its neighbours.
  candidate       an adjacency entry (a, b), a < b, both ends regular, that passes the link rule, whose cost is finite and that folds no face.
  link rule       N(a) and N(b) share exactly two vertices c < d, and not (a face of a holds c and d, and a face of b holds c and d).
  face list       the faces of a ascending, then the faces of b that do not hold a, ascending.
  placement       mid = (P_a + P_b) * 0.5; per face of the list, q_i = P_i - mid, u = q_1 - q_0, w = q_2 - q_0, n = u x w (each component
                  p*q - r*s), m = (n_x q_0x + n_y q_0y) + n_z q_0z; A00 += n_x n_x ... A22 += n_z n_z, b_a += m n_a (simplify_spec's order);
                  lambda = 1e-3 * ((A00 + A11) + A22), M = A + lambda I, r = b, x from the cofactor formulas of simplify_spec.place.
                  x = (0, 0, 0), a fallback, when the trace is 0, a component of x is not finite or (x_0^2 + x_1^2) + x_2^2 > |P_b - P_a|^2.
  cost            over the same list: t = ((n_x x_0 + n_y x_1) + n_z x_2) - m, cost = cost + t * t from +0.0.
  fold rule       every face of the list that does not hold both ends, its end replaced by x, gives n' with (n_x n'_x + n_y n'_y) + n_z n'_z > 0.
  priority        (the bits of the cost as u64, h(key), key), key = (a << 32) | b, h = the splitmix64 finaliser of key + 0x9E3779B97F4A7C15;
                  compared lexicographically; every other entry has NONE three times.
  winners         m1[u] = the minimum over the candidates at u; best[w] = the minimum of m1 over {w} and N(w); an edge wins when
                  best[a] == best[b] == its priority.  With more winners than need = ceil((|F| - max_faces) / 2), the first `need` in
                  ascending priority.
  apply           P_a = mid + x; every b becomes a in F; the faces that now repeat a vertex leave, the rest keep their order.
The rounds end when |F| <= max_faces, when a round has no winner, or after max_rounds rounds.
"""
import numpy as np

from topology_spec import adjacency, incidence, valid_faces

D = np.float64
U = np.uint64
NONE = U(0xFFFFFFFFFFFFFFFF)
MAX_COUNT = 2 ** 31 - 1


def mix(key):
    """uint64: the splitmix64 finaliser of key + 0x9E3779B97F4A7C15, modulo 2^64."""
    with np.errstate(over='ignore'):
        z = np.asarray(key, dtype=U) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def sources(offsets):
    """int64 [ne]: the row of every entry."""
    return np.repeat(np.arange(offsets.shape[0] - 1, dtype=np.int64), np.diff(offsets))


def regular_spec(offsets, mult, inc_offsets):
    """bool [nv]."""
    nv = offsets.shape[0] - 1
    faces_at, nbrs_at = np.diff(inc_offsets), np.diff(offsets)
    odd = np.bincount(sources(offsets)[mult != 2], minlength=nv) > 0
    return (faces_at >= 1) & ~odd & (faces_at == nbrs_at)


def _expand(offsets, rows):
    """(owner, position): the entries of the rows `rows` one after the other; owner indexes `rows`."""
    n = offsets[rows + 1] - offsets[rows]
    owner = np.repeat(np.arange(rows.shape[0], dtype=np.int64), n)
    within = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    return owner, np.repeat(offsets[rows], n) + within


def _turn_sums(values, offsets):
    """out[r] = ((0 + values[o_r]) + values[o_r + 1]) + ...: one turn per position of the lists."""
    rows = offsets.shape[0] - 1
    length = np.diff(offsets)
    out = np.zeros((rows,) + values.shape[1:], dtype=D)
    for k in range(int(length.max()) if rows else 0):
        live = np.nonzero(length > k)[0]
        out[live] = out[live] + values[offsets[live] + k]
    return out


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def _dot(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]


def solve(A, b):
    """x [n,3] of (A + lambda I) x = b with simplify_spec.place's formulas, and the trace."""
    a00, a01, a02, a11, a12, a22 = (A[:, i] for i in range(6))
    with np.errstate(all='ignore'):
        trace = (a00 + a11) + a22
        lam = D(1e-3) * trace
        m00, m11, m22, m01, m02, m12 = a00 + lam, a11 + lam, a22 + lam, a01, a02, a12
        r0, r1, r2 = b[:, 0], b[:, 1], b[:, 2]
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
    return x, trace


def edges_spec(P, F, offsets, nbr, inc_offsets, inc, regular):
    """(prio uint64 [ne,3], x float64 [ne,3], fell bool [ne]) per adjacency entry: rules (1) to (6).  x and fell are zero where the entry is
    no candidate."""
    nv, ne = offsets.shape[0] - 1, nbr.shape[0]
    prio, X, fell_out = np.full((ne, 3), NONE, dtype=U), np.zeros((ne, 3), dtype=D), np.zeros(ne, dtype=bool)
    src = sources(offsets)
    ent = np.nonzero((src < nbr) & regular[src] & regular[nbr])[0]
    if ent.shape[0] == 0:
        return prio, X, fell_out
    a, b = src[ent], nbr[ent]
    # the link rule: the common neighbours by a merge of the two rows
    ka, pa = _expand(offsets, a)
    kb, pb = _expand(offsets, b)
    common = np.intersect1d(ka * nv + nbr[pa], kb * nv + nbr[pb], assume_unique=True)
    owner = common // nv
    two = np.bincount(owner, minlength=ent.shape[0]) == 2
    ent, a, b = ent[two], a[two], b[two]
    first = np.searchsorted(owner, np.nonzero(two)[0])
    c, d = common[first] % nv, common[first + 1] % nv
    # the face list
    fa_own, fa_pos = _expand(inc_offsets, a)
    fb_own, fb_pos = _expand(inc_offsets, b)
    fa, fb = inc[fa_pos], inc[fb_pos]

    def holds(face, v):
        return (F[face] == v[:, None]).any(axis=1)

    n_e = ent.shape[0]
    tet_a = np.bincount(fa_own[holds(fa, c[fa_own]) & holds(fa, d[fa_own])], minlength=n_e) > 0
    tet_b = np.bincount(fb_own[holds(fb, c[fb_own]) & holds(fb, d[fb_own])], minlength=n_e) > 0
    keep_b = ~holds(fb, a[fb_own])
    own, face = np.concatenate([fa_own, fb_own[keep_b]]), np.concatenate([fa, fb[keep_b]])
    order = np.argsort(own, kind='stable')
    own, face = own[order], face[order]
    lists = np.zeros(n_e + 1, dtype=np.int64)
    lists[1:] = np.cumsum(np.bincount(own, minlength=n_e))
    with np.errstate(all='ignore'):
        mid = (P[a] + P[b]) * D(0.5)
        q = [P[F[face, i]] - mid[own] for i in range(3)]
        n = _cross(q[1] - q[0], q[2] - q[0])
        m = _dot(n, q[0])
        terms = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                          m * n[:, 0], m * n[:, 1], m * n[:, 2]], axis=1)
        sums = _turn_sums(terms, lists)
        x, trace = solve(sums[:, :6], sums[:, 6:])
        delta = P[b] - P[a]
        ok = (trace != 0.0) & np.isfinite(x).all(axis=1) & ~(_dot(x, x) > _dot(delta, delta))
        x = np.where(ok[:, None], x, D(0.0))
        t = _dot(n, x[own]) - m
        cost = _turn_sums(t * t, lists)
        # the fold rule
        ends = [(F[face, i] == a[own]) | (F[face, i] == b[own]) for i in range(3)]
        moved = [np.where(ends[i][:, None], x[own], q[i]) for i in range(3)]
        after = _cross(moved[1] - moved[0], moved[2] - moved[0])
        one_end = (ends[0].astype(int) + ends[1] + ends[2]) == 1
        folds = np.bincount(own[one_end & ~(_dot(n, after) > 0)], minlength=n_e) > 0
    cand = ~(tet_a & tet_b) & np.isfinite(cost) & ~folds
    key = (a.astype(U) << U(32)) | b.astype(U)
    mine = np.stack([cost.view(U), mix(key), key], axis=1)
    prio[ent[cand]] = mine[cand]
    X[ent[cand]] = x[cand]
    fell_out[ent[cand]] = ~ok[cand]
    return prio, X, fell_out


def ascending(prio):
    """The order of the rows of prio uint64 [n,3], ascending and lexicographic."""
    return np.lexsort((prio[:, 2], prio[:, 1], prio[:, 0]))


def group_min(owner, prio, groups):
    """uint64 [groups,3]: the lexicographic minimum of the rows of prio per owner, NONE three times for a group without a row."""
    out = np.full((groups, 3), NONE, dtype=U)
    order = ascending(prio)[::-1]                                    # descending: the last write to a group is its minimum
    out[owner[order]] = prio[order]
    return out


def vertex_min_spec(offsets, nbr, prio):
    """m1 uint64 [nv,3]: the minimum over the entries of every row, the entry (u, v) with u > v read at its mirror (v, u)."""
    nv = offsets.shape[0] - 1
    src = sources(offsets)
    up = np.nonzero(src < nbr)[0]
    return group_min(np.concatenate([src[up], nbr[up]]), np.concatenate([prio[up], prio[up]]), nv)


def ring_min_spec(offsets, nbr, m1):
    """best uint64 [nv,3]: the minimum of m1 over a vertex and its row."""
    nv = offsets.shape[0] - 1
    return group_min(np.concatenate([np.arange(nv), sources(offsets)]), np.concatenate([m1, m1[nbr]]), nv)


def winners_spec(offsets, nbr, prio, best):
    """bool [ne]."""
    src = sources(offsets)
    live = (src < nbr) & (prio != NONE).any(axis=1)
    return live & (best[src] == prio).all(axis=1) & (best[nbr] == prio).all(axis=1)


def round_spec(P, F, nv):
    """Everything a round computes, by name."""
    offsets, nbr, mult = adjacency(F, nv)
    inc_offsets, inc = incidence(F, nv)
    regular = regular_spec(offsets, mult, inc_offsets)
    prio, x, fell = edges_spec(P, F, offsets, nbr, inc_offsets, inc, regular)
    m1 = vertex_min_spec(offsets, nbr, prio)
    best = ring_min_spec(offsets, nbr, m1)
    return {'offsets': offsets, 'nbr': nbr, 'mult': mult, 'inc_offsets': inc_offsets, 'inc': inc, 'regular': regular, 'prio': prio, 'x': x,
            'fell': fell, 'm1': m1, 'best': best, 'flag': winners_spec(offsets, nbr, prio, best), 'src': sources(offsets)}


def taken(prio, flag, need):
    """The winning entries, at most `need` of them: the first in ascending priority."""
    win = np.nonzero(flag)[0]
    if win.shape[0] > need:
        win = np.sort(win[ascending(prio[win])[:need]])
    return win


def rename_spec(F, rename):
    """(renamed faces, keep bool): keep where the three renamed indices are pairwise distinct."""
    G = rename[F]
    return G, (G[:, 0] != G[:, 1]) & (G[:, 1] != G[:, 2]) & (G[:, 2] != G[:, 0])


def decimate_spec(verts, faces, max_faces, max_rounds=1000):
    """(verts float32, faces int64, info) of decimate.decimate_mesh."""
    return decimate_rows_spec(verts, faces, max_faces, max_rounds)[1:]


def decimate_rows_spec(verts, faces, max_faces, max_rounds=1000):
    """(kept, verts float32, faces int64, info): decimate_spec with the input row of every output vertex (a moved vertex has the row of the
    surviving end of its collapses)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    F = f[valid_faces(f, nv)]
    info = {'faces_in': int(f.shape[0]), 'faces_valid': int(F.shape[0]), 'faces_out': int(f.shape[0]), 'vertices_in': nv, 'vertices_out': nv,
            'rounds': 0, 'collapses': 0, 'fallbacks': 0, 'locked_vertices': 0, 'reached': F.shape[0] <= max_faces, 'max_faces': int(max_faces),
            'max_rounds': int(max_rounds)}
    if F.shape[0] > 0:
        offsets, _, mult = adjacency(F, nv)
        info['locked_vertices'] = int((~regular_spec(offsets, mult, incidence(F, nv)[0])).sum())
    if F.shape[0] == 0 or F.shape[0] <= max_faces:
        return np.arange(nv), v, f, info
    P = v.astype(D)
    while F.shape[0] > max_faces and info['rounds'] < max_rounds:
        r = round_spec(P, F, nv)
        win = taken(r['prio'], r['flag'], (F.shape[0] - max_faces + 1) // 2)
        if win.shape[0] == 0:
            break
        a, b = r['src'][win], r['nbr'][win]
        P[a] = (P[a] + P[b]) * D(0.5) + r['x'][win]
        rename = np.arange(nv, dtype=np.int64)
        rename[b] = a
        G, keep = rename_spec(F, rename)
        F = G[keep]
        info['rounds'] += 1
        info['collapses'] += int(win.shape[0])
        info['fallbacks'] += int(r['fell'][win].sum())
    used = np.zeros(nv, dtype=bool)
    used[F.reshape(-1)] = True
    info.update(faces_out=int(F.shape[0]), vertices_out=int(used.sum()), reached=bool(F.shape[0] <= max_faces))
    return np.nonzero(used)[0], P[used].astype(np.float32), (np.cumsum(used) - 1)[F], info


# ---- measures ----------------------------------------------------------------------------------------------------------------------------------
def edge_owners(faces):
    """The number of faces on every undirected edge of the mesh."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def euler(verts, faces):
    """V - E + F with V the vertices that a face uses."""
    return int(np.unique(faces).shape[0]) - int(edge_owners(faces).shape[0]) + int(faces.shape[0])


def closed_manifold(verts, faces):
    """Every edge has exactly two owners, no face repeats as a vertex set, every face is valid."""
    f = np.asarray(faces, dtype=np.int64)
    return bool((edge_owners(f) == 2).all() and np.unique(np.sort(f, axis=1), axis=0).shape[0] == f.shape[0] and valid_faces(f, verts.shape[0]).all())


def signed_volume(verts, faces):
    p = np.asarray(verts, dtype=D)[faces]
    return float((_dot(p[:, 0], _cross(p[:, 1], p[:, 2]))).sum() / 6.0)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------
def octahedron():
    verts = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
    return verts, faces


def tetrahedron():
    verts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    return verts, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)


def torus(nu=16, nw=8):
    """(verts f32 [nu nw,3], faces int64 [2 nu nw,3]): a lattice of nu x nw quads on a torus of radii 2 and 0.7, every quad split alike."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nw), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    s, t = 2.0 * np.pi * i / nu, 2.0 * np.pi * j / nw
    verts = np.stack([(2.0 + 0.7 * np.cos(t)) * np.cos(s), (2.0 + 0.7 * np.cos(t)) * np.sin(s), 0.7 * np.sin(t)], axis=1).astype(np.float32)
    at = lambda p, r: (p % nu) * nw + r % nw
    quad = np.stack([at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)], axis=1)
    return verts, np.ascontiguousarray(np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]), dtype=np.int64)


def patch(n=12):
    """(verts f32 [(n + 1)^2,3], faces int64 [2 n^2,3]): a flat open lattice of n x n quads with the z noise 0.01 N(0,1) of default_rng(0)."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    verts = np.stack([i, j, 0.01 * np.random.default_rng(0).standard_normal(i.shape[0])], axis=1).astype(np.float32)
    qi, qj = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    qi, qj = qi.reshape(-1), qj.reshape(-1)
    at = lambda p, r: p * (n + 1) + r
    quad = np.stack([at(qi, qj), at(qi + 1, qj), at(qi + 1, qj + 1), at(qi, qj + 1)], axis=1)
    return verts, np.ascontiguousarray(np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]), dtype=np.int64)


def border_vertices(faces, nv):
    """bool [nv]: the vertices with an edge of one owner."""
    offsets, _, mult = adjacency(faces, nv)
    out = np.zeros(nv, dtype=bool)
    out[sources(offsets)[mult == 1]] = True
    return out


def named(name):
    """(verts f32, faces int64, max_faces) of the meshes both tiers run."""
    import denoise_spec
    import pieces_spec
    import smooth_spec
    if name == 'cube8':
        return denoise_spec.cube(8)[0].astype(np.float32), denoise_spec.cube(8)[1], 192
    if name == 'cube8:12':
        return denoise_spec.cube(8)[0].astype(np.float32), denoise_spec.cube(8)[1], 12
    if name == 'sphere':
        verts, faces = smooth_spec.noisy_sphere(3)
        return verts, faces, faces.shape[0] // 2
    if name == 'fan':
        verts, faces = smooth_spec.fan(300, closed=True)
        return verts, faces, faces.shape[0] // 2
    if name == 'torus':
        return torus() + (128,)
    if name == 'patch':
        return patch() + (144,)
    if name == 'welded':
        return pieces_spec.welded((1, 1, 0)) + (4,)
    if name == 'octahedron':
        return octahedron() + (4,)
    assert name == 'tetrahedron'
    return tetrahedron() + (4,)


NAMES = ('cube8', 'cube8:12', 'sphere', 'fan', 'torus', 'patch', 'welded', 'octahedron', 'tetrahedron')
CLOSED = {'cube8': 2, 'sphere': 2, 'fan': 2, 'torus': 0}          # name: V - E + F
