"""numpy restatement of the isotropic remeshing (ppsurf_amd/csrc/pps_remesh.hip, ppsurf_amd/remesh.py): the specification
the GPU is held to, byte for byte.  Every fp64 step is one numpy float64 operation in the order the kernels use; nothing here comes from the
device.  The rows, the regular vertices, the priorities and the winners are those of decimate_spec (section 22); the sequential sums of the
relaxation run in turns, as there.

Short-edge collapse, per round, on the positions P float64 [nv,3] and the current faces F (all valid):
  candidate       an adjacency entry (a, b), a < b, both ends regular, that passes section 22's link rule, with
                  len2 = (dx dx + dy dy) + dz dz < min2; with mid = (P_a + P_b) * 0.5 every face of the list of section 22 that holds one end
                  only keeps (n . n') > 0 with that corner at mid (a face without area at an end blocks the collapse); and every w of the
                  rows of a and b other than a, b has |P_w - mid|^2 <= max2.
  priority        (the bits of len2, h(key), key); the winners of section 22 all collapse: P_a = mid + 0.0, every b becomes a.
The rounds end when an evaluation finds no candidate (converged) or after max_rounds rounds.

Tangential relaxation, per pass, a Jacobi step from x to y: a regular vertex v has d = (the mean of its row) - P_v, N = the sum of the cross
products of its faces, t = d - N * ((N . d) / (N . N)), P' = P_v + lam * t.  State 0: not regular, copied.  State 2: N . N is 0 or not finite
or t is not finite, copied.  State 3: a face of v with v at P' and the other corners where they were does not keep (n . n') > 0, copied.
State 1: moved.

The loop: per iteration split_long_edges(max_edge = 4/3 L), collapse_short_edges(4/5 L, 4/3 L), flip_edges(flip_angle),
relax_tangential(1, relax_lam), float32 meshes between them: the chain of subdivide_spec, collapse_spec, flip_spec and relax_spec.
"""
import numpy as np

import decimate_spec as DS
import flip_spec
import smooth_spec
import subdivide_spec
from decimate_spec import _cross, _dot, _expand, _turn_sums
from topology_spec import adjacency, incidence, valid_faces

D = np.float64
U = np.uint64
NONE = DS.NONE


# ---- short-edge collapse ---------------------------------------------------------------------------------------------------------------------
def short_edges_spec(P, F, offsets, nbr, inc_offsets, inc, regular, min2, max2):
    """prio uint64 [ne,3] per adjacency entry."""
    nv, ne = offsets.shape[0] - 1, nbr.shape[0]
    nbr = np.asarray(nbr, dtype=np.int64)
    prio = np.full((ne, 3), NONE, dtype=U)
    src = DS.sources(offsets)
    ent = np.nonzero((src < nbr) & regular[src] & regular[nbr])[0]
    if ent.shape[0] == 0:
        return prio
    a, b = src[ent], nbr[ent]
    ka, pa = _expand(offsets, a)
    kb, pb = _expand(offsets, b)
    common = np.intersect1d(ka * nv + nbr[pa], kb * nv + nbr[pb], assume_unique=True)
    owner = common // nv
    two = np.bincount(owner, minlength=ent.shape[0]) == 2
    first = np.searchsorted(owner, np.nonzero(two)[0])
    ent, a, b = ent[two], a[two], b[two]
    c, d = common[first] % nv, common[first + 1] % nv
    with np.errstate(all='ignore'):
        delta = P[b] - P[a]
        len2 = _dot(delta, delta)
        short = len2 < D(min2)
    ent, a, b, c, d, len2 = ent[short], a[short], b[short], c[short], d[short], len2[short]
    n_e = ent.shape[0]
    if n_e == 0:
        return prio
    fa_own, fa_pos = _expand(inc_offsets, a)
    fb_own, fb_pos = _expand(inc_offsets, b)
    fa, fb = inc[fa_pos], inc[fb_pos]

    def holds(face, v):
        return (F[face] == v[:, None]).any(axis=1)

    tet_a = np.bincount(fa_own[holds(fa, c[fa_own]) & holds(fa, d[fa_own])], minlength=n_e) > 0
    tet_b = np.bincount(fb_own[holds(fb, c[fb_own]) & holds(fb, d[fb_own])], minlength=n_e) > 0
    keep_b = ~holds(fb, a[fb_own])
    own, face = np.concatenate([fa_own, fb_own[keep_b]]), np.concatenate([fa, fb[keep_b]])
    with np.errstate(all='ignore'):
        mid = (P[a] + P[b]) * D(0.5)
        q = [P[F[face, i]] - mid[own] for i in range(3)]
        n = _cross(q[1] - q[0], q[2] - q[0])
        ends = [(F[face, i] == a[own]) | (F[face, i] == b[own]) for i in range(3)]
        moved = [np.where(ends[i][:, None], D(0.0), q[i]) for i in range(3)]
        after = _cross(moved[1] - moved[0], moved[2] - moved[0])
        one_end = (ends[0].astype(int) + ends[1] + ends[2]) == 1
        folds = np.bincount(own[one_end & ~(_dot(n, after) > 0)], minlength=n_e) > 0
        longer = np.zeros(n_e, dtype=bool)
        for end in (a, b):
            k, p = _expand(offsets, end)
            w = nbr[p]
            w_ok = (w >= 0) & (w < nv) & (w != a[k]) & (w != b[k])
            k, w = k[w_ok], w[w_ok]
            qq = P[w] - mid[k]
            longer |= np.bincount(k[~(_dot(qq, qq) <= D(max2))], minlength=n_e) > 0
    cand = ~(tet_a & tet_b) & ~folds & ~longer
    key = (a.astype(U) << U(32)) | b.astype(U)
    prio[ent[cand]] = np.stack([len2.view(U), DS.mix(key), key], axis=1)[cand]
    return prio


def round_spec(P, F, nv, min2, max2):
    """Everything a collapse round computes, by name."""
    offsets, nbr, mult = adjacency(F, nv)
    inc_offsets, inc = incidence(F, nv)
    regular = DS.regular_spec(offsets, mult, inc_offsets)
    prio = short_edges_spec(P, F, offsets, nbr, inc_offsets, inc, regular, min2, max2)
    m1 = DS.vertex_min_spec(offsets, nbr, prio)
    best = DS.ring_min_spec(offsets, nbr, m1)
    return {'offsets': offsets, 'nbr': nbr, 'mult': mult, 'inc_offsets': inc_offsets, 'inc': inc, 'regular': regular, 'prio': prio, 'm1': m1,
            'best': best, 'flag': DS.winners_spec(offsets, nbr, prio, best), 'src': DS.sources(offsets)}


def bounds2(min_edge, max_edge):
    """(min2, max2) as the host forms them: one float64 product each, +inf without an upper bound."""
    return D(min_edge) * D(min_edge), (D(np.inf) if max_edge is None else D(max_edge) * D(max_edge))


def collapse_rows_spec(verts, faces, min_edge, max_edge=None, max_rounds=1000):
    """(kept, verts float32, faces int64, info): collapse_spec with the input row of every output vertex (a moved vertex has the row of the
    surviving end of its collapses)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    F = f[valid_faces(f, nv)]
    min2, max2 = bounds2(min_edge, max_edge)
    info = {'faces_in': int(f.shape[0]), 'faces_valid': int(F.shape[0]), 'faces_out': int(f.shape[0]), 'vertices_in': nv, 'vertices_out': nv,
            'rounds': 0, 'collapses': 0, 'candidates': 0, 'locked_vertices': 0, 'converged': True, 'min_edge': float(min_edge),
            'max_edge': None if max_edge is None else float(max_edge), 'max_rounds': int(max_rounds)}
    if F.shape[0] == 0:
        return np.arange(nv), v, f, info
    P, first = v.astype(D), True
    while True:
        r = round_spec(P, F, nv, min2, max2)
        count = int((r['prio'][:, 0] != NONE).sum())
        if first:
            info['candidates'], info['locked_vertices'], first = count, int((~r['regular']).sum()), False
        if count == 0 or info['rounds'] == max_rounds:
            info['converged'] = count == 0
            break
        win = np.nonzero(r['flag'])[0]
        assert win.shape[0] > 0
        a, b = r['src'][win], r['nbr'][win]
        P[a] = (P[a] + P[b]) * D(0.5) + D(0.0)
        rename = np.arange(nv, dtype=np.int64)
        rename[b] = a
        G, keep = DS.rename_spec(F, rename)
        F = G[keep]
        info['rounds'] += 1
        info['collapses'] += int(win.shape[0])
    if info['collapses'] == 0:
        return np.arange(nv), v, f, info
    used = np.zeros(nv, dtype=bool)
    used[F.reshape(-1)] = True
    info.update(faces_out=int(F.shape[0]), vertices_out=int(used.sum()))
    return np.nonzero(used)[0], P[used].astype(np.float32), (np.cumsum(used) - 1)[F], info


def collapse_spec(verts, faces, min_edge, max_edge=None, max_rounds=1000):
    """(verts float32, faces int64, info) of remesh.collapse_short_edges."""
    return collapse_rows_spec(verts, faces, min_edge, max_edge, max_rounds)[1:]


# ---- tangential relaxation -------------------------------------------------------------------------------------------------------------------
def relax_pass_spec(x, F, offsets, nbr, inc_offsets, inc, regular, lam):
    """(y float64 [nv,3], state uint8 [nv]) of one pass over x; F are the faces as given, the rows name the valid ones."""
    nv, nf = x.shape[0], F.shape[0]
    nbr, inc = np.asarray(nbr, dtype=np.int64), np.asarray(inc, dtype=np.int64)
    y, state = x.copy(), np.zeros(nv, dtype=np.uint8)
    rows = np.nonzero(regular)[0]
    n_r = rows.shape[0]
    if n_r == 0:
        return y, state

    def lists_of(own):
        out = np.zeros(n_r + 1, dtype=np.int64)
        out[1:] = np.cumsum(np.bincount(own, minlength=n_r))
        return out

    own, pos = _expand_checked(offsets, nbr.shape[0], rows)
    w = nbr[pos]
    ok = (w >= 0) & (w < nv)
    own, w = own[ok], w[ok]
    fown, fpos = _expand_checked(inc_offsets, inc.shape[0], rows)
    t = inc[fpos]
    ok = (t >= 0) & (t < nf)
    fown, t = fown[ok], t[ok]
    ok = valid_faces(F[t], nv)
    fown, t = fown[ok], t[ok]
    with np.errstate(all='ignore'):
        s = _turn_sums(x[w], lists_of(own))
        count = np.bincount(own, minlength=n_r).astype(D)
        pv = x[rows]
        d = s / count[:, None] - pv
        g = [x[F[t, i]] for i in range(3)]
        n = _cross(g[1] - g[0], g[2] - g[0])
        N = _turn_sums(n, lists_of(fown))
        nn, nd = _dot(N, N), _dot(N, d)
        r = nd / nn
        tang = d - N * r[:, None]
        bad = (nn == 0.0) | ~np.isfinite(nn) | ~np.isfinite(tang).all(axis=1)
        q = pv + D(lam) * tang
        h = [np.where((F[t, i] == rows[fown])[:, None], q[fown], g[i]) for i in range(3)]
        after = _cross(h[1] - h[0], h[2] - h[0])
        folds = np.bincount(fown[~(_dot(n, after) > 0)], minlength=n_r) > 0
    st = np.where(bad, 2, np.where(folds, 3, 1)).astype(np.uint8)
    state[rows] = st
    y[rows[st == 1]] = q[st == 1]
    return y, state


def _expand_checked(offsets, count, rows):
    """decimate_spec._expand with every row that cannot be read taken as empty: a row must satisfy 0 <= o0 <= o1 <= count."""
    o0, o1 = offsets[rows], offsets[rows + 1]
    ok = (o0 >= 0) & (o0 <= o1) & (o1 <= count)
    n = np.where(ok, o1 - o0, 0)
    owner = np.repeat(np.arange(rows.shape[0], dtype=np.int64), n)
    within = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    return owner, np.repeat(np.where(ok, o0, 0), n) + within


def mesh_rows(faces, nv):
    """The rows of a pass over the faces as given: adjacency and incidence of the valid ones and the regular vertices."""
    offsets, nbr, mult = adjacency(faces, nv)
    inc_offsets, inc = incidence(faces, nv)
    return {'offsets': offsets, 'nbr': nbr, 'mult': mult, 'inc_offsets': inc_offsets, 'inc': inc, 'regular': DS.regular_spec(offsets, mult, inc_offsets)}


def relax_spec(verts, faces, iters=1, lam=0.5):
    """(verts float32, faces as given, info) of remesh.relax_tangential."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    info = {'vertices': nv, 'regular': 0, 'moved': 0, 'states': [0, 0, 0, 0], 'iters': int(iters), 'lam': float(lam)}
    if nv == 0 or f.shape[0] == 0:
        return v, f, info
    r = mesh_rows(f, nv)
    info['regular'] = int(r['regular'].sum())
    if iters == 0:
        return v, f, info
    x = v.astype(D)
    for _ in range(int(iters)):
        x, state = relax_pass_spec(x, f, r['offsets'], r['nbr'], r['inc_offsets'], r['inc'], r['regular'], lam)
    out = x.astype(np.float32)
    info['moved'] = int((out.view(np.int32) != v.view(np.int32)).any(axis=1).sum())
    info['states'] = np.bincount(state, minlength=4).astype(int).tolist()
    return out, f, info


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def bounds_of(target):
    """(low, high) = (4/5, 4/3) of the target edge, as the host forms them."""
    return (4.0 * target) / 5.0, (4.0 * target) / 3.0


def remesh_rows_spec(verts, faces, target_edge=None, factor=None, iters=5, relax_lam=0.5, flip_angle=10.0, max_faces=None, colors=None):
    """(origin, verts float32, faces int64, colors, info): remesh_spec with the input row of every output vertex (-1 for a vertex that a split
    made; a vertex moved by a collapse has the row of the surviving end) and the colours carried along by the rules of the command."""
    assert (target_edge is None) != (factor is None)
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(f, v.shape[0])
    target = float(target_edge) if factor is None else float(factor) * (subdivide_spec.median_edge(v, np.where(ok[:, None], f, -1)) if ok.any() else 0.0)
    low, high = bounds_of(target)
    info = {'target_edge': target, 'low': low, 'high': high, 'faces_in': int(f.shape[0]), 'faces_out': int(f.shape[0]), 'vertices_in': int(v.shape[0]),
            'vertices_out': int(v.shape[0]), 'iters': int(iters), 'relax_lam': float(relax_lam), 'flip_angle': float(flip_angle),
            'max_faces': subdivide_spec.MAX_FACES if max_faces is None else int(max_faces), 'iterations': [], 'limited': False}
    origin = np.arange(v.shape[0], dtype=np.int64)
    if not ok.any() or not target > 0.0:
        return origin, v, f, colors, info
    V, F = v, f
    for _ in range(int(iters)):
        V, F, ends, split = subdivide_spec.subdivide_spec(V, F, max_edge=high, max_faces=max_faces)
        origin = np.concatenate([origin, np.full(split['splits'], -1, dtype=np.int64)])
        if colors is not None:
            colors = subdivide_spec.interpolate_colors(colors, ends, split['added'])
        kept, V, F, collapse = collapse_rows_spec(V, F, low, high)
        origin = origin[kept]
        if colors is not None:
            colors = np.asarray(colors)[kept]
        V, F, flips = flip_spec.flip_spec(V, F, flip_angle)
        V, F, relax = relax_spec(V, F, 1, relax_lam)
        info['iterations'].append({'splits': split['splits'], 'collapses': collapse['collapses'], 'flips': flips['flips'], 'moved': relax['moved']})
        info['limited'] = info['limited'] or bool(split['limited'])
    info.update(faces_out=int(F.shape[0]), vertices_out=int(V.shape[0]))
    return origin, V, F, colors, info


def remesh_spec(verts, faces, target_edge=None, factor=None, iters=5, relax_lam=0.5, flip_angle=10.0, max_faces=None):
    """(verts float32, faces int64, info) of remesh.remesh_isotropic."""
    out = remesh_rows_spec(verts, faces, target_edge, factor, iters, relax_lam, flip_angle, max_faces)
    return out[1], out[2], out[4]


# ---- measures ----------------------------------------------------------------------------------------------------------------------------------
def edge_lengths(verts, faces):
    """float64: the lengths of the distinct edges of the valid faces."""
    f = np.asarray(faces, dtype=np.int64)
    f = f[valid_faces(f, np.asarray(verts).shape[0])]
    return np.sqrt(subdivide_spec.edge_lengths2(verts, f)[2])


def edge_cv(verts, faces):
    """The coefficient of variation of the edge lengths: standard deviation over mean."""
    e = edge_lengths(verts, faces)
    return float(e.std() / e.mean())


def small_corner_share(verts, faces, degrees=30.0):
    """The share of the corners of the valid faces below `degrees`."""
    f = np.asarray(faces, dtype=np.int64)
    a = flip_spec.angles(verts, f[valid_faces(f, np.asarray(verts).shape[0])])
    return float((a < degrees).mean())


def corner_histogram(verts, faces, edges=(0, 10, 20, 30, 40, 50, 60, 90, 120, 180.0001)):
    f = np.asarray(faces, dtype=np.int64)
    a = flip_spec.angles(verts, f[valid_faces(f, np.asarray(verts).shape[0])])
    return np.histogram(a, bins=np.array(edges))[0].tolist()


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------
PLANTED = 12
NEEDLE_SEED = 11


def needles():
    """(verts f32 [642,3], faces int64 [1280,3], planted int64 [PLANTED]): decimate_spec's noisy icosphere with PLANTED vertices -- the first
    of a default_rng(NEEDLE_SEED) permutation that lie more than three rings from every one taken before -- each pulled to within a
    hundredth of an edge of its smallest neighbour: P_v = P_w + (P_v - P_w) * 0.005."""
    verts, faces = smooth_spec.noisy_sphere(3)
    nv = verts.shape[0]
    offsets, nbr, _ = adjacency(faces, nv)
    taken, blocked = [], np.zeros(nv, dtype=bool)
    for v in np.random.default_rng(NEEDLE_SEED).permutation(nv).tolist():
        if blocked[v]:
            continue
        taken.append(v)
        ring = np.array([v])
        for _ in range(3):
            ring = np.unique(np.concatenate([ring] + [nbr[offsets[u]:offsets[u + 1]] for u in ring.tolist()]))
        blocked[ring] = True
        if len(taken) == PLANTED:
            break
    assert len(taken) == PLANTED
    out = verts.astype(D)
    for v in taken:
        w = int(nbr[offsets[v]])
        out[v] = out[w] + (out[v] - out[w]) * 0.005
    return out.astype(np.float32), faces, np.array(taken, dtype=np.int64)


def spindle(n=300):
    """(verts f32 [n + 2,3], faces int64 [2 n,3]): two apexes over a ring of n -- smooth_spec's closed fan.  Both apexes are regular vertices
    with rows of n entries: the closed counterpart of the open fan, whose hub is a border."""
    return smooth_spec.fan(n, closed=True)


def pillow():
    """(verts f32 [3,3], faces int64 [2,3]): one triangle and its mirror image on the same three vertices.  Every vertex is regular -- two
    neighbours, two faces, both edges shared by two faces -- and the cross products of its faces sum to zero: state 2."""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32), np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int64)


def four_states():
    """(verts f32, faces int64): decimate_spec's open patch (its border: state 0, its interior: state 1) with the face that holds the three
    interior vertices 40, 53, 54 made a face without area by putting 53 onto 40 (its corners: state 3; the other face on that edge has the
    border vertex 39 for its third corner) and a pillow far away (state 2)."""
    verts, faces = DS.patch()
    row = int(np.nonzero((np.sort(faces, axis=1) == np.array([40, 53, 54])).all(axis=1))[0][0])
    verts = verts.copy()
    assert faces[row].tolist() == [40, 53, 54]
    verts[53] = verts[40]
    pv, pf = pillow()
    return np.concatenate([verts, pv + np.float32(40.0)]), np.concatenate([faces, pf + verts.shape[0]])
