"""numpy restatement of the hole filling (ppsurf_amd/fill.py, ppsurf_amd/csrc/pps_fill.hip): rim half-edges, simple rim
vertices, a brute-force walk from every leader, the new vertices and faces.  Nothing here comes from the device.  The valid-face rule and the
adjacency are those of topology_spec.  Also the meshes the fill tests share: the height-field grid and the open cylinder.
"""
import numpy as np

import topology_spec as T

MAX_EDGES = 4096


def rim_half_edges(faces, nv):
    """(src int64 [r], dst int64 [r], loose triangles, border edges): the directed half-edges a->b, b->c, c->a of the valid, non-loose faces
    whose edge a single valid face holds, in face order; how many valid faces have three such edges; how many edges a single face holds."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    g = f[T.valid_faces(f, nv)]
    offsets, nbr, mult = T.adjacency(f, nv)
    rows = (np.repeat(np.arange(nv, dtype=np.int64), np.diff(offsets)) << 32) | nbr           # every half-edge once, ascending
    u, v = g, g[:, [1, 2, 0]]
    m = mult[np.searchsorted(rows, ((u << 32) | v).reshape(-1))].reshape(-1, 3) if g.shape[0] else np.zeros((0, 3), dtype=np.int64)
    loose = (m == 1).all(axis=1)
    rim = (m == 1) & ~loose[:, None]
    return u[rim], v[rim], int(loose.sum()), int((mult == 1).sum()) // 2


def successors(src, dst, nv):
    """(succ int64 [nv], rim vertices, simple rim vertices): succ(u) = the destination of the one rim half-edge that leaves u where exactly
    one leaves and exactly one enters, -1 elsewhere."""
    leave, enter = np.bincount(src, minlength=nv), np.bincount(dst, minlength=nv)
    simple = (leave == 1) & (enter == 1)
    succ = np.full(nv, -1, dtype=np.int64)
    pick = simple[src]
    succ[src[pick]] = dst[pick]
    return succ, int(((leave > 0) | (enter > 0)).sum()), int(simple.sum())


def loops(succ):
    """[[s_0, .., s_{L-1}], ..] in ascending leader s_0: every cycle of succ, of any length.  The walk starts at every vertex in ascending
    order and runs until it is back, meets a vertex without succ or meets a vertex an earlier walk has seen: that vertex lies on a chain
    that started at a smaller index, so the start is no leader (a cycle) or its chain ends where that one ended (no cycle)."""
    nv = succ.shape[0]
    seen = np.zeros(nv, dtype=bool)
    found = []
    for s in range(nv):
        if succ[s] < 0 or seen[s]:
            continue
        chain, cur = [], s
        while True:
            seen[cur] = True
            chain.append(cur)
            cur = int(succ[cur])
            if cur == s:
                assert min(chain) == s and len(chain) >= 3
                found.append(chain)
                break
            if cur < 0 or seen[cur]:
                break
    return found


def fill_spec(verts, faces, max_edges):
    """(verts f32 [nv + new, 3], faces int64 [nf + new, 3], info) by the rule of DESIGN.md section 19."""
    assert isinstance(max_edges, int) and 3 <= max_edges <= MAX_EDGES
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    nv = v.shape[0]
    src, dst, loose, border = rim_half_edges(f, nv)
    succ, rim_vertices, simple = successors(src, dst, nv)
    new_v, new_f, filled, edges = [], [], 0, 0
    for s in loops(succ):
        L = len(s)
        if L > max_edges:
            continue
        filled += 1
        edges += L
        if L == 3:
            new_f.append((s[0], s[2], s[1]))
            continue
        acc = np.zeros(3, dtype=np.float64)
        for j in s:
            acc = acc + v[j].astype(np.float64)
        c = nv + len(new_v)
        new_v.append((acc / np.float64(L)).astype(np.float32))
        new_f.extend((s[(j + 1) % L], s[j], c) for j in range(L))
    info = {'vertices': nv, 'faces_valid': int(T.valid_faces(f, nv).sum()), 'border_edges': border, 'loose_triangles': loose,
            'rim_vertices': rim_vertices, 'nonsimple_rim_vertices': rim_vertices - simple, 'loops_filled': filled, 'new_vertices': len(new_v),
            'new_faces': len(new_f), 'border_edges_left': border - edges, 'max_edges': max_edges}
    out_v = np.concatenate([v, np.asarray(new_v, dtype=np.float32).reshape(-1, 3)])
    out_f = np.concatenate([f, np.asarray(new_f, dtype=np.int64).reshape(-1, 3)])
    return out_v, out_f, info


def loop_lengths(faces, nv):
    """The lengths of all loops of a mesh, in ascending leader."""
    src, dst, _, _ = rim_half_edges(faces, nv)
    return [len(s) for s in loops(successors(src, dst, nv)[0])]


def directed_half_edge_counts(faces, nv):
    """How often each directed half-edge a->b, b->c, c->a of the valid faces occurs: the counts of the distinct ones."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    g = f[T.valid_faces(f, nv)]
    keys = ((g << 32) | g[:, [1, 2, 0]]).reshape(-1)
    return np.unique(keys, return_counts=True)[1]


# ---- the meshes of the tests ----------------------------------------------------------------------------------------------------------------
def height_grid(n):
    """(verts f32 [n n, 3], faces int64 [2 (n - 1)^2, 3]): vertex i n + j at (j, i, 0.1 sin(i) cos(j)), every cell split along the diagonal
    (i, j) - (i + 1, j + 1), consistently wound.  An interior vertex has six neighbours, the outer rim 4 (n - 1) edges."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    verts = np.stack([j, i, 0.1 * np.sin(i) * np.cos(j)], axis=-1).reshape(-1, 3).astype(np.float32)
    c = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1).astype(np.int64)
    faces = np.stack([np.stack([c, c + 1, c + n + 1], axis=1), np.stack([c, c + n + 1, c + n], axis=1)], axis=1).reshape(-1, 3)
    return verts, faces


def without_fans(faces, vertices):
    """The faces that hold none of `vertices`."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return f[~np.isin(f, np.asarray(vertices, dtype=np.int64)).any(axis=1)]


def open_cylinder(segments):
    """(verts f32 [2 segments, 3], faces int64 [2 segments, 3]): a tube of one ring of quads; vertex k on the lower rim, segments + k above
    it.  Both rims have `segments` edges.  The upper rim's half-edges run segments + k -> segments + k + 1: the indices ascend along it up to
    the wrap, the longest walks the rule allows (candidate segments + k walks segments - k steps before it meets its leader).  The lower
    rim's run k + 1 -> k: every candidate but the leader stops at its first step."""
    k = np.arange(segments, dtype=np.int64)
    t = 2.0 * np.pi * k / segments
    ring = np.stack([np.cos(t), np.sin(t)], axis=1)
    verts = np.concatenate([np.concatenate([ring, np.full((segments, 1), -0.5)], axis=1),
                            np.concatenate([ring, np.full((segments, 1), 0.5)], axis=1)]).astype(np.float32)
    n = (k + 1) % segments
    faces = np.stack([np.stack([k, segments + n, n], axis=1), np.stack([k, segments + k, segments + n], axis=1)], axis=1).reshape(-1, 3)
    return verts, faces
