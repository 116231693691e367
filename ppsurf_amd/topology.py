"""The topology layer of the mesh stages: faces -> sorted keys -> row tables, and the checks on a mesh argument.

smooth.py takes its adjacency from here, normals.py its incidence, fill.py its adjacency and its rims (section 19), pieces.py its
face pairs (section 21), orient.py the same pairs with their edge slots (section 23) and manifold.py those pairs and slots once more,
with the owner count of every edge (section 25), flip.py the same runs with their keys (section 27) and subdivide.py those runs and keys again (section 28); intersect.py takes only the checks (section 29); the hooking and compressing loop
that runs on those pairs is labels.py (section 26), the
frame of the commands mesh_cli.py; the valid-face rule on the device is csrc/pps_faces.h, the numpy restatement tests/topology_spec.py.  One key
kernel per face, one torch.sort, the sentinel keys of the invalid faces dropped from the end, ops.row_offsets for the rows.
"""
import torch

from . import _lib, ops

SENTINEL = 2 ** 63 - 1                     # KEY_SENTINEL of csrc/pps_faces.h: the keys of an invalid face, they sort last
MAX_COUNT = 2 ** 31 - 1                    # vertices and faces: a key is (row << 32) | entry


class CpuTensorError(_lib.PpsError, ValueError):
    """CPU tensors given to a mesh stage (smooth_mesh, vertex_normals, point_normals, ...): the PpsError of every module's device guard, and
    a ValueError like their other argument errors."""


def need_device(what, *tensors):
    try:
        return _lib.need_device(what, *tensors)
    except _lib.PpsError as e:
        raise CpuTensorError(str(e)) from None


def checked_mesh(what, verts, faces, limit=False, finite=True):
    """(verts f32 contiguous, faces contiguous) of a device mesh, or a ValueError: non-finite vertices (unless `finite` is off: intersect.py
    takes them, a face with such a corner is not live there), with `limit` more than 2^31 - 1 vertices or faces."""
    assert verts.dim() == 2 and verts.shape[1] == 3 and faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    v, f = verts.contiguous().float(), faces.contiguous()
    if limit and (v.shape[0] > MAX_COUNT or f.shape[0] > MAX_COUNT):
        raise ValueError('{}: at most 2^31 - 1 vertices and faces, got {} and {}'.format(what, v.shape[0], f.shape[0]))
    if finite and not bool(torch.isfinite(v).all()):
        raise ValueError('{}: the mesh has non-finite vertices'.format(what))
    return v, f


def valid_faces(faces, nv):
    """bool [nf]: the faces int64 [nf,3] whose indices lie in [0, nv) and are pairwise distinct -- the rule of csrc/pps_faces.h and of
    tests/topology_spec.py as a torch expression, for the stages that filter the faces themselves.  Only comparisons: CPU tensors work too."""
    f = faces
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0]) & ((f >= 0) & (f < nv)).all(dim=1)


def used_rows(faces, n):
    """(used bool [n], remap int64 [n]) of faces that index n rows: which rows a face uses, and remap = cumsum(used) - 1, the row of every
    used one after the unused are dropped with the order kept.  `verts[used]` and `remap[faces]` are the compacted mesh."""
    used = torch.zeros(n, dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    return used, torch.cumsum(used, 0) - 1


def live_keys(keys):
    """The keys int64 of a key entry in ascending order without the SENTINEL ones."""
    keys = torch.sort(keys)[0]
    return keys[keys != SENTINEL]


def sorted_keys(entry, per_face, faces, nv):
    """(live keys int64 ascending, valid faces) of a key entry on contiguous device faces: ppsx_smooth_half_edges writes 6 keys per face,
    (src << 32) | dst, and ppsx_normals_corner_keys 3, (vertex << 32) | face; an invalid face gets SENTINEL for all of them, and those leave."""
    nf = int(faces.shape[0])
    keys = torch.empty(per_face * nf, dtype=torch.int64, device=faces.device)
    _lib.call(entry, faces, nf, nv, keys)
    keys = live_keys(keys)
    return keys, int(keys.shape[0]) // per_face


def adjacency_rows(faces, nv):
    """(offsets, nbr, mult, valid faces) of contiguous device faces."""
    keys, valid = sorted_keys('ppsx_smooth_half_edges', 6, faces, nv)
    uniq, counts = torch.unique_consecutive(keys, return_counts=True)
    return ops.row_offsets(uniq >> 32, nv), (uniq & 0xFFFFFFFF).to(torch.int32), counts.to(torch.int32), valid


def incidence_rows(faces, nv):
    """(offsets, inc, valid faces) of contiguous device faces."""
    keys, valid = sorted_keys('ppsx_normals_corner_keys', 3, faces, nv)
    return ops.row_offsets(keys >> 32, nv), (keys & 0xFFFFFFFF).to(torch.int32), valid


def rim_rows(faces, nv, offsets, nbr, mult):
    """(succ int32 [nv], candidates int64 ascending, rim half-edges, rim vertices, simple rim vertices) of contiguous device faces and their
    adjacency_rows: the rim half-edges of DESIGN.md section 19 (an edge of one valid face, loose triangles left out) as sorted keys
    (src << 32) | dst, how many leave and enter every vertex, succ = the destination where exactly one leaves and one enters and -1
    elsewhere, and the vertices with a succ.  The key count is no multiple of a face count, so this does not go through sorted_keys."""
    nf = int(faces.shape[0])
    keys = torch.empty(3 * nf, dtype=torch.int64, device=faces.device)
    _lib.call('ppsx_fill_rim_keys', faces, nf, nv, offsets, nbr, mult, int(nbr.shape[0]), keys)
    keys = live_keys(keys)
    dst = keys & 0xFFFFFFFF
    rows = ops.row_offsets(keys >> 32, nv)
    leave, enter = rows[1:] - rows[:-1], torch.bincount(dst, minlength=nv)
    simple = (leave == 1) & (enter == 1)
    cand = torch.nonzero(simple).reshape(-1)
    succ = torch.full((nv,), -1, dtype=torch.int32, device=faces.device)
    succ[cand] = dst[rows[:-1][cand]].to(torch.int32)
    return succ, cand, int(keys.shape[0]), int(((leave > 0) | (enter > 0)).sum().item()), int(cand.shape[0])


def manifold_pair_edges(faces, nv):
    """(fa, fb, ea, eb int32 [np], valid bool [nf]) of contiguous device faces: the pairs of valid faces that share an undirected edge
    which exactly two valid faces hold (an edge with one owner or with three and more gives no pair, a duplicated face
    is two faces), the slot of that edge in each face (slot k is corner k -> corner k + 1 mod 3; section 23), and which faces are valid.
    ppsx_pieces_edge_keys writes 3 keys per face, (min << 32) | max, one sort with indices puts equal edges side by side, and the runs of
    exactly two give the pairs; the owner of a key is its position // 3 and its slot the position % 3, so two copies of one triangle are
    three pairs with their own slots.  The pairs are a set: their order, and which owner comes first, follow the sort."""
    return pairs_of_runs(*edge_runs(faces, nv))


def edge_runs(faces, nv):
    """(order int64 [3 nf], first int64 [ne], owners int64 [ne], valid bool [nf]) of contiguous device faces: the ne distinct undirected
    edges of the valid faces in ascending key.  ppsx_pieces_edge_keys writes 3 keys per face, (min << 32) | max, and one sort with indices
    puts equal edges side by side: edge e is the sorted positions first[e] .. first[e] + owners[e] - 1, and order gives the unsorted
    position of each, whose owner is position // 3 and whose slot is position % 3.  owners == 1 is a border edge, 2 a manifold one, 3 and
    more a non-manifold one (section 25 counts them).  Where there are invalid faces their SENTINEL keys form one more run at the end,
    with owners 0, so that no compaction (and no synchronisation) is spent on it here."""
    return edge_runs_keys(faces, nv)[:4]


def edge_runs_keys(faces, nv):
    """edge_runs with a fifth entry, keys int64 [ne]: the key of every run, ascending and distinct, the SENTINEL of the run of the invalid
    faces last where there is one.  flip.py looks up in them whether an edge exists; subdivide.py reads the two
    ends of every edge from them (section 28)."""
    nf = int(faces.shape[0])
    keys = torch.empty(3 * nf, dtype=torch.int64, device=faces.device)
    if nf == 0:
        return keys, keys, keys, keys.bool(), keys
    _lib.call('ppsx_pieces_edge_keys', faces, nf, nv, keys)
    valid = keys[0::3] != SENTINEL
    keys, order = torch.sort(keys)
    uniq, counts = torch.unique_consecutive(keys, return_counts=True)
    return order, torch.cumsum(counts, 0) - counts, torch.where(uniq != SENTINEL, counts, torch.zeros_like(counts)), valid, uniq


def pairs_of_runs(order, first, owners, valid):
    """manifold_pair_edges from the edge_runs of the same faces: the runs of exactly two."""
    first = first[owners == 2]
    one, two = order[first], order[first + 1]
    return (one // 3).to(torch.int32), (two // 3).to(torch.int32), (one % 3).to(torch.int32), (two % 3).to(torch.int32), valid


def manifold_pairs(faces, nv):
    """(fa int32 [np], fb int32 [np], valid bool [nf]) of contiguous device faces: manifold_pair_edges without the slots."""
    fa, fb, _, _, valid = manifold_pair_edges(faces, nv)
    return fa, fb, valid


def mesh_adjacency(faces: torch.Tensor, nv: int):
    """(offsets int64 [nv + 1], nbr int32 [ne], mult int32 [ne]) on the device: row i lists the distinct vertices that share a valid face
    with vertex i, ascending, and the number of valid faces on each of those edges.  A face is valid when its indices lie in [0, nv) and
    are pairwise distinct.  One key per half-edge from the kernel, one sort, the distinct keys with their counts (ops.row_offsets says why
    not pps_csr; a fan vertex of a simplified mesh is a crowded row).  Does not depend on the order of the faces."""
    need_device('mesh_adjacency', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_COUNT:
        raise ValueError('nv must be in 0..2^31 - 1, got {}'.format(nv))
    return adjacency_rows(faces.contiguous(), int(nv))[:3]


def vertex_incidence(faces: torch.Tensor, nv: int):
    """(offsets int64 [nv + 1], inc int32 [ni]) on the device: row i lists the valid faces that hold vertex i in ascending face index (a
    duplicated face is two faces).  A face is valid when its indices lie in [0, nv) and are pairwise distinct.  One key per corner from the
    kernel and one sort; the keys are distinct, so the rows do not depend on the sort implementation."""
    need_device('vertex_incidence', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_COUNT or faces.shape[0] > MAX_COUNT:
        raise ValueError('nv and the number of faces must be in 0..2^31 - 1, got {} and {}'.format(nv, faces.shape[0]))
    return incidence_rows(faces.contiguous(), int(nv))[:2]
