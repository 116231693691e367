"""numpy restatements of the evaluation kernels (ppsurf_amd/csrc/pps_eval.hip) and meshes with known answers, for the tests."""
import numpy as np

_GAMMA, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(x):
    """splitmix64 finaliser of x + golden gamma, uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        z = np.asarray(x, dtype=np.uint64) + _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def sample_spec(corners, prefix, n, seed, stream_id):
    """The sampler of the header comment of pps_eval.hip (generator: pps_rng.h): (points f32 [n,3], face ids int64 [n]) from corners
    f32 [nf,9] and the fp64 inclusive area prefix."""
    corners = np.asarray(corners, dtype=np.float32)
    prefix = np.asarray(prefix, dtype=np.float64)
    key = mix64(mix64(np.uint64(seed)) ^ np.uint64(stream_id))
    ctr = np.arange(n, dtype=np.uint64) << np.uint64(2)
    u = (mix64(key ^ ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r1 = (mix64(key ^ (ctr | np.uint64(1))) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    r2 = (mix64(key ^ (ctr | np.uint64(2))) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    total = prefix[-1]
    face = np.searchsorted(prefix, u * total, side='right')
    face = np.where(face == prefix.shape[0], np.searchsorted(prefix, total, side='left'), face)
    fold = (r1 + r2) > np.float32(1.0)
    r1 = np.where(fold, np.float32(1.0) - r1, r1).astype(np.float32)
    r2 = np.where(fold, np.float32(1.0) - r2, r2).astype(np.float32)
    c = corners[face]
    v0, e1, e2 = c[:, 0:3], c[:, 3:6] - c[:, 0:3], c[:, 6:9] - c[:, 0:3]
    pts = (r1[:, None] * e1 + r2[:, None] * e2) + v0
    return pts.astype(np.float32), face


def face_stats_spec(verts, faces):
    """(area [nf], unit normal [nf,3], corners [nf,9]) in fp64."""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(cr, axis=1)
    normal = np.where(ln[:, None] > 0, cr / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    return 0.5 * ln, normal, v.reshape(-1, 9)


def winding_spec(verts, faces, pts, chunk=64):
    """Generalised winding number in fp64 by brute force: sum_f 2 atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi."""
    tri = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    pts = np.asarray(pts, dtype=np.float64)
    out = np.empty(pts.shape[0])
    for s in range(0, pts.shape[0], chunk):
        p = pts[s:s + chunk, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        la, lb, lc = [np.linalg.norm(x, axis=2) for x in (a, b, c)]
        det = np.einsum('qfi,qfi->qf', a, np.cross(b, c))
        den = la * lb * lc + np.einsum('qfi,qfi->qf', a, b) * lc + np.einsum('qfi,qfi->qf', b, c) * la + np.einsum('qfi,qfi->qf', c, a) * lb
        out[s:s + chunk] = np.arctan2(det, den).sum(axis=1) / (2.0 * np.pi)
    return out


def icosphere(subdiv, radius=1.0):
    """Subdivided icosahedron on a sphere of `radius`, faces counter-clockwise seen from outside -> (verts f64 [nv,3], faces int64 [nf,3])."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = f
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = verts[i] + verts[j]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return np.array(verts) * radius, np.array(faces, dtype=np.int64)


def mesh_volume(verts, faces):
    """Signed volume of a closed triangle mesh (positive for outward faces)."""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    return float(np.einsum('fi,fi->f', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def ply_header_counts(path):
    """{element name: count} from a PLY header."""
    counts = {}
    with open(path, 'rb') as f:
        for line in f:
            tok = line.decode('ascii', 'replace').split()
            if tok and tok[0] == 'element':
                counts[tok[1]] = int(tok[2])
            if tok and tok[0] == 'end_header':
                break
    return counts
