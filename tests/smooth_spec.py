"""numpy restatement of the Taubin lambda|mu smoothing (ppsurf_amd/csrc/pps_smooth.hip, ppsurf_amd/smooth.py): the
specification the GPU is held to, bit for bit.  Every step is one float64 numpy operation in the order the kernel uses; nothing here comes
from the device.

Rule: a face is valid when its three indices lie in [0, nv) and are pairwise distinct; a valid face (a, b, c) contributes the half-edges
a->b, b->a, b->c, c->b, c->a, a->c; the multiplicity of i->j is the number of times it occurs.  An edge of multiplicity 1 is a border edge, a
vertex with a border half-edge a border vertex.  An interior vertex takes every distinct j with a half-edge i->j, a border vertex only those
over a border edge.  pass(s): acc = 0.0, acc = acc + x_j in ascending j, m = acc / |N|, x_i' = x_i + s (m - x_i), all from the old positions;
an iteration is pass(lam) then pass(mu); the state is float64 and is rounded to float32 once at the end.
"""
import numpy as np

from topology_spec import SENTINEL, adjacency, half_edge_keys, valid_faces  # noqa: F401  (the rows of section 16 are restated in topology_spec)

D = np.float64


def neighbours(faces, nv):
    """(offsets, nbr, border bool [nv]): the rows of `adjacency` after the border rule -- a vertex with an entry of multiplicity 1 keeps only
    its entries of multiplicity 1."""
    offsets, nbr, mult = adjacency(faces, nv)
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(offsets))
    border = np.zeros(nv, dtype=bool)
    border[src[mult == 1]] = True
    keep = ~border[src] | (mult == 1)
    out = np.zeros(nv + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(src[keep], minlength=nv))
    return out, nbr[keep], border


def one_pass(x, offsets, nbr, s):
    """One Jacobi pass with factor s over x float64 [nv,3].  The sum of a row runs in row order, one float64 addition per neighbour: turn k
    adds the k-th neighbour of every row that has one."""
    deg = np.diff(offsets)
    acc = np.zeros_like(x)
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.nonzero(deg > k)[0]
        acc[rows] = acc[rows] + x[nbr[offsets[rows] + k]]
    out = x.copy()
    rows = np.nonzero(deg > 0)[0]
    m = acc[rows] / deg[rows].astype(D)[:, None]
    out[rows] = x[rows] + D(s) * (m - x[rows])
    return out


def smooth_spec(verts, faces, iters, lam=0.5, mu=-0.53):
    """float32 [nv,3]: `iters` iterations of pass(lam), pass(mu) on the widened float32 vertices, rounded to float32 once at the end."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    offsets, nbr, _ = neighbours(faces, v.shape[0])
    x = v.astype(D)
    for _ in range(int(iters)):
        x = one_pass(x, offsets, nbr, lam)
        x = one_pass(x, offsets, nbr, mu)
    return x.astype(np.float32)


def info_spec(verts, faces, iters, lam=0.5, mu=-0.53):
    """The `info` of smooth.smooth_mesh."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    out = smooth_spec(v, faces, iters, lam, mu)
    return {'vertices': int(v.shape[0]), 'faces_valid': int(valid_faces(faces, v.shape[0]).sum()),
            'border_vertices': int(neighbours(faces, v.shape[0])[2].sum()),
            'moved_vertices': int((out.view(np.int32) != v.view(np.int32)).any(axis=1).sum()), 'iters': int(iters), 'lam': float(lam), 'mu': float(mu)}


def noisy_sphere(subdiv=3):
    """(verts f32 [nv,3], faces int64 [nf,3]): eval_spec.icosphere(subdiv) with the radial noise 1 + 0.02 N(0,1) of default_rng(0)."""
    import eval_spec
    verts, faces = eval_spec.icosphere(subdiv)
    rng = np.random.default_rng(0)
    verts = (verts * (1.0 + 0.02 * rng.standard_normal(verts.shape[0]))[:, None]).astype(np.float32)
    return verts, faces


def fan(n=300, closed=False):
    """(verts f32 [n + 1,3], faces int64): a hub (vertex 0, lifted off the plane) and a ring of n vertices with noisy radii.  Open: the n
    hub triangles.  Closed: a second hub below (vertex n + 1) closes the surface, so nothing is a border."""
    rng = np.random.default_rng(7)
    t = 2.0 * np.pi * np.arange(n) / n
    rad = 1.0 + 0.05 * rng.standard_normal(n)
    ring = np.stack([rad * np.cos(t), rad * np.sin(t), 0.02 * rng.standard_normal(n)], axis=1)
    i = np.arange(n, dtype=np.int64)
    top = np.stack([np.zeros(n, dtype=np.int64), 1 + i, 1 + (i + 1) % n], axis=1)
    if not closed:
        return np.concatenate([[[0.01, -0.02, 0.3]], ring]).astype(np.float32), top
    bottom = np.stack([np.full(n, n + 1, dtype=np.int64), 1 + (i + 1) % n, 1 + i], axis=1)
    return np.concatenate([[[0.01, -0.02, 0.3]], ring, [[0.0, 0.03, -0.4]]]).astype(np.float32), np.concatenate([top, bottom])
