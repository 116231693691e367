"""numpy restatement of the topology layer of the mesh stages (ppsurf_amd/topology.py, ppsurf_amd/csrc/pps_faces.h): the
valid-face rule, the keys of the two key kernels and the row tables made of them.  smooth_spec and normals_spec import these names; nothing
here comes from the device.
"""
import numpy as np

SENTINEL = np.iinfo(np.int64).max


def valid_faces(faces, nv):
    """bool [nf]: the three indices lie in [0, nv) and are pairwise distinct."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    return ((f >= 0) & (f < nv)).all(axis=1) & (a != b) & (b != c) & (c != a)


def half_edge_keys(faces, nv):
    """int64 [6 nf]: (src << 32) | dst of a->b, b->a, b->c, c->b, c->a, a->c per face, in that order; INT64_MAX six times for an invalid face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    keys = np.stack([(a << 32) | b, (b << 32) | a, (b << 32) | c, (c << 32) | b, (c << 32) | a, (a << 32) | c], axis=1)
    keys[~valid_faces(f, nv)] = SENTINEL
    return keys.reshape(-1)


def adjacency(faces, nv):
    """(offsets int64 [nv + 1], nbr int64 [ne], mult int64 [ne]): per vertex the distinct targets of its half-edges in ascending order and how
    often each occurs."""
    keys = half_edge_keys(faces, nv)
    uniq, counts = np.unique(keys[keys != SENTINEL], return_counts=True)
    offsets = np.zeros(nv + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(uniq >> 32, minlength=nv))
    return offsets, uniq & 0xFFFFFFFF, counts.astype(np.int64)


def corner_keys(faces, nv):
    """int64 [3 nf]: (a << 32) | t, (b << 32) | t, (c << 32) | t per face t = (a, b, c), in that order; INT64_MAX three times for an invalid face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    t = np.arange(f.shape[0], dtype=np.int64)
    keys = (f << 32) | t[:, None]
    keys[~valid_faces(f, nv)] = SENTINEL
    return keys.reshape(-1)


def incidence(faces, nv):
    """(offsets int64 [nv + 1], inc int64 [ni]): per vertex the valid faces that hold it, in ascending face index (a duplicated face is two
    faces and sits in the row twice)."""
    keys = corner_keys(faces, nv)
    keys = np.sort(keys[keys != SENTINEL])
    offsets = np.zeros(nv + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(keys >> 32, minlength=nv))
    return offsets, keys & 0xFFFFFFFF
