"""GPU tier of the shared layer of the mesh stages: ops.row_offsets against numpy, the sorted keys of both key kernels
through topology.sorted_keys against tests/topology_spec.py, and adjacency against incidence on one mesh."""
import numpy as np
import pytest
import torch

import smooth_spec
import topology_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NV = 642


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: from_numpy wants a writable array)


@pytest.fixture(scope='module')
def faces():
    """The 1280 faces of the noisy icosphere(3) with every seventh face invalid, one way or another (as test_half_edge_keys_alone)."""
    f = np.array(smooth_spec.noisy_sphere(3)[1])
    f[::7, 1] = -1
    f[3::7, 2] = NV
    f[5::7, 0] = f[5::7, 1]
    f.setflags(write=False)
    return f


def numpy_offsets(ids, n):
    out = np.zeros(n + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(ids, minlength=n))
    return out


@pytest.mark.parametrize('n', [0, 1, 5])
def test_row_offsets_small(n):
    from ppsurf_amd import ops
    cases = [np.zeros(0, dtype=np.int64)]                             # no ids
    if n:
        cases += [np.full(9, n - 1, dtype=np.int64), np.sort(np.random.default_rng(n).integers(0, n, size=33))]          # all in the last row; any
    for ids in cases:
        got = ops.row_offsets(dev(ids), n)
        assert got.dtype == torch.int64 and got.device.type == 'cuda' and tuple(got.shape) == (n + 1,)
        assert np.array_equal(got.cpu().numpy(), numpy_offsets(ids, n))


def test_row_offsets_over_257_rows():
    from ppsurf_amd import ops
    ids = np.sort(np.random.default_rng(257).integers(0, 257, size=5000))
    ids = ids[(ids != 100) & (ids != 256)]                            # an empty row inside and an empty last row
    want = numpy_offsets(ids, 257)
    assert np.array_equal(ops.row_offsets(dev(ids), 257).cpu().numpy(), want) and want[-1] == ids.shape[0] and want[101] == want[100]
    unsorted = np.random.default_rng(1).permutation(ids)              # the offsets are counts: the order of the ids does not matter
    assert np.array_equal(ops.row_offsets(dev(unsorted), 257).cpu().numpy(), want)


@pytest.mark.parametrize('nf', [0, 1, 255, 256, 257])
def test_sorted_keys_of_both_kinds(faces, nf):
    from ppsurf_amd import topology
    f = np.array(faces[:nf]).reshape(-1, 3)
    valid = int(T.valid_faces(f, NV).sum())
    for entry, per_face, spec in (('ppsx_smooth_half_edges', 6, T.half_edge_keys), ('ppsx_normals_corner_keys', 3, T.corner_keys)):
        want = np.sort(spec(f, NV))
        assert want.shape[0] == per_face * nf and int((want == T.SENTINEL).sum()) == per_face * (nf - valid)
        keys, count = topology.sorted_keys(entry, per_face, dev(f), NV)
        assert keys.dtype == torch.int64 and keys.device.type == 'cuda' and count == valid
        assert np.array_equal(keys.cpu().numpy(), want[:per_face * valid])           # the sorted keys without the sentinels at their end


def test_adjacency_and_incidence_tell_one_story(faces):
    from ppsurf_amd import topology
    f = dev(faces)
    a_off, nbr, mult, a_valid = topology.adjacency_rows(f, NV)
    i_off, inc, i_valid = topology.incidence_rows(f, NV)
    assert a_valid == i_valid == int(T.valid_faces(faces, NV).sum()) and 0 < a_valid < faces.shape[0]
    for got, want in zip((a_off, nbr, mult), T.adjacency(faces, NV)):
        assert np.array_equal(got.cpu().numpy(), want)
    for got, want in zip((i_off, inc), T.incidence(faces, NV)):
        assert np.array_equal(got.cpu().numpy(), want)
    assert all(torch.equal(a, b) for a, b in zip(topology.mesh_adjacency(f, NV), (a_off, nbr, mult)))
    assert all(torch.equal(a, b) for a, b in zip(topology.vertex_incidence(f, NV), (i_off, inc)))
    a_off, nbr, i_off, inc = (t.cpu().numpy() for t in (a_off, nbr, i_off, inc))
    for i in range(NV):                                               # j is in row i of the adjacency exactly when a face of row i of the incidence holds j
        held = np.unique(faces[inc[i_off[i]:i_off[i + 1]]])
        assert np.array_equal(nbr[a_off[i]:a_off[i + 1]], held[held != i]), i
