"""GPU tier of the labelling layer: the one compress entry of csrc/pps_labels.hip alone between canary rows against a
numpy walk, its argument rules, and labels.fixed_point on a hand-made pair table.  The hooks are tested with their stages."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
I32 = torch.int32


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def guarded(n, fill=-7):
    """(buffer [n + 2] filled with `fill`, its rows 1 .. n): labels between two canary rows."""
    buf = torch.full((n + 2,), fill, dtype=I32, device=DEV)
    return buf, buf[1:n + 1]


def compressed(label):
    """The specification: every slot with a label >= 0 gets the end of its walk, which steps from x to label[x] while 0 <= label[x] < x."""
    out = label.copy()
    for x in range(label.shape[0]):
        if label[x] >= 0:
            e = x
            while 0 <= label[e] < e:
                e = int(label[e])
            out[x] = e
    return out


def run_compress(start):
    from ppsurf_amd import _lib
    n = start.shape[0]
    buf, label = guarded(n)
    label.copy_(dev(start))
    got = []
    for _ in range(2):                                                  # a second compress changes nothing
        _lib.call('ppsx_labels_compress', label, n)
        got.append(label.cpu().numpy())
        assert buf[0].item() == -7 and buf[-1].item() == -7
    return got


@pytest.mark.parametrize('n', [255, 256, 257])
def test_compress_alone_matches_a_numpy_walk_across_a_block_edge(n):
    start = (np.arange(n) // 2).astype(np.int32)                        # a tree of depth log2 n under slot 0
    start[n - 9] = n - 9                                                # a root, and a chain of depth 8 down to it: at n = 257 it crosses the block edge
    start[n - 8:] = np.arange(n - 9, n - 1)
    start[[50, 120]] = [-1, -(1 << 31)]                                 # negative labels: never touched, and a walk that reaches one ends there
    start[[7, 90, 201]] = [300, (1 << 31) - 1, n]                       # labels above their slots (and above n): the walk ends as at a root
    want = compressed(start)
    assert want[n - 1] == n - 9 and want[50] == -1 and want[120] == -(1 << 31) and want[100] == 50 and want[7] == 7 and want[14] == 7
    assert np.array_equal(compressed(want), want)
    first, second = run_compress(start)
    assert first.tobytes() == want.tobytes() and second.tobytes() == want.tobytes()


def test_compress_alone_on_the_hand_made_chains_of_the_stages():
    # chains, an untouched negative label, and a label above its slot, where a walk ends as at a root (from the pieces and the weld tests)
    for start, want in (([0, 0, 1, 2, -1, 7, 5, 3], [0, 0, 0, 0, -1, 5, 5, 0]), ([0, 0, 1, 2, -1, 9, 5, 4], [0, 0, 0, 0, -1, 5, 5, 4])):
        start = np.array(start, dtype=np.int32)
        assert compressed(start).tolist() == want
        for got in run_compress(start):
            assert got.tolist() == want


def test_bad_arguments_are_an_error_return_and_write_nothing():
    from ppsurf_amd import _lib
    label0 = torch.arange(8, dtype=I32, device=DEV).flip(0).contiguous()          # a compress that ran would change it
    label = label0.clone()

    def run(label, n):
        rc = _lib.call('ppsx_labels_compress', label, n, on=torch.device(DEV), unchecked=True)
        torch.cuda.synchronize()
        return rc

    assert run(label, -1) == 1 and run(label, 2 ** 31) == 1 and run(None, 8) == 1
    assert run(label, 0) == 0 and run(None, 0) == 0 and torch.equal(label, label0)
    with pytest.raises(_lib.PpsError, match='ppsx_labels_compress failed with status 1'):
        _lib.call('ppsx_labels_compress', label, -1)
    _lib.call('ppsx_labels_compress', None, 0, on=torch.device(DEV))
    assert torch.equal(label, label0)


def test_fixed_point_on_the_hand_made_pair_table_of_the_pieces():
    from ppsurf_amd import _lib, labels
    # nf = 8, face 3 invalid; pairs onto it, out of range on either side, and three good ones (test_gpu_pieces.py)
    buf, label = guarded(8)
    label.copy_(dev(np.array([0, 1, 2, -1, 4, 5, 6, 7], dtype=np.int32)))
    fa = dev(np.array([0, 2, 2, 4, -1, 6, 3, 8, 2 ** 31 - 1], dtype=np.int32))
    fb = dev(np.array([1, 1, 3, 9, 5, 5, 7, 0, 0], dtype=np.int32))
    flags = []

    def hook(changed):
        assert changed.dtype == I32 and tuple(changed.shape) == (1,) and changed.item() == 0
        _lib.call('ppsx_pieces_hook', fa, fb, 9, label, 8, changed)
        flags.append(int(changed.item()))

    rounds = labels.fixed_point(hook, lambda: labels.compress(label, 8), torch.device(DEV))
    assert rounds >= 2 and flags == [1] * (rounds - 1) + [0]
    assert label.cpu().numpy().tolist() == [0, 0, 0, -1, 4, 5, 5, 7] and buf[0].item() == -7 and buf[-1].item() == -7
    # a fixed point leaves the flag down at once and writes nothing
    assert labels.fixed_point(hook, lambda: labels.compress(label, 8), torch.device(DEV)) == 1
    assert label.cpu().numpy().tolist() == [0, 0, 0, -1, 4, 5, 5, 7] and buf[0].item() == -7 and buf[-1].item() == -7
