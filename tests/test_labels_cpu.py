"""The host side of the labelling layer without a GPU (ppsurf_amd/labels.py): the loop with stub launches, the numbering of the leaders
against numpy, and where the one compress entry is declared and called."""
import ctypes

import numpy as np
import torch

import call_sites


def test_fixed_point_alternates_hook_and_compress_until_the_flag_stays_down():
    from ppsurf_amd import labels
    calls, raises = [], [True, True, False]

    def hook(changed):
        assert changed.dtype == torch.int32 and tuple(changed.shape) == (1,) and int(changed.item()) == 0          # zeroed before every hook
        if raises[calls.count('hook')]:
            changed.fill_(1)
        calls.append('hook')

    assert labels.fixed_point(hook, lambda: calls.append('compress'), 'cpu') == 3
    assert calls == ['hook', 'compress', 'hook', 'compress', 'hook']
    calls.clear()
    assert labels.fixed_point(lambda changed: calls.append('hook'), lambda: calls.append('compress'), 'cpu') == 1
    assert calls == ['hook']


def _leaders_numpy(label, live=None):
    leads = label == np.arange(label.shape[0])
    if live is not None:
        leads &= live
    return leads, np.nonzero(leads)[0], np.cumsum(leads) - 1


def test_leaders_match_numpy_with_negative_slots_a_live_mask_and_no_slots():
    from ppsurf_amd import labels
    label = np.array([0, 0, -1, 3, 0, 3, -1, 7, 7, 3], dtype=np.int32)
    live = label >= 0
    live[7] = False                                                      # slot 7 holds its own index and is masked out
    for lab, mask in ((label, None), (label, live), (np.zeros(0, dtype=np.int32), None), (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=bool))):
        leads, leader, number = labels.leaders(torch.from_numpy(lab), None if mask is None else torch.from_numpy(mask))
        want = _leaders_numpy(lab, mask)
        assert leads.dtype == torch.bool and leader.dtype == torch.int64 and number.dtype == torch.int64
        for got, ref in zip((leads, leader, number), want):
            assert got.shape == ref.shape and np.array_equal(got.numpy(), ref)
        assert np.all(np.diff(leader.numpy()) > 0)                                                      # ascending
        assert np.array_equal(number.numpy()[leader.numpy()], np.arange(leader.shape[0]))               # consecutive from 0
    assert labels.leaders(torch.from_numpy(label))[1].tolist() == [0, 3, 7]
    assert labels.leaders(torch.from_numpy(label), torch.from_numpy(live))[1].tolist() == [0, 3]


def test_the_one_compress_entry_is_declared_once_and_called_from_labels_py():
    from ppsurf_amd import _lib, build
    I, I64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.EXT_SIGNATURES['ppsx_labels_compress'] == (I, [P, I64, P])
    assert _lib.EXT_PARAMS['ppsx_labels_compress'] == ['label', 'n', 'stream']
    # the stages' own int32 compress entries are gone: orient's works on 64-bit words with a parity
    assert sorted(n for n in _lib.EXT_SIGNATURES if n.endswith('_compress')) == ['ppsx_labels_compress', 'ppsx_orient_compress']
    sites = call_sites.ext_call_sites('ppsx_labels')
    assert {name: [(path, nargs) for path, _, nargs in where] for name, where in sites.items()} == {'ppsx_labels_compress': [('labels.py', 2)]}
    assert not any(n.startswith('pps_labels') or n.startswith('ppsx_') for n in _lib.SIGNATURES)          # the main header stays frozen
    assert 'pps_labels.hip' in build.SOURCES and 'pps_labels.h' in build.HEADERS
    lib = _lib.lib()
    assert lib.pps_abi_version() == 2 and 'ppsx_labels_compress' in _lib._ext_entries
