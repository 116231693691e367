"""The labelling layer of the mesh stages on the host: the hooking and compressing loop, the one compress call and the numbering of the
leaders (csrc/pps_labels.h, where the argument is written out; csrc/pps_labels.hip).

No stage knowledge lives here: pieces.py labels faces, weld.py vertices, manifold.py corners and orient.py faces with a parity; each
builds its start labels, hands its hook (and, for orient, its own compress) to `fixed_point` and reads the leaders off with `leaders`.
"""
import torch

from . import _lib


def fixed_point(hook, compress, device):
    """The rounds of { flag = 0; hook(changed); flag down -> done; compress() }: `changed` is the int32 [1] flag on `device` that the hook
    launch raises, and reading it is the round's one synchronisation.  At least one hook runs; the guards (no pairs, no vertices) are the
    callers'.  The rounds depend on the order of the input and on timing; the labels at the end do not."""
    changed = torch.zeros(1, dtype=torch.int32, device=device)
    rounds = 0
    while True:
        changed.zero_()
        hook(changed)
        rounds += 1
        if int(changed.item()) == 0:
            return rounds
        compress()


def compress(label, n):
    """Every slot of label int32 [n] with a label >= 0 gets the end of its descending walk (ppsx_labels_compress): the step between two
    hooking rounds, on face, vertex and corner labels alike."""
    _lib.call('ppsx_labels_compress', label, n)


def leaders(label, live=None):
    """(leads bool [n], leader int64 [nc] ascending, number int64 [n]) of label int32 [n] at its fixed point: a slot leads when it holds
    its own index (and `live`, a bool mask, when given); number = cumsum(leads) - 1 is the component number at every leader, so that
    number[label] numbers every slot that takes part in ascending leader."""
    leads = label == torch.arange(label.shape[0], dtype=torch.int32, device=label.device)
    if live is not None:
        leads = live & leads
    return leads, torch.nonzero(leads).reshape(-1), torch.cumsum(leads, 0) - 1
