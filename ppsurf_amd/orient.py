"""Orientation of a mesh on the GPU: one coherent winding per face component, outward where the component is closed
(csrc/pps_orient.hip).

    python -m ppsurf_amd.orient MESH OUT.ply [--mode outward|inward|majority]

Every other mesh stage takes the winding of the faces as it comes: the normals follow it, the denoising drops neighbours across what looks
like a crease, the decimation's fold rule refuses collapses.  This module makes the winding right first.  Two valid faces are adjacent
across an undirected edge that exactly two valid faces hold (the components of pieces.py); a pair that runs its edge in the same direction
twice is incoherent, and within an orientable component that fixes every face's flip relative to the leader, the smallest face index.  A
closed component is then turned so that its signed volume is positive (`outward`) or negative (`inward`); an open one, and every
component in `majority` mode, keeps the winding of its larger half.  A component that cannot be oriented (a Moebius strip, a Klein
bottle) comes back byte for byte and is counted.  The volume is summed in fp64 in a fixed order, so the result is a pure function of
(verts, faces, mode).  The models have no switch for this stage: run the command on the PLY that `pps.py rec` wrote.  Vertices are never
welded here: a soup of unconnected triangles is one component per face and comes back unchanged; run `python -m ppsurf_amd.weld` first.
"""
import json
import sys

import torch

from . import _lib, labels, mesh_cli, meshio, topology
from .topology import CpuTensorError  # noqa: F401  (its home is topology.py; the name stays importable from here)

MAX_COUNT = topology.MAX_COUNT
MODES = ('outward', 'inward', 'majority')
SUM_BLOCK = 256                            # positions per block of the volume sum (SUM_BLOCK of csrc/pps_orient.hip)


def _checked_mode(mode):
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError('mode must be one of {}, got {!r}'.format(', '.join(MODES), mode))
    return mode


def _flips(f, nv):
    """(label int32 [nf], flip uint8 [nf], bad uint8 [nf], valid bool [nf], fa int32 [np], rounds) of contiguous device faces: the pairs
    of the topology layer and their labelling with a parity."""
    fa, fb, ea, eb, valid = topology.manifold_pair_edges(f, nv)
    return _parity_labels(f, fa, fb, ea, eb, valid)


def _parity_labels(f, fa, fb, ea, eb, valid):
    """_flips on a given pair list: the pair signs, hooking and compressing with a parity until a hook launch changes nothing, and the
    check of every pair.  The rounds depend on the face order and on timing; label does not, and flip does not where bad[label] is 0."""
    nf, dev = int(f.shape[0]), f.device
    own = torch.arange(nf, dtype=torch.int64, device=dev)
    word = torch.where(valid, own << 1, torch.full_like(own, -1))
    bad = torch.zeros(nf, dtype=torch.uint8, device=dev)
    pairs, rounds = int(fa.shape[0]), 0
    if pairs > 0:
        sign = torch.empty(pairs, dtype=torch.uint8, device=dev)
        _lib.call('ppsx_orient_pair_sign', f, nf, fa, fb, ea, eb, pairs, sign)
        rounds = labels.fixed_point(lambda changed: _lib.call('ppsx_orient_hook', fa, fb, sign, pairs, word, nf, changed),
                                    lambda: _lib.call('ppsx_orient_compress', word, nf), dev)
        _lib.call('ppsx_orient_check', fa, fb, sign, pairs, word, nf, bad)
    label = torch.where(valid, word >> 1, word).to(torch.int32)
    flip = (word & 1).to(torch.uint8) * valid
    return label, flip, bad, valid, fa, rounds


def _volumes(v, f, flip, cid, leader, need, faces_c):
    """f64 [nc]: six times the signed volume, the flips applied, of the components with `need` set (0 for the others): their faces in
    ascending index, blocks of SUM_BLOCK laid out per component from its start, one wave per block, one thread per component."""
    nv, nf, nc, dev = int(v.shape[0]), int(f.shape[0]), int(leader.shape[0]), f.device
    comp = cid.long()
    rows = torch.nonzero((comp >= 0) & need[comp.clamp(min=0)]).reshape(-1)
    order = torch.sort(comp[rows], stable=True)[1]
    listed = rows[order].to(torch.int32)
    n = torch.where(need, faces_c, torch.zeros_like(faces_c))
    blocks = (n + (SUM_BLOCK - 1)) // SUM_BLOCK
    start = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(blocks, 0)
    nb = int(start[-1].item())
    of = torch.repeat_interleave(torch.arange(nc, dtype=torch.int64, device=dev), blocks)          # the component of every block
    within = torch.arange(nb, dtype=torch.int64, device=dev) - start[:-1][of]
    first = (torch.cumsum(n, 0) - n)[of] + within * SUM_BLOCK
    count = torch.clamp(n[of] - within * SUM_BLOCK, max=SUM_BLOCK).to(torch.int32)
    lead = leader[of].to(torch.int32)
    sums = torch.empty(nb, dtype=torch.float64, device=dev)
    vol = torch.empty(nc, dtype=torch.float64, device=dev)
    _lib.call('ppsx_orient_block_sums', v, nv, f, nf, flip, listed, int(listed.shape[0]), first, count, lead, nb, sums)
    _lib.call('ppsx_orient_comp_sums', sums, nb, start, nc, vol)
    return vol


def _oriented(v, f, mode):
    """(faces or None, info) of a checked device mesh and a checked mode; None when nothing turns."""
    nv, nf = int(v.shape[0]), int(f.shape[0])
    label, flip, bad, valid, fa, _ = _flips(f, nv)
    _, leader, number = labels.leaders(label, live=valid)
    nc = int(leader.shape[0])
    info = {'faces_in': nf, 'faces_valid': int(valid.sum().item()), 'faces_flipped': 0, 'components': nc, 'components_closed': 0,
            'components_open': 0, 'components_non_orientable': 0, 'faces_non_orientable': 0, 'components_flipped': 0, 'zero_volume': 0,
            'mode': mode}
    if nc == 0:
        return None, info
    cid = torch.where(valid, number[label.clamp(min=0).long()], torch.full_like(number, -1)).to(torch.int32)
    live = cid[valid].long()
    faces_c = torch.bincount(live, minlength=nc)
    ones_c = torch.bincount(cid[flip == 1].long(), minlength=nc)                                  # |T|; an invalid face has flip 0
    pairs_c = torch.bincount(cid[fa.long()].long(), minlength=nc)
    broken = bad[leader].bool()
    closed = 2 * pairs_c == 3 * faces_c
    turn = torch.where(2 * ones_c <= faces_c, 1, 2)                                               # the majority: T when it is no larger than U
    zero = torch.zeros_like(closed)
    if mode != 'majority':
        need = closed & ~broken
        if bool(need.any()):
            vol = _volumes(v, f, flip, cid, leader, need, faces_c)
            plus, minus = need & (vol > 0), need & (vol < 0)
            zero = need & ~plus & ~minus
            out_t, out_u = (plus, minus) if mode == 'outward' else (minus, plus)
            turn = torch.where(out_t, 1, torch.where(out_u, 2, turn))
    turn = torch.where(broken, 0, turn).to(torch.uint8)
    turned_c = torch.where(turn == 1, ones_c, torch.where(turn == 2, faces_c - ones_c, torch.zeros_like(ones_c)))
    flipped = int(turned_c.sum().item())
    info.update(faces_flipped=flipped, components_closed=int(closed.sum().item()), components_open=int((~closed).sum().item()),
                components_non_orientable=int(broken.sum().item()), faces_non_orientable=int(faces_c[broken].sum().item()),
                components_flipped=int((turn == 2).sum().item()), zero_volume=int(zero.sum().item()))
    if flipped == 0:
        return None, info
    out = torch.empty_like(f)
    _lib.call('ppsx_orient_apply', f, nf, cid, flip, turn, nc, out)
    return out, info


def face_flips(faces: torch.Tensor, nv: int):
    """(label int32 [nf], flip uint8 [nf], bad uint8 [nf]) on the device for faces int64 [nf,3]: label as pieces.face_components (the
    smallest face index of the component of a valid face, -1 for an invalid one); flip, 1 when the face must turn for its winding to
    agree with its leader's (0 for an invalid face); bad, indexed by leader, 1 when the leader's component is not orientable -- there the
    flips mean nothing."""
    topology.need_device('face_flips', faces)
    assert faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int64
    if not 0 <= int(nv) <= MAX_COUNT or faces.shape[0] > MAX_COUNT:
        raise ValueError('nv and the number of faces must be in 0..2^31 - 1, got {} and {}'.format(nv, faces.shape[0]))
    return _flips(faces.contiguous(), int(nv))[:3]


def orient_mesh(verts: torch.Tensor, faces: torch.Tensor, mode='outward'):
    """(verts, faces, info) of the device mesh verts f32 [nv,3] / faces int64 [nf,3] with one coherent winding per orientable component.
    mode 'majority': of the two halves of a component that disagree the smaller turns, on a tie the half without the leader.  'outward'
    ('inward'): a closed component -- every face lies in three pairs -- is turned so that its signed volume is positive (negative); a
    closed component whose volume is exactly 0 and every open component take the majority.  A component that is not orientable comes back
    byte for byte.  A turned face (a, b, c) becomes (a, c, b); every other row, the invalid ones included, and the vertices come back as
    they are, the faces in their given order; when nothing turns the same tensors come back.  info: faces_in, faces_valid, faces_flipped,
    components, components_closed, components_open, components_non_orientable, faces_non_orientable, components_flipped (the leader
    turned), zero_volume, mode.  ValueError: a mode that is none of the three strings, non-finite vertices, more than 2^31 - 1 vertices
    or faces, CPU tensors (CpuTensorError)."""
    mode = _checked_mode(mode)
    topology.need_device('orient_mesh', verts, faces)
    v, f = topology.checked_mesh('orient_mesh', verts, faces, limit=True)
    out, info = _oriented(v, f, mode)
    return verts, faces if out is None else out, info


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m ppsurf_amd.orient',
                                 description='Orient a mesh: one coherent winding per component, outward where it is closed (GPU).')
    ap.add_argument('mesh', help='PLY or OBJ mesh')
    ap.add_argument('out_file', help='PLY mesh with the faces re-wound')
    ap.add_argument('--mode', choices=MODES, default='outward',
                    help='outward / inward: by the signed volume of every closed component; majority: the larger half of every component stays')
    args = ap.parse_args(argv)
    meshio.need_ply_output(ap, args.out_file)
    mesh = mesh_cli.load(args.mesh, 'python -m ppsurf_amd.orient')
    out, info = _oriented(*mesh.to_device(limit='faces'), args.mode)
    mesh.write_as_read(args.out_file, faces=out)
    print(json.dumps(info))
    return info


if __name__ == '__main__':
    main(sys.argv[1:])
