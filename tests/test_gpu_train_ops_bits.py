"""Every autograd op of ppsurf_amd/train_ops.py, bit for bit: SHA-256 of each forward output, of each buffer updated in place (running statistics,
norm radius) and of the gradient of each differentiable input, and the ordered list of C entries that went through _lib.call during forward and
backward, compared with tests/golden/train_ops_bits.json -- recorded on an MI355X from the train_ops.py BEFORE its marshalling was folded into
shared helpers (tests/golden/make_train_ops_bits.py; the fixture's header names the git blob it came from).  The kernels are deterministic (no
floating-point atomics, fixed-order partial sums) and a helper that only marshals arguments changes neither a bit nor a launch: one more cast, a
`zeros` for an `empty`, one more `.contiguous()` or a reordered call shows here.

Inputs come from a seeded CPU torch.Generator (seed = CRC-32 of the case's name) and are moved to the device; no device RNG.  Shapes are the
smallest at which each path can still go wrong:
    rows_layer             (rows, cin, cout, in-affine, bn, bias) = (33, 256, 128, +, +, +), (70, 64, 64, -, +, -), (33, 128, 256, +, -, +), in-ReLU on:
                           32-row tiles (one full + a 1-row tile; two full + a 6-row tile), every width the kernels take, the bn / non-bn returns
    rows_layer_max,        128 -> 256 (the one shape the pooled backward takes), (groups, p) = (3, 50) with ReLU and (5, 7) without: groups straddle
    rows_layer_patch_attn  a tile edge; p = 50 is the workload's
    act_max                (5, 7, 64): an affine with negative scales + ReLU (min / max selection); affine None with and without ReLU
    rows3_layer            257 rows (32-row blocks, partial last one), under autocast (the op takes its storage type from it)
    patch_transform,       (nq, p) = (5, 50), (3, 7): 4 groups per block -> a partial block; patch_transform also with Act(affine=None, relu=True),
    patch_attn             the identity affine patch_transform() synthesises
    head_input, query_attn_pool, head_chain      40 table rows, (nq, k) = (7, 5), (5, 64): 35 rows are a partial 256-row unit, 320 one full + a partial
                           one; the last two under both PPS_ATTN_GRAD values; once with table.requires_grad = False (the needs_input_grad branches)
    gather_rows            fp32 c = 3; bf16 c = 64; bf16 c = 5 (odd width: up-cast); an empty idx; the last source row is never referenced
    neighbour_max          n = 40, m = 13, k = 5, c = 64: fp32 entry and 16-bit entry
    neighbour_contract     (c, k) = (32, 5) 16-bit (matrix-pipe path), (6, 20) fp32; x / g with and without gradient
    fka_geometry           b = 2, m = 13, k = 5; momentum 0.1 / 0; owned on / off (radius moved in place in the caller's vector or in a copy)
    bn_act, bn_add_relu    (33, 64), (70, 256); fp32, bf16, fp16 (dtype codes 0, 1, 2); bn_act with and without ReLU
    attn_pool              qy [7, 5, 64], h [7, 5, 256], relu_h on / off
    col_sum / sum_rows     (33, 64); the column block [:, 64:128] of [33, 256] (summed where it lies); c = 6 (padded to 4 columns' multiple), c = 10
                           (padded twice: to 12, which the thread layout does not divide, then to 16); c = 1028 (split at 1024)
    gemm_nt, gemm_tn       M = 33, K = 64, N = 72; each operand once as a column slice at an odd offset (address not a multiple of 16: the
                           .contiguous() repair); bias, out_f32
16-bit cases run in bfloat16 and IEEE half.

The result of gathering zero rows is empty and its gradient is zero by definition: those two digests are the only ones allowed to be the digest
of zeros (ZERO_BY_DEFINITION), and the CPU test holds them to it."""
import hashlib
import json
import os
import zlib

import pytest
import torch

from ppsurf_amd import train_ops

DEV = 'cuda:0'
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_ops_bits.json')
PARENT_BLOB = '1a06c4dd85327288d10ff657d99ae5f65a6af9bd'        # git blob of the train_ops.py the fixture was recorded from
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
LOW = (BF16, F16)
TAG = {F32: 'f32', BF16: 'bf16', F16: 'f16'}
ZERO_BY_DEFINITION = {('gather_rows-empty', 'out:out'), ('gather_rows-empty', 'grad:x')}


def _t(g, *shape, scale=1.0, shift=0.0, dt=F32, grad=False):
    """seeded normal values, made on the CPU, rounded to dt, moved to the device"""
    t = (torch.randn(*shape, generator=g) * scale + shift).to(dt).to(DEV)
    return t.requires_grad_(True) if grad else t


def _leaf(g, *shape, **kw):
    return _t(g, *shape, grad=True, **kw)


def _pair(g, c, scale0=0.3, shift0=1.0):
    """[2, c] (scale, shift) of a stored activation; scale0 = 1, shift0 = 0 gives scales of both signs"""
    return torch.stack([torch.randn(c, generator=g) * scale0 + shift0, torch.randn(c, generator=g) * 0.4]).to(DEV).requires_grad_(True)


def _ids(g, n, *shape):
    """row numbers below n - 1: the last row is never referenced"""
    return torch.randint(0, n - 1, shape, generator=g).to(DEV)


class _Bn:
    """what the ops read of a BatchNorm1d: affine parameters (leaves), running statistics (updated in place), momentum, eps"""

    def __init__(self, g, c, signed=False):
        self.weight = _leaf(g, c, scale=1.0 if signed else 0.2, shift=0.0 if signed else 1.0)
        self.bias = _leaf(g, c, scale=0.3)
        self.running_mean, self.running_var = _t(g, c, scale=0.1), (torch.rand(c, generator=g) + 0.5).to(DEV)
        self.momentum, self.eps = 0.1, 1e-5

    def leaves(self):
        return {'gamma': self.weight, 'beta': self.bias}

    def buffers(self):
        return {'running_mean': self.running_mean, 'running_var': self.running_var}


def _finish(g, outs, leaves, buffers=None):
    """-> {'out:..', 'buf:..', 'grad:..': tensor}: one backward pass with seeded gradients of every differentiable output towards every leaf"""
    outs = {k: v for k, v in outs.items() if v is not None}
    res = {'out:' + k: v.detach() for k, v in outs.items()}
    diff = [v for v in outs.values() if v.requires_grad]
    want = {k: v for k, v in leaves.items() if v is not None and v.requires_grad}
    if want:
        gos = [torch.randn(*v.shape, generator=g).to(v.dtype).to(DEV) for v in diff]
        grads = torch.autograd.grad(diff, list(want.values()), gos)
        res.update({'grad:' + k: gr for k, gr in zip(want, grads)})
    res.update({'buf:' + k: v.detach() for k, v in (buffers or {}).items()})
    return res


# ---------------------------------------------------------------------------------------------------------------- the ops

def _rows_layer(g, dt, rows, cin, cout, affine, bn, bias):
    x = _leaf(g, rows, cin, scale=1.5, shift=0.3, dt=dt)
    aff = _pair(g, cin) if affine else None
    w, b = _leaf(g, cout, cin, scale=cin ** -0.5), (_leaf(g, cout, scale=0.2) if bias else None)
    hold = _Bn(g, cout) if bn else None
    out = train_ops.rows_layer(train_ops.Act(x, aff, True), w, b, hold, relu=True)
    return _finish(g, {'raw': out.raw, 'affine': out.affine}, dict({'x': x, 'in_affine': aff, 'w': w, 'b': b}, **(hold.leaves() if bn else {})),
                   hold.buffers() if bn else None)


def _pooled_inputs(g, dt, groups, p):
    x = _leaf(g, groups * p, 128, scale=0.7, dt=dt)
    aff = _pair(g, 128)
    w, b = _leaf(g, 256, 128, scale=0.1), _leaf(g, 256, scale=0.1)
    return x, aff, w, b, _Bn(g, 256, signed=True)                # negative scales: the minimum wins there


def _rows_layer_max(g, dt, groups, p, relu):
    x, aff, w, b, hold = _pooled_inputs(g, dt, groups, p)
    assert train_ops.rows_layer_max_supported(groups * p, 128, 256, groups, p)
    out = train_ops.rows_layer_max(train_ops.Act(x, aff, True), w, b, hold, relu, groups, p)
    return _finish(g, {'out': out}, dict({'x': x, 'in_affine': aff, 'w': w, 'b': b}, **hold.leaves()), hold.buffers())


def _rows_layer_patch_attn(g, dt, groups, p, relu):
    x, aff, w, b, hold = _pooled_inputs(g, dt, groups, p)
    wq = _leaf(g, 1, 256, scale=0.2)
    assert train_ops.rows_layer_patch_attn_supported(128, 256, p, groups * p)
    pooled, out_affine = train_ops.rows_layer_patch_attn(train_ops.Act(x, aff, relu), w, b, hold, wq, groups, p)
    return _finish(g, {'pooled': pooled, 'affine': out_affine}, dict({'x': x, 'in_affine': aff, 'w': w, 'b': b, 'wq': wq}, **hold.leaves()),
                   hold.buffers())


def _act_max(g, dt, affine, relu):
    groups, p, c = 5, 7, 64
    raw = _leaf(g, groups * p, c, dt=dt)
    aff = _pair(g, c, scale0=1.0, shift0=0.0) if affine else None
    return _finish(g, {'out': train_ops.act_max(train_ops.Act(raw, aff, relu), groups, p)}, {'raw': raw, 'affine': aff})


def _rows3_layer(g, dt):
    x = _t(g, 257, 3, scale=0.5)
    w, b, hold = _leaf(g, 64, 3), _leaf(g, 64, scale=0.1), _Bn(g, 64)
    with torch.autocast('cuda', dtype=dt):
        out = train_ops.rows3_layer(x, w, b, hold, True)
    assert out.raw.dtype == dt
    return _finish(g, {'raw': out.raw, 'affine': out.affine}, dict({'w': w, 'b': b}, **hold.leaves()), hold.buffers())


def _patch_transform(g, dt, nq, p, affine):
    x = _leaf(g, nq * p, 64, dt=dt)
    t = _leaf(g, nq, 64, 64, scale=0.3, dt=dt)
    aff = _pair(g, 64) if affine else None
    assert train_ops.patch_transform_supported(p, 64)
    return _finish(g, {'out': train_ops.patch_transform(train_ops.Act(x, aff, True), t, p)}, {'x': x, 'affine': aff, 't': t})


def _patch_attn(g, dt, nq, p):
    h, v = _leaf(g, nq, p, 256, dt=dt), _leaf(g, 256, scale=0.2)
    return _finish(g, {'pooled': train_ops.patch_attn(h, v)}, {'h': h, 'v': v})


def _head_inputs(g, dt, nq, k, table_grad):
    n = 40
    table = _t(g, n, 256, dt=dt, grad=table_grad)
    ids = _ids(g, n, nq * k)
    pts, query = (torch.rand(n, 3, generator=g) - 0.5).to(DEV), (torch.rand(nq, 3, generator=g) - 0.5).to(DEV)
    return table, ids, pts, query, _leaf(g, 256, 3, scale=0.5)


def _head_input(g, dt, nq, k, table_grad=True):
    table, ids, pts, query, wx = _head_inputs(g, dt, nq, k, table_grad)
    assert train_ops.head_input_supported(256)
    return _finish(g, {'h1': train_ops.head_input(table, ids, pts, query, k, wx)}, {'table': table, 'wx': wx})


def _query_attn_pool(g, dt, nq, k):
    y3 = _leaf(g, nq * k, 256, dt=dt)
    wq, bq = _leaf(g, 64, 256, scale=1 / 8), _leaf(g, 64, scale=0.1)
    return _finish(g, {'pooled': train_ops.query_attn_pool(y3, wq, bq, k)}, {'y3': y3, 'wq': wq, 'bq': bq})


def _head_chain(g, dt, nq, k, table_grad=True):
    table, ids, pts, query, wx = _head_inputs(g, dt, nq, k, table_grad)
    w2, w3, wq = _leaf(g, 256, 256, scale=1 / 16), _leaf(g, 256, 256, scale=1 / 16), _leaf(g, 64, 256, scale=1 / 8)
    b2, b3, bq = _leaf(g, 256, scale=0.1), _leaf(g, 256, scale=0.1), _leaf(g, 64, scale=0.1)
    assert train_ops.head_chain_supported(256, 64, k)
    out = train_ops.head_chain(table, ids, pts, query, k, wx, (w2, b2), (w3, b3), (wq, bq))
    return _finish(g, {'pooled': out}, {'table': table, 'wx': wx, 'w2': w2, 'b2': b2, 'w3': w3, 'b3': b3, 'wq': wq, 'bq': bq})


def _gather_rows(g, dt, c, r):
    n = 40
    x = _leaf(g, n, c, dt=dt)
    idx = _ids(g, n, r)
    return _finish(g, {'out': train_ops.gather_rows(x, idx)}, {'x': x})


def _neighbour_max(g, dt):
    n, m, k, c = 40, 13, 5, 64
    x = _leaf(g, n, c, dt=dt)
    return _finish(g, {'out': train_ops.neighbour_max(x, _ids(g, n, m, k))}, {'x': x})


def _neighbour_contract(g, dt, c, k, x_grad, g_grad):
    n, m = 40, 13
    x = _t(g, n, c, dt=dt, grad=x_grad)
    geo = _t(g, m, k, 16, grad=g_grad)
    return _finish(g, {'out': train_ops.neighbour_contract(x, _ids(g, n, m, k), geo)}, {'x': x, 'g': geo})


def _fka_geometry(g, momentum, owned):
    b, n, m, k = 2, 40, 13, 5
    pts = (torch.rand(b * n, 3, generator=g) - 0.5).to(DEV)
    sup = pts[torch.cat([torch.randperm(n, generator=g)[:m] + i * n for i in range(b)]).to(DEV)].contiguous()
    idx = torch.stack([torch.randperm(n, generator=g)[:k] + (row // m) * n for row in range(b * m)]).to(DEV)
    r = lambda count, scale=1.0, shift=0.0: torch.randn(count, generator=g) * scale + shift
    geo = torch.cat([torch.tensor([0.2, 1.3, 0.7, 2.0 if momentum else 1.0]), r(48, 0.5), r(512, 1 / 6), r(512, 1 / 6), r(16, 0.2, 1.0), r(16, 0.2),
                     r(16, 0.2, 1.0), r(16, 0.2)]).to(DEV).requires_grad_(True)
    assert geo.numel() == train_ops.GEO_FLOATS
    out, radius = train_ops.fka_geometry(geo, pts, sup, idx, b, m, momentum, owned)
    return _finish(g, {'g': out, 'radius': radius}, {'geo': geo}, {'geo': geo})        # owned: entry 0 of the caller's vector has moved


def _bn_inputs(g, dt, rows, c):
    x = _leaf(g, rows, c, scale=1.5, shift=0.5, dt=dt)
    hold = _Bn(g, c)
    return x, hold


def _bn_act(g, dt, rows, c, relu):
    x, h = _bn_inputs(g, dt, rows, c)
    assert train_ops.bn_supported(rows, c)
    out = train_ops.bn_act(x, h.weight, h.bias, h.running_mean, h.running_var, h.momentum, h.eps, relu)
    return _finish(g, {'y': out}, dict({'x': x}, **h.leaves()), h.buffers())


def _bn_add_relu(g, dt, rows, c):
    x, h = _bn_inputs(g, dt, rows, c)
    res = _leaf(g, rows, c, dt=dt)
    out = train_ops.bn_add_relu(x, res, h.weight, h.bias, h.running_mean, h.running_var, h.momentum, h.eps)
    return _finish(g, {'y': out}, dict({'x': x, 'res': res}, **h.leaves()), h.buffers())


def _attn_pool(g, dt, relu_h):
    qy, h = _leaf(g, 7, 5, 64, scale=3.0, dt=dt), _leaf(g, 7, 5, 256, dt=dt)
    assert train_ops.attn_pool_supported(5, 64, 256)
    return _finish(g, {'pooled': train_ops.attn_pool(qy, h, relu_h)}, {'qy': qy, 'h': h})


def _sums(g, dt, c, block):
    x = _t(g, 33, 256, dt=dt)[:, 64:128] if block else _t(g, 33, c, dt=dt)
    return _finish(g, {'col_sum': train_ops.col_sum(x), 'sum_rows': train_ops.sum_rows(x)}, {})


def _sliced(g, dt, rows, cols, scale=1.0):
    """[rows, cols] at column 3 of a [rows, cols + 16] tensor: unit column stride, a row stride that is a multiple of 8, an address that is
    no multiple of 16"""
    t = _t(g, rows, cols + 16, scale=scale, dt=dt)[:, 3:3 + cols]
    assert t.stride(0) % 8 == 0 and t.data_ptr() % 16
    return t


def _gemm_nt(g, dt, slice_of, bias, out_f32):
    m, k, n = 33, 64, 72
    assert train_ops.gemm_supported(torch.empty(0, device=DEV, dtype=dt), k)
    x = _sliced(g, dt, m, k) if slice_of == 'x' else _t(g, m, k, dt=dt)
    w = _sliced(g, dt, n, k, scale=1 / 8) if slice_of == 'w' else _t(g, n, k, scale=1 / 8, dt=dt)
    return _finish(g, {'y': train_ops.gemm_nt(x, w, _t(g, n) if bias else None, out_f32=out_f32)}, {})


def _gemm_tn(g, dt, slice_of):
    m, k, n = 33, 64, 72
    gr = _sliced(g, dt, m, n, scale=0.1) if slice_of == 'g' else _t(g, m, n, scale=0.1, dt=dt)
    x = _sliced(g, dt, m, k) if slice_of == 'x' else _t(g, m, k, dt=dt)
    return _finish(g, {'dw': train_ops.gemm_tn(gr, x)}, {})


# ---------------------------------------------------------------------------------------------------------------- the cases

CASES = {}          # name -> (function, positional arguments after the generator, environment)


def _add(name, fn, *args, env=None):
    assert name not in CASES
    CASES[name] = (fn, args, env or {})


def _yn(flag, word):
    return word if flag else 'no' + word


for _dt in LOW:
    _s = TAG[_dt]
    for _shape in ((33, 256, 128, True, True, True), (70, 64, 64, False, True, False), (33, 128, 256, True, False, True)):
        _add('rows_layer-{}-{}x{}x{}-{}-{}-{}'.format(_s, *_shape[:3], _yn(_shape[3], 'affine'), _yn(_shape[4], 'bn'), _yn(_shape[5], 'bias')),
             _rows_layer, _dt, *_shape)
    for _groups, _p, _relu in ((3, 50, True), (5, 7, False)):
        _add('rows_layer_max-{}-{}x{}-{}'.format(_s, _groups, _p, _yn(_relu, 'relu')), _rows_layer_max, _dt, _groups, _p, _relu)
        _add('rows_layer_patch_attn-{}-{}x{}-{}'.format(_s, _groups, _p, _yn(_relu, 'relu')), _rows_layer_patch_attn, _dt, _groups, _p, _relu)
    for _affine, _relu in ((True, True), (False, False), (False, True)):
        _add('act_max-{}-{}-{}'.format(_s, _yn(_affine, 'affine'), _yn(_relu, 'relu')), _act_max, _dt, _affine, _relu)
    _add('rows3_layer-{}-257'.format(_s), _rows3_layer, _dt)
    for _nq, _p, _affine in ((5, 50, True), (3, 7, True), (5, 50, False)):
        _add('patch_transform-{}-{}x{}-{}'.format(_s, _nq, _p, _yn(_affine, 'affine')), _patch_transform, _dt, _nq, _p, _affine)
    for _nq, _p in ((5, 50), (3, 7)):
        _add('patch_attn-{}-{}x{}'.format(_s, _nq, _p), _patch_attn, _dt, _nq, _p)
    for _nq, _k in ((7, 5), (5, 64)):
        _add('head_input-{}-{}x{}'.format(_s, _nq, _k), _head_input, _dt, _nq, _k)
        for _mode in ('rebuilt', 'stored'):
            _add('query_attn_pool-{}-{}x{}-{}'.format(_s, _nq, _k, _mode), _query_attn_pool, _dt, _nq, _k, env={'PPS_ATTN_GRAD': _mode})
            _add('head_chain-{}-{}x{}-{}'.format(_s, _nq, _k, _mode), _head_chain, _dt, _nq, _k, env={'PPS_ATTN_GRAD': _mode})
    _add('head_input-{}-7x5-table_without_grad'.format(_s), _head_input, _dt, 7, 5, False)
    _add('head_chain-{}-7x5-rebuilt-table_without_grad'.format(_s), _head_chain, _dt, 7, 5, False, env={'PPS_ATTN_GRAD': 'rebuilt'})
    _add('neighbour_contract-{}-c32-k5'.format(_s), _neighbour_contract, _dt, 32, 5, True, True)
    _add('neighbour_contract-{}-c32-k5-g_without_grad'.format(_s), _neighbour_contract, _dt, 32, 5, True, False)
    for _slice in ('none', 'x', 'w'):
        _add('gemm_nt-{}-slice_{}'.format(_s, _slice), _gemm_nt, _dt, _slice, _slice != 'none', _slice == 'x')
    for _slice in ('none', 'g', 'x'):
        _add('gemm_tn-{}-slice_{}'.format(_s, _slice), _gemm_tn, _dt, _slice)
for _dt in (F32, BF16, F16):
    _s = TAG[_dt]
    _add('neighbour_max-{}'.format(_s), _neighbour_max, _dt)
    for _rows, _c in ((33, 64), (70, 256)):
        for _relu in (True, False):
            _add('bn_act-{}-{}x{}-{}'.format(_s, _rows, _c, _yn(_relu, 'relu')), _bn_act, _dt, _rows, _c, _relu)
        _add('bn_add_relu-{}-{}x{}'.format(_s, _rows, _c), _bn_add_relu, _dt, _rows, _c)
    for _relu in (True, False):
        _add('attn_pool-{}-{}'.format(_s, _yn(_relu, 'relu_h')), _attn_pool, _dt, _relu)
for _dt in (F32, BF16):
    _s = TAG[_dt]
    for _c in (64, 6, 10, 1028):
        _add('sums-{}-33x{}'.format(_s, _c), _sums, _dt, _c, False)
    _add('sums-{}-33x64-column_block'.format(_s), _sums, _dt, 64, True)
_add('gather_rows-f32-c3', _gather_rows, F32, 3, 17)
_add('gather_rows-bf16-c64', _gather_rows, BF16, 64, 17)
_add('gather_rows-bf16-c5', _gather_rows, BF16, 5, 17)
_add('gather_rows-empty', _gather_rows, F32, 3, 0)
_add('neighbour_contract-f32-c6-k20', _neighbour_contract, F32, 6, 20, True, True)
_add('neighbour_contract-f32-c6-k20-x_without_grad', _neighbour_contract, F32, 6, 20, False, True)
for _momentum in (0.1, 0.0):
    for _owned in (False, True):
        _add('fka_geometry-momentum{}-{}'.format(_momentum, _yn(_owned, 'owned')), _fka_geometry, _momentum, _owned)
# no case may be left out of the rows-layer family (tests/golden/make_train_ops_bits.py refuses)
ROWS_FAMILY = ('rows_layer', 'rows_layer_max', 'rows_layer_patch_attn', 'rows3_layer', 'act_max', 'patch_transform', 'patch_attn', 'head_input', 'query_attn_pool', 'head_chain')


# ---------------------------------------------------------------------------------------------------------------- running and comparing

def digest(t):
    """what the fixture keeps of a tensor: SHA-256 of its contiguous bytes, dtype, shape"""
    t = t.detach().contiguous().cpu()
    return {'sha256': hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest(), 'dtype': str(t.dtype).replace('torch.', ''),
            'shape': list(t.shape)}


def zero_digest(entry):
    dt = getattr(torch, entry['dtype'])
    count = 1
    for s in entry['shape']:
        count *= s
    return hashlib.sha256(bytes(count * torch.empty(0, dtype=dt).element_size())).hexdigest()


def run(name, setattr_, setenv):
    """-> {'launches': [entry names in call order], 'tensors': {key: digest}} of case `name`; setattr_ / setenv: monkeypatch's in the test, the
    plain ones in the recorder (which puts _lib.call back itself)"""
    fn, args, env = CASES[name]
    launches = []
    real = train_ops._lib.call

    def spy(entry, *a, **kw):
        launches.append(entry)
        return real(entry, *a, **kw)

    for key, value in env.items():
        setenv(key, value)
    train_ops.clear_cache()                        # a cached CSR of an earlier case would drop pps_csr_build from this one's sequence
    setattr_(train_ops._lib, 'call', spy)
    try:
        tensors = fn(torch.Generator().manual_seed(zlib.crc32(name.encode())), *args)
        torch.cuda.synchronize()
    finally:
        setattr_(train_ops._lib, 'call', real)
        train_ops.clear_cache()
    return {'launches': launches, 'tensors': {k: digest(v) for k, v in tensors.items()}}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def recorded_cases():
    """the cases the fixture has a record of: all but those its `left_out` names (run-to-run differences on the parent, found by the recorder)"""
    left_out = load_fixture()['left_out'] if os.path.isfile(FIXTURE) else {}
    return sorted(n for n in CASES if n not in left_out)


def test_fixture_lists_every_case_with_well_formed_entries():
    """no GPU: recorded from the parent's train_ops.py; every case is there or left out by name with a reason (at most two, none of the rows-layer
    family); each entry has launches and digests, and no digest is that of a zero tensor of its shape (but the two that are zero by definition)"""
    fx = load_fixture()
    assert fx['header']['train_ops_blob'] == PARENT_BLOB
    left_out = fx['left_out']
    assert len(left_out) <= 2 and all(isinstance(r, str) and r for r in left_out.values())
    assert not [n for n in left_out if n.split('-')[0] in ROWS_FAMILY]
    assert set(left_out) <= set(CASES) and sorted(fx['cases']) == sorted(set(CASES) - set(left_out))
    for name, case in fx['cases'].items():
        assert case['launches'] and all(isinstance(e, str) and e.startswith('pps_') for e in case['launches']), name
        assert any(k.startswith('out:') for k in case['tensors']), name
        for key, entry in case['tensors'].items():
            assert key.split(':')[0] in ('out', 'buf', 'grad') and sorted(entry) == ['dtype', 'sha256', 'shape'], (name, key)
            assert len(entry['sha256']) == 64 and int(entry['sha256'], 16) >= 0 and isinstance(getattr(torch, entry['dtype']), torch.dtype), (name, key)
            assert (entry['sha256'] == zero_digest(entry)) == ((name, key) in ZERO_BY_DEFINITION), (name, key)


def test_dtype_code_is_total():
    """no GPU: fp32 has a code of its own (0, the fp32 kernels) instead of falling into the IEEE-half branch; anything else is refused"""
    assert (train_ops._code(F32), train_ops._code(BF16), train_ops._code(F16)) == (0, 1, 2)
    for dt in (torch.int32, torch.float64, torch.uint8):
        with pytest.raises(ValueError):
            train_ops._code(dt)


@pytest.mark.gpu
@pytest.mark.parametrize('name', recorded_cases())
def test_bits_and_launches_are_the_parents(name, monkeypatch):
    want = load_fixture()['cases'][name]
    got = run(name, monkeypatch.setattr, monkeypatch.setenv)
    assert got['launches'] == want['launches'], (name, got['launches'], want['launches'])
    assert sorted(got['tensors']) == sorted(want['tensors']), name
    for key in want['tensors']:
        assert got['tensors'][key] == want['tensors'][key], (name, key, got['tensors'][key], want['tensors'][key])
