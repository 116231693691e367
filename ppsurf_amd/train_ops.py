"""Autograd ops of the training step backed by the HIP kernels of csrc/pps_train.hip (forward AND backward hand-written).

    gather_rows(x [n,c], idx [r])                     -> [r,c]          (latent gather, nearest up-sampling)
    neighbour_max(x [n,c], idx [m,k])                 -> [m,c]          (nn.py:677-680 max_pool)
    neighbour_contract(x [n,c], idx [m,k], g [m,k,16])-> [m, c*16]      (nn.py:598,647-649 FKAConv feature aggregation)
    fka_geometry(geo [1140], pts, sup, idx, b, m, momentum) -> (g [b*m,k,16], norm_radius')   (nn.py:601-643, pps_fka_train.hip)
    bn_act(x [rows,c], weight, bias, running_mean, running_var, momentum, eps, relu) -> [rows,c]   (train-mode BatchNorm1d + ReLU)
    attn_pool(qy [Q,k,H], h [Q,k,C], relu_h) / query_attn_pool(y3, wq, bq, k)          (attention pooling of the interpolation head)
  bf16 row layers on STORED activations (Act = raw tensor + per-channel (scale, shift) + relu flag, applied by the consumer on load;
  pps_rows_train.hip):
    rows_layer(act, w, b, bn, relu) -> Act        rows3_layer(x [rows,3], w, b, bn) -> Act        act_max(act, groups, p) -> [groups, C]
    patch_transform(act, t_raw [Q,64,64], p)      patch_attn(h [Q,k,256], v [256])               head_input(table, ids, pts, query, k, wx)

Device tensors only: there is no CPU implementation in the product (tests/train_ref_ops.py holds the torch twins the CPU
suite patches in to check the surrounding graph).  Backward scatter-adds are atomics-free and bit-reproducible: the id table
is sorted once (`csr`, cached per table and step) and each target row sums its contributions in a fixed order.
All ops compute in fp32; gather_rows, neighbour_contract (matrix-pipe shapes), bn_act and the attention ops read and write 16-bit activations as they
are, the others up-cast them.
"""
import os

import torch

from . import _lib
from .ops import csr_build, csr_build_table           # csr() below calls csr_build through this module's name


LOW = (torch.bfloat16, torch.float16)          # 16-bit storage types of the fused training ops (trainer.precision bf16-mixed / 16-mixed)


_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _code(dt):
    """dtype argument of the C entries: 0 float32, 1 bfloat16, 2 IEEE half; no other type reaches a kernel."""
    if dt not in _CODES:
        raise ValueError('train_ops: no kernel reads {}'.format(dt))
    return _CODES[dt]


def _f32(t):
    """t as the fp32 contiguous constant the kernels read (weights, affine pairs, points); None stays None."""
    return None if t is None else t.detach().float().contiguous()


def _empty32(dev, *shape):
    return torch.empty(shape, device=dev, dtype=torch.float32)


def _ws(nbytes, dev, floor=0):
    """Scratch of one call, sized by the library's *_ws_bytes (floor: where the entry wants a valid address even for a shape that needs none)."""
    return torch.empty((max(int(nbytes), floor),), device=dev, dtype=torch.uint8)


def _low(t, like=None):
    """t in a 16-bit storage type: as it is if it has one, else the type of `like` / the autocast type / bfloat16."""
    if t.dtype in LOW:
        return t.contiguous()
    if like is not None and like.dtype in LOW:
        return t.to(like.dtype).contiguous()
    dt = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else torch.bfloat16
    return t.to(dt if dt in LOW else torch.bfloat16).contiguous()


def _row1(affine, c):
    """Address of the second row of an fp32 pair [2, c] (the shift of a stored activation's affine part); None stays None."""
    return None if affine is None else affine.data_ptr() + 4 * c


_csr_cache = {}


def csr(idx_flat: torch.Tensor, n: int):
    """(order, offsets) of a flat id table: entries stably sorted by target row, offsets int64 [n+1].  Cached per table."""
    key = (idx_flat.data_ptr(), idx_flat._version, idx_flat.numel(), n)
    hit = _csr_cache.get(key)                       # the cached entry keeps the table alive, so the address cannot be reused
    if hit is not None:
        return hit[1], hit[2]
    order, offsets = csr_build(idx_flat, n)
    if len(_csr_cache) > 64:
        _csr_cache.clear()
    _csr_cache[key] = (idx_flat, order, offsets)
    return order, offsets


def csr_register(idx_flat, n, order, offsets):
    """Enter a CSR built elsewhere (with the batch, train_graph.table_extras) so that the backward pass finds it."""
    _csr_cache[(idx_flat.data_ptr(), idx_flat._version, idx_flat.numel(), n)] = (idx_flat, order, offsets)


def clear_cache():
    _csr_cache.clear()


class _GatherRows(torch.autograd.Function):
    """Row gather; a pure copy, so bf16 rows travel as they are (viewed as half as many 4-byte words).  The backward
    (segmented sum over the rows pointing at each source row) accumulates in fp32."""

    @staticmethod
    def forward(ctx, x, idx):
        _lib.need_device('train_ops', x, idx)
        if x.dtype not in (torch.float32,) + LOW or (x.dtype in LOW and x.shape[1] % 2):
            x = x.float()
        x = x.contiguous()
        idx = idx.contiguous()
        out = torch.empty((idx.numel(), x.shape[1]), device=x.device, dtype=x.dtype)
        words = x.shape[1] if x.dtype == torch.float32 else x.shape[1] // 2
        _lib.call('pps_gather_rows_f32', x, idx, idx.numel(), words, out)
        ctx.save_for_backward(idx)
        ctx.n = x.shape[0]
        ctx.dtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, = ctx.saved_tensors
        if idx.numel() == 0:
            return torch.zeros((ctx.n, dout.shape[1]), device=dout.device, dtype=ctx.dtype), None
        order, offsets = csr(idx, ctx.n)
        dout = dout.contiguous()
        dx = _empty32(dout.device, ctx.n, dout.shape[1])
        if dout.dtype in LOW and dout.shape[1] % 4 == 0:
            _lib.call('pps_segment_sum_rows_16', dout, order, offsets, ctx.n, dout.shape[1], _code(dout.dtype), dx)
        else:
            dout = dout.float()
            _lib.call('pps_segment_sum_rows_f32', dout, order, offsets, ctx.n, dout.shape[1], dx)
        return dx.to(ctx.dtype), None


class _HeadInput(torch.autograd.Function):
    """h1[(q,j)] = table[ids[q,j]] + wx (query[q] - pts[ids[q,j]]): gather, neighbour offset, 3 -> C layer and sum of the interpolation head's
    first layer in one pass (pps_head_input_fwd); backward: d table by the segmented sum of the gather, d wx by pps_head_input_dwx."""

    @staticmethod
    def forward(ctx, table, ids, pts, query, k, wx):
        _lib.need_device('train_ops', table, ids, pts, query, wx)
        table = _low(table)
        ids = ids.contiguous()
        pts32, q32, wx32 = _f32(pts), _f32(query), _f32(wx)
        nq, c = q32.shape[0], table.shape[1]
        h1 = torch.empty((nq * k, c), device=table.device, dtype=table.dtype)
        _lib.call('pps_head_input_fwd', table, ids, pts32, q32, nq, k, c, _code(table.dtype), wx32, h1)
        ctx.save_for_backward(ids, pts32, q32)
        ctx.meta = (table.shape[0], k, wx.dtype, wx.shape, table.dtype)
        return h1

    @staticmethod
    def backward(ctx, dh1):
        n, k, wdt, wshape, dt = ctx.meta
        dtable, dwx = _head_input_bwd(dh1.to(dt).contiguous(), *ctx.saved_tensors, n, k, wshape, wdt, ctx.needs_input_grad[0], ctx.needs_input_grad[5])
        return dtable, None, None, None, None, dwx


def _head_input_bwd(dh1, ids, pts32, q32, n, k, wshape, wdt, need_table, need_wx):
    """Backward of the head's first layer from dh1 [Q*k, C] (16-bit, contiguous) -> (d table [n, C] in dh1's type by the segmented sum of the gather,
    d wx in wx's shape and type by pps_head_input_dwx); None for what is not needed.  Shared by _HeadInput and _HeadChain."""
    c, dt, dev = dh1.shape[1], dh1.dtype, dh1.device
    dtable = dwx = None
    if need_table:
        order, offsets = csr(ids, n)
        dt32 = _empty32(dev, n, c)
        _lib.call('pps_segment_sum_rows_16', dh1, order, offsets, n, c, _code(dt), dt32)
        dtable = dt32.to(dt)
    if need_wx:
        dwx = _empty32(dev, c, 3)
        _lib.call('pps_head_input_dwx', dh1, ids, pts32, q32, q32.shape[0], k, c, _code(dt), dwx, _ws(_lib.lib().pps_head_input_ws_bytes(c), dev))
        dwx = dwx.reshape(wshape).to(wdt)
    return dtable, dwx


def head_input_supported(c):
    return c % 8 == 0 and 256 % (c // 8) == 0


def head_input(table, ids, pts, query, k, wx):
    """table [N, C] (bf16), ids [Q*k] rows of table / pts, pts [N, 3], query [Q, 3], wx [C, 3] -> h1 [Q*k, C] bf16 (before its ReLU)."""
    return _HeadInput.apply(table, ids, pts, query, k, wx)


class _NeighbourMax(torch.autograd.Function):
    """x fp32, or 16-bit storage (kept: the maximum of stored values is one of them; the incoming gradient is read in that type, summed in fp32
    and rounded once -- the values an fp32 op between two casts produces, without the four cast kernels)."""

    @staticmethod
    def forward(ctx, x, idx):
        _lib.need_device('train_ops', x, idx)
        if x.dtype not in LOW:
            x = x.float()
        x = x.contiguous()
        idx = idx.contiguous()
        m, k = idx.shape
        c = x.shape[1]
        out = torch.empty((m, c), device=x.device, dtype=x.dtype)
        arg = torch.empty((m, c), device=x.device, dtype=torch.int32)
        if x.dtype in LOW:
            _lib.call('pps_gather_max_arg_16', x, idx, m, k, c, _code(x.dtype), out, arg)
        else:
            _lib.call('pps_gather_max_arg_f32', x, idx, m, k, c, out, arg)
        ctx.save_for_backward(idx, arg)
        ctx.n = x.shape[0]
        ctx.dtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, arg = ctx.saved_tensors
        order, offsets = csr(idx.view(-1), ctx.n)
        dout = dout.contiguous().to(ctx.dtype)
        c = dout.shape[1]
        dx = torch.empty((ctx.n, c), device=dout.device, dtype=ctx.dtype)
        if ctx.dtype in LOW:
            _lib.call('pps_gather_max_bwd_16', dout, arg, order, offsets, ctx.n, idx.shape[1], c, _code(ctx.dtype), dx)
        else:
            _lib.call('pps_gather_max_bwd_f32', dout, arg, order, offsets, ctx.n, idx.shape[1], c, dx)
        return dx, None


class _NeighbourContract(torch.autograd.Function):
    """x [n,c] in fp32 or, when the matrix-pipe kernels take the shape (c % 16 == 0, k <= 16), in the 16-bit type it arrives in: the output has x's
    type and the incoming gradient is read in it (no cast kernels around the op in an autocast step); g, dg and the arithmetic are fp32."""

    @staticmethod
    def forward(ctx, x, idx, g):
        _lib.need_device('train_ops', x, idx, g)
        m, k = idx.shape
        c = x.shape[1]
        low = x.dtype in LOW and bool(_lib.lib().pps_neighbour_contract_16_supported(k, c))
        if not low:
            x = x.float()
        x, idx, g = x.contiguous(), idx.contiguous(), g.float().contiguous()
        if g.shape != (m, k, 16):
            raise ValueError('neighbour_contract: g must be [m, k, 16], got {}'.format(tuple(g.shape)))
        out = torch.empty((m, c * 16), device=x.device, dtype=x.dtype)
        _lib.call('pps_neighbour_contract_fwd', x, idx, g, m, k, c, _code(x.dtype), out)
        ctx.save_for_backward(x, idx, g)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, idx, g = ctx.saved_tensors
        m, k = idx.shape
        n, c = x.shape
        dout = dout.to(x.dtype).contiguous()
        need_x, _, need_g = ctx.needs_input_grad
        dxg = _empty32(x.device, m * k, c) if need_x else None
        dg = _empty32(x.device, m, k, 16) if need_g else None
        if need_x or need_g:
            _lib.call('pps_neighbour_contract_bwd', x, idx, g, dout, m, k, c, _code(x.dtype), dxg if need_x else None, dg if need_g else None)
        dx = None
        if need_x:
            order, offsets = csr(idx.view(-1), n)
            dx = _empty32(x.device, n, c)
            _lib.call('pps_segment_sum_rows_f32', dxg, order, offsets, n, c, dx)
        return dx, None, dg


GEO_FLOATS = 1140          # pps_fkaconv_geo_floats(): radius, alpha, beta, act, fc1 [16,3], fc2 [16,32], fc3 [16,32], IN1 w/b, IN2 w/b


class _FkaGeometry(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, geo, pts, sup, idx, b, m, momentum, owned=False):
        _lib.need_device('train_ops', geo, pts, sup, idx)
        pts, sup, idx = pts.contiguous(), sup.contiguous(), idx.contiguous()
        k = idx.shape[1]
        if geo.numel() != GEO_FLOATS or idx.shape[0] != b * m or sup.shape[0] != b * m:
            raise ValueError('fka_geometry: inconsistent sizes')
        # the kernel moves entry 0 (norm_radius) in place: on a copy, unless the caller hands over a vector nobody else reads (pack_geo's)
        geo_w = geo.detach() if owned and geo.is_contiguous() and geo.dtype == torch.float32 else geo.detach().clone().contiguous()
        g, stat = _empty32(pts.device, b * m, k, 16), _empty32(pts.device, 2, b, 32)
        ws = _ws(_lib.lib().pps_fka_train_ws_bytes(b, m, k), pts.device)
        _lib.call('pps_fka_geometry_fwd_f32', pts, sup, idx, b, m, k, geo_w, float(momentum), g, stat, ws)
        ctx.save_for_backward(pts, sup, idx, geo_w, stat)
        ctx.dims = (b, m, k)
        radius = geo_w[0:1]                                     # (a view: the caller copies it into the layer's buffer)
        ctx.mark_non_differentiable(radius)
        ctx.set_materialize_grads(False)                        # no zero tensor for the gradient of radius that nobody computes
        return g, radius

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, dg, _dradius):
        if dg is None:
            return None, None, None, None, None, None, None, None
        pts, sup, idx, geo_w, stat = ctx.saved_tensors
        b, m, k = ctx.dims
        dg = dg.contiguous().float()
        dgeo = _empty32(dg.device, GEO_FLOATS)
        ws = _ws(_lib.lib().pps_fka_train_ws_bytes(b, m, k), dg.device)
        _lib.call('pps_fka_geometry_bwd_f32', pts, sup, idx, b, m, k, geo_w, stat, dg, dgeo, ws)
        return dgeo, None, None, None, None, None, None, None


def fka_geometry(geo, pts, sup, idx, b, m, momentum, owned=False):
    """geo: packed small parameters of the layer (differentiable); pts [rows,3], sup [b*m,3], idx int64 [b*m,k] rows of pts.
    momentum > 0: train() -- norm_radius is first moved towards the mean neighbourhood radius, the new value is used and
    returned.  owned: geo is a temporary of the caller's (its entry 0 may be overwritten with the new norm_radius) -- saves the copy.
    -> (g [b*m,k,16], norm_radius [1])."""
    return _FkaGeometry.apply(geo, pts, sup, idx, b, m, momentum, owned)


def _bn_fwd_args(op, x, weight, bias):
    """What the two BatchNorm nodes prepare alike -> (x fp32 or 16-bit and contiguous, w32, b32, y, save [2, c], workspace); `op` names the node in
    the error for a shape the reduction does not take."""
    if x.dtype not in (torch.float32,) + LOW:
        x = x.float()
    x = x.contiguous()
    rows, c = x.shape
    w32, b32 = _f32(weight), _f32(bias)
    y = torch.empty_like(x)
    save = _empty32(x.device, 2, c)
    nbytes = _lib.lib().pps_bn_train_ws_bytes(rows, c)
    if nbytes == 0 and rows > 0:
        raise ValueError('{}: unsupported shape [{}, {}]'.format(op, rows, c))
    return x, w32, b32, y, save, _ws(nbytes, x.device, 1)


def _bn_bwd_args(x, dy):
    """-> (dy in x's type, dx, dgamma, dbeta, workspace) of the two BatchNorm nodes' backward."""
    rows, c = x.shape
    return (dy.to(x.dtype).contiguous(), torch.empty_like(x), _empty32(x.device, c), _empty32(x.device, c),
            _ws(_lib.lib().pps_bn_train_ws_bytes(rows, c), x.device, 1))


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu):
        _lib.need_device('train_ops', x, weight, bias)
        x, w32, b32, y, save, ws = _bn_fwd_args('bn_act', x, weight, bias)
        _lib.call('pps_bn_train_fwd', x, x.shape[0], x.shape[1], _code(x.dtype), w32, b32, running_mean, running_var, float(momentum), float(eps),
                  int(bool(relu)), y, save, ws)
        ctx.save_for_backward(x, w32, b32, save)
        ctx.relu = bool(relu)
        ctx.dtypes = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32, b32, save = ctx.saved_tensors
        dy, dx, dgamma, dbeta, ws = _bn_bwd_args(x, dy)
        _lib.call('pps_bn_train_bwd', x, dy, x.shape[0], x.shape[1], _code(x.dtype), w32, b32, save, int(ctx.relu), dx, dgamma, dbeta, ws)
        return dx, dgamma.to(ctx.dtypes[0]), dbeta.to(ctx.dtypes[1]), None, None, None, None, None


class _BnAddRelu(torch.autograd.Function):
    """relu(BatchNorm(x) + res) in train(): the tail of a residual block inside the BatchNorm's apply pass (pps_bn_add_relu_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, running_mean, running_var, momentum, eps):
        _lib.need_device('train_ops', x, res, weight, bias)
        x, w32, b32, y, save, ws = _bn_fwd_args('bn_add_relu', x, weight, bias)
        res = res.to(x.dtype).contiguous()
        _lib.call('pps_bn_add_relu_fwd', x, res, x.shape[0], x.shape[1], _code(x.dtype), w32, b32, running_mean, running_var, float(momentum),
                  float(eps), y, save, ws)
        ctx.save_for_backward(x, res, w32, b32, save)
        ctx.dtypes = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, w32, b32, save = ctx.saved_tensors
        dy, dx, dgamma, dbeta, ws = _bn_bwd_args(x, dy)
        dres = torch.empty_like(x)
        _lib.call('pps_bn_add_relu_bwd', x, res, dy, x.shape[0], x.shape[1], _code(x.dtype), w32, b32, save, dx, dres, dgamma, dbeta, ws)
        return dx, dres, dgamma.to(ctx.dtypes[0]), dbeta.to(ctx.dtypes[1]), None, None, None, None


def bn_add_relu(x, res, weight, bias, running_mean, running_var, momentum, eps):
    """relu(BatchNorm1d(x) + res) over the rows of x [rows, c] in train() mode (batch statistics, running statistics updated in place)."""
    return _BnAddRelu.apply(x, res, weight, bias, running_mean, running_var, momentum, eps)


def col_sum(x):
    """x [rows, c] -> fp32 [c] column sums (the bias gradient of a row layer) by the HIP reduction; None if the shape is not one it takes
    (the caller then uses torch's sum).  x may be a block of columns of a wider contiguous tensor (unit column stride, row stride and first column
    multiples of 4): summed where it lies.  No autograd: called from backward passes."""
    if not x.is_cuda or x.dim() != 2 or x.dtype not in (torch.float32,) + LOW:
        return None
    rows, c = x.shape
    ld = x.stride(0) if rows > 1 else c
    if rows < 1 or (c > 1 and x.stride(1) != 1) or ld < c or ld % 4 or x.data_ptr() % (4 * x.element_size()):
        return None
    nbytes = _lib.lib().pps_bn_train_ws_bytes(rows, c)
    if nbytes == 0:
        return None
    out = _empty32(x.device, c)
    _lib.call('pps_col_sum_strided', x, rows, c, ld, _code(x.dtype), out, _ws(nbytes, x.device))
    return out


def sum_rows(x):
    """x [rows, c] -> [c] sums over the rows in fp32: the HIP reduction wherever it takes the shape (any c: blocks of <= 1024 columns, narrow tensors
    padded to 4 columns), torch's sum only for what is left (non-contiguous / other types).  The step's own reductions go through here so that a
    replayed HIP graph runs the same reduction kernels as the eager step (train_graph._bias_grad: torch's sum of a [rows, 4096] tensor did not
    replay like it ran eagerly; ADVICE r5 asked for the rest of the class to follow)."""
    if x.dim() == 2 and x.is_cuda and x.dtype in (torch.float32,) + LOW:
        x = x.contiguous()
        rows, c = x.shape
        if c % 4:
            pad = 4 - c % 4
            return sum_rows(torch.cat([x, x.new_zeros((rows, pad))], dim=1))[:c]
        if c <= 1024:
            out = col_sum(x)
            if out is not None:
                return out
            if c < 64:                                   # column counts the kernel's thread layout does not divide: pad to the next power of two
                width = 4
                while width < c:
                    width *= 2
                if width != c:
                    return sum_rows(torch.cat([x, x.new_zeros((rows, width - c))], dim=1))[:c]
        else:
            parts = [col_sum(x[:, i:min(i + 1024, c)]) for i in range(0, c, 1024)]        # column blocks summed where they lie
            if all(q is not None for q in parts):
                return torch.cat(parts)
    return x.sum(0, dtype=torch.float32)


class _AffineRows(torch.autograd.Function):
    """x [rows, c] * scale [c] + shift [c] (fp32) with the parameter gradients summed over the rows by the HIP reduction (autograd's own broadcast
    backward is torch.sum: see sum_rows)."""

    @staticmethod
    def forward(ctx, x, scale, shift):
        ctx.save_for_backward(x, scale)
        return x * scale + shift

    @staticmethod
    def backward(ctx, g):
        x, scale = ctx.saved_tensors
        g = g.float()
        dx = g * scale if ctx.needs_input_grad[0] else None
        dscale = sum_rows(g * x).to(scale.dtype) if ctx.needs_input_grad[1] else None
        dshift = sum_rows(g).to(scale.dtype) if ctx.needs_input_grad[2] else None
        return dx, dscale, dshift


def affine_rows(x, scale, shift):
    return _AffineRows.apply(x, scale, shift)


def gemm_supported(x, k):
    """The hand-written dense-layer kernels (csrc/pps_gemm_train.hip) take this operand: device tensor in a 16-bit storage type, contraction length a
    multiple of 8."""
    return x.is_cuda and x.dtype in LOW and k % 8 == 0 and k >= 8


def _gemm_operand(t):
    """t [rows, cols] as the dense-layer kernels read it: unit column stride, a row pitch that is a multiple of 8 elements and a 16-byte aligned
    address (a block of columns of a wider tensor is read where it lies); copied only when it is not like that."""
    return t.contiguous() if t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16 else t


def gemm_nt(x, w, bias=None, out_f32=False):
    """x [M, K] @ w [N, K]^T (+ bias [N] fp32) -> [M, N] in x's 16-bit type (or fp32): pps_gemm_nt_16.  No autograd (called from autograd functions)."""
    _lib.need_device('train_ops', x, w)
    assert x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1] and x.dtype == w.dtype and x.dtype in LOW
    x, w = _gemm_operand(x), _gemm_operand(w)
    m, k = x.shape
    n = w.shape[0]
    y = torch.empty((m, n), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    _lib.call('pps_gemm_nt_16', x, x.stride(0), w, w.stride(0), _f32(bias), y, n, m, n, k, _code(x.dtype), int(bool(out_f32)))
    return y


def gemm_tn(g, x):
    """g [M, N]^T @ x [M, K] -> fp32 [N, K] (the weight gradient of a row layer: contraction over the rows): pps_gemm_tn_16.  N, K multiples of 8."""
    _lib.need_device('train_ops', g, x)
    assert g.dim() == 2 and x.dim() == 2 and g.shape[0] == x.shape[0] and g.dtype == x.dtype and g.dtype in LOW
    g, x = _gemm_operand(g), _gemm_operand(x)
    m, n = g.shape
    k = x.shape[1]
    dw = _empty32(g.device, n, k)
    ws = _ws(_lib.lib().pps_gemm_tn_ws_bytes(m, n, k), g.device, 16)
    _lib.call('pps_gemm_tn_16', g, g.stride(0), x, x.stride(0), m, n, k, _code(g.dtype), dw, ws)
    return dw


class _AttnPool(torch.autograd.Function):
    """pooled[q] = sum_j mean_h softmax_j(qy[q,j,h]) * h[q,j]  (poco_model.py:412-414 in the pooled form): one HIP kernel forward, one
    backward; fp32 or bf16 storage, fp32 arithmetic; the softmax is recomputed in backward, only the two inputs are saved."""

    @staticmethod
    def forward(ctx, qy, h, relu_h=False):
        _lib.need_device('train_ops', qy, h)
        ctx.relu_h = int(bool(relu_h))
        dt = h.dtype if h.dtype in (torch.float32,) + LOW else torch.float32
        qy, h = qy.to(dt).contiguous(), h.to(dt).contiguous()
        q, k, heads = qy.shape
        c = h.shape[2]
        pooled = torch.empty((q, c), device=h.device, dtype=dt)
        _lib.call('pps_attn_pool_fwd', qy, h, q, k, heads, c, _code(dt), ctx.relu_h, pooled)
        ctx.save_for_backward(qy, h)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        qy, h = ctx.saved_tensors
        q, k, heads = qy.shape
        c = h.shape[2]
        dpooled = dpooled.to(h.dtype).contiguous()
        dqy, dh = torch.empty_like(qy), torch.empty_like(h)
        _lib.call('pps_attn_pool_bwd', qy, h, dpooled, q, k, heads, c, _code(h.dtype), ctx.relu_h, dqy, dh)
        return dqy, dh, None


class Act:
    """A layer output that is NOT stored in its activated form: `raw` [rows, C] bf16 plus the per-channel `affine` [2, C] (scale, shift;
    None = identity) and `relu` that the consumer applies while loading -- act = relu?(raw * scale + shift)."""
    __slots__ = ('raw', 'affine', 'relu')

    def __init__(self, raw, affine=None, relu=False):
        self.raw, self.affine, self.relu = raw, affine, relu

    def materialize(self):
        if self.affine is None:
            return torch.relu(self.raw) if self.relu else self.raw
        z = self.raw.float() * self.affine[0] + self.affine[1]
        return (torch.relu(z) if self.relu else z).to(self.raw.dtype)


def _rows_fwd(x, in_affine, in_relu, w, b, bn=None):
    """The one caller of pps_rows_layer_fwd: y = act(x) W^T + b with x in its stored form (in_affine [2, cin] or None, in_relu applied on load);
    bn = (gamma, beta, running_mean, running_var, momentum, eps) takes the batch statistics of y on store (running statistics updated in place), None
    leaves them.  -> (x, aff, w32, g32, save, y) in the order the nodes save them for _rows_bwd, and out_affine [2, cout] (save, out_affine, g32: None
    without bn)."""
    x = _low(x)
    rows, cin = x.shape
    cout = w.shape[0]
    dev = x.device
    w32, b32, aff = _f32(w), _f32(b), _f32(in_affine)
    gamma, beta, running_mean, running_var, momentum, eps = bn or (None,) * 6
    g32, be32 = _f32(gamma), _f32(beta)
    y = torch.empty((rows, cout), device=dev, dtype=x.dtype)
    out_affine = _empty32(dev, 2, cout) if bn else None
    save = _empty32(dev, 2, cout) if bn else None
    ws = _ws(_lib.lib().pps_rows_layer_ws_bytes(cin, cout), dev)
    _lib.call('pps_rows_layer_fwd', x, rows, cin, _code(x.dtype), aff, _row1(aff, cin), int(bool(in_relu)), w32,
              b32, cout, y, g32, be32, running_mean, running_var, float(momentum or 0.0), float(eps or 0.0), out_affine,
              save, ws)
    return (x, aff, w32, g32, save, y), out_affine


def _rows_meta(in_relu, w, b):
    """What _rows_bwd needs of a layer besides its saved tensors: (in_relu, dtype of w, dtype of b or None)."""
    return bool(in_relu), w.dtype, None if b is None else b.dtype


def _rows_bwd(ctx, entry, grad_args, saved, meta, g_affine):
    """The one place that allocates the gradients and the workspace of a row layer and calls its backward entry.  `entry` says how the gradient of
    the raw output y arrives, `grad_args` are that entry's own leading arguments:
        'rows'    (gy [rows, cout],)                 the gradient as a tensor                          pps_rows_layer_bwd
        'pooled'  (gval, arg, p)                     one value per (group, channel) in row arg        pps_rows_layer_bwd_pooled
        'rank2'   (a, dl, dpooled, v, p)             a[q, j] dpooled[q, :] + dl[q, j] v per group     pps_rows_layer_bwd_rank2
    saved = (x, aff, w32, g32, save, y) of _rows_fwd, meta of _rows_meta, g_affine [2, cout] the gradient of the layer's BatchNorm affine (None
    without one).  ctx.needs_input_grad[0 / 1] must be those of x / in_affine.  -> the gradients of the first seven arguments every row-layer
    forward has: (dx, d_in_affine, None, dw, db, dgamma, dbeta) in the parameters' types."""
    x, aff, w32, g32, save, y = saved
    in_relu, wdt, bdt = meta
    rows, cin = x.shape
    cout = w32.shape[0]
    dev = x.device
    bn = g32 is not None
    need_dx, need_daff = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and aff is not None
    dx = torch.empty_like(x) if (need_dx or need_daff) else None
    d_in = _empty32(dev, 2, cin) if need_daff else None
    dw = _empty32(dev, cout, cin)
    db = _empty32(dev, cout) if bdt is not None else None
    dgamma = _empty32(dev, cout) if bn else None
    dbeta = _empty32(dev, cout) if bn else None
    ws = _ws(_lib.lib().pps_rows_layer_ws_bytes(cin, cout), dev)
    code, shift, in_relu, g_affine = _code(x.dtype), _row1(aff, cin), int(in_relu), (g_affine if bn else None)
    if entry == 'rows':                                      # (spelled out, not starred: tests/test_call_layer_cpu.py counts each site's arguments)
        gy, = grad_args
        _lib.call('pps_rows_layer_bwd', x, y, gy, rows, cin, cout, code, aff, shift, in_relu, w32, g32, save, g_affine, dx, None, d_in, dw, db,
                  dgamma, dbeta, ws)                         # (None: no second gradient of x to add, dx_add)
    elif entry == 'pooled':
        gval, arg, p = grad_args
        _lib.call('pps_rows_layer_bwd_pooled', x, y, gval, arg, p, rows, cin, cout, code, aff, shift, in_relu, w32, g32, save, g_affine, dx, d_in,
                  dw, db, dgamma, dbeta, ws)
    else:
        a, dl, dpooled, v, p = grad_args
        _lib.call('pps_rows_layer_bwd_rank2', x, y, a, dl, dpooled, v, p, rows, cin, cout, code, aff, shift, in_relu, w32, g32, save, g_affine, dx,
                  d_in, dw, db, dgamma, dbeta, ws)
    return dx if need_dx else None, d_in, None, dw.to(wdt), None if db is None else db.to(bdt), dgamma, dbeta


class _RowsLayer(torch.autograd.Function):
    """y = act(x) W^T + b over rows with the input's BatchNorm + ReLU applied on load and the output's batch statistics taken on store
    (pps_rows_train.hip).  Returns (y bf16, out_affine [2, cout] or None)."""

    @staticmethod
    def forward(ctx, x, in_affine, in_relu, w, b, gamma, beta, running_mean, running_var, momentum, eps):
        _lib.need_device('train_ops', x, w)
        bn = None if gamma is None else (gamma, beta, running_mean, running_var, momentum, eps)
        saved, out_affine = _rows_fwd(x, in_affine, in_relu, w, b, bn)
        ctx.save_for_backward(*saved)
        ctx.meta = _rows_meta(in_relu, w, b)
        return saved[5], out_affine

    @staticmethod
    def backward(ctx, gy, g_affine):
        saved = ctx.saved_tensors
        x, g32 = saved[0], saved[3]
        gy = gy.to(x.dtype).contiguous()
        if g32 is not None:
            g_affine = torch.zeros((2, g32.shape[0]), device=x.device, dtype=torch.float32) if g_affine is None else g_affine.float().contiguous()
        return _rows_bwd(ctx, 'rows', (gy,), saved, ctx.meta, g_affine) + (None, None, None, None)


def _extrema_act(raw, affine, relu, groups, p, arg_dtype=torch.int32):
    """max over the p rows of every group of relu?(raw * scale + shift) from the extrema of the RAW rows (pps_rows_extrema_16): the activation is
    monotone per channel, so the maximum is taken where scale >= 0 and the minimum elsewhere, and only that value is activated.  affine [2, c] or
    None (identity).  -> (out [groups, c] fp32, ext the chosen raw extremum, arg (arg_dtype) its row in the group, scale fp32 or None, live = out > 0
    under relu or None): the last four are what the backward pass needs."""
    c = raw.shape[1]
    dev = raw.device
    mx, mn = torch.empty((groups, c), device=dev), torch.empty((groups, c), device=dev)
    amx, amn = torch.empty((groups, c), device=dev, dtype=torch.int32), torch.empty((groups, c), device=dev, dtype=torch.int32)
    _lib.call('pps_rows_extrema_16', raw, groups, p, c, _code(raw.dtype), mx, mn, amx, amn)
    if affine is None:
        ext, arg, out = mx, amx, mx
        scale = None
    else:
        scale, shift = affine[0].float(), affine[1].float()
        up = scale >= 0
        ext, arg = torch.where(up, mx, mn), torch.where(up, amx, amn).to(arg_dtype)
        out = ext * scale + shift
    live = None
    if relu:
        live = out > 0
        out = torch.relu(out)
    return out, ext, arg, scale, live


def _extrema_act_bwd(dout, ext, scale, live, need_daff):
    """Start of the backward pass of _extrema_act -> (gradient of (scale, shift) [2, c] or None, gradient of the chosen raw value [groups, c] fp32)."""
    d = dout.float()
    if live is not None:
        d = d * live
    daff = torch.stack([sum_rows(d * ext), sum_rows(d)]) if need_daff else None
    return daff, (d if scale is None else d * scale)


class _RowsLayerMax(torch.autograd.Function):
    """rows_layer (with BatchNorm statistics) followed by act_max over the p rows of every group, as ONE node: the raw output is stored (its
    own backward needs it), but the gradient that comes back is one value per (group, channel) in the winning row -- pps_rows_layer_bwd_pooled
    rebuilds those rows on load, so the [rows, cout] gradient tensor (98 % zeros at p = 50) is neither written nor read (three passes over
    512 MB per step for the STN of PointNet).  Returns the activated maxima [groups, cout] fp32."""

    @staticmethod
    def forward(ctx, x, in_affine, in_relu, w, b, gamma, beta, running_mean, running_var, momentum, eps, relu, groups, p):
        _lib.need_device('train_ops', x, w)
        saved, out_affine = _rows_fwd(x, in_affine, in_relu, w, b, (gamma, beta, running_mean, running_var, momentum, eps))
        out, ext, arg, scale, live = _extrema_act(saved[5], out_affine, relu, groups, p, torch.uint8)          # (p <= 255: a byte per winning row)
        ctx.save_for_backward(*saved, ext, arg, scale.clone(), live)
        ctx.meta = _rows_meta(in_relu, w, b)
        ctx.p = int(p)
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, (ext, arg, scale, live) = ctx.saved_tensors[:6], ctx.saved_tensors[6:]
        g_affine, gval = _extrema_act_bwd(dout, ext, scale, live, True)          # gradient of (scale, shift) of this layer's BatchNorm
        gval = gval.to(saved[0].dtype).contiguous()                             # gradient of the raw output, per (group, channel)
        return _rows_bwd(ctx, 'pooled', (gval, arg, ctx.p), saved, ctx.meta, g_affine) + (None,) * 7


class _Rows3Layer(torch.autograd.Function):
    """conv0a of PointNet in train(): x [rows, 3] fp32 -> (y [rows, 64] bf16, out_affine [2, 64] of the BatchNorm on y); x gets no gradient."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, momentum, eps):
        _lib.need_device('train_ops', x, w)
        x = _f32(x)
        rows = x.shape[0]
        w32, b32, g32, be32 = _f32(w), _f32(b), _f32(gamma), _f32(beta)
        dt = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else torch.bfloat16
        y = torch.empty((rows, 64), device=x.device, dtype=dt if dt in LOW else torch.bfloat16)
        aff, save = _empty32(x.device, 2, 64), _empty32(x.device, 2, 64)
        ws = _ws(_lib.lib().pps_rows3_ws_bytes(), x.device)
        _lib.call('pps_rows3_fwd', x, rows, w32, b32, _code(y.dtype), y, g32, be32, running_mean, running_var, float(momentum), float(eps), aff,
                  save, ws)
        ctx.save_for_backward(x, y, g32, save)
        ctx.meta = (b is not None, w.dtype, None if b is None else b.dtype)
        return y, aff

    @staticmethod
    def backward(ctx, gy, g_aff):
        x, y, g32, save = ctx.saved_tensors
        has_b, wdt, bdt = ctx.meta
        dev = x.device
        gy = gy.to(y.dtype).contiguous()
        g_aff = torch.zeros((2, 64), device=dev) if g_aff is None else g_aff.float().contiguous()
        dw = _empty32(dev, 64, 3)
        db = _empty32(dev, 64) if has_b else None
        dgamma, dbeta = _empty32(dev, 64), _empty32(dev, 64)
        ws = _ws(_lib.lib().pps_rows3_ws_bytes(), dev)
        _lib.call('pps_rows3_bwd', x, y, gy, x.shape[0], _code(y.dtype), g32, save, g_aff, dw, db, dgamma, dbeta, ws)
        return None, dw.to(wdt), None if db is None else db.to(bdt), dgamma, dbeta, None, None, None, None


def rows3_layer(x, w, b, bn, relu=True):
    """x [rows, 3] -> Act(raw [rows, 64] bf16, affine of bn (train() statistics), relu)."""
    y, aff = _Rows3Layer.apply(x, w, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
    return Act(y, aff, relu)


class _PatchTransform(torch.autograd.Function):
    """out[q, i, :] = act(x)[q, i, :] (T[q] + I)^T for groups of p <= 64 rows (PointNet's feature transform, nn.py:330-331): x [Q*p, 64] stored
    activation, t [Q, 64, 64] the RAW output of the STN's fc3 (the identity is added inside) -> [Q*p, 64] bf16."""

    @staticmethod
    def forward(ctx, x, affine, relu, t, p):
        _lib.need_device('train_ops', x, t)
        x = _low(x)
        t16 = t.to(x.dtype).contiguous()
        nq = t16.shape[0]
        aff = _f32(affine)
        out = torch.empty_like(x)
        _lib.call('pps_patch_transform_fwd', x, aff, _row1(aff, 64), int(bool(relu)), t16, 1,
                  nq, p, _code(x.dtype), out)
        ctx.save_for_backward(x, aff, t16)
        ctx.meta = (bool(relu), p, t.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        x, aff, t16 = ctx.saved_tensors
        relu, p, tdt = ctx.meta
        nq = t16.shape[0]
        g = g.to(x.dtype).contiguous()
        dx, dt = torch.empty_like(x), torch.empty_like(t16)
        need_daff = aff is not None and ctx.needs_input_grad[1]
        daff = _empty32(x.device, 2, 64) if need_daff else None
        ws = _ws(_lib.lib().pps_patch_transform_ws_bytes(), x.device)
        _lib.call('pps_patch_transform_bwd', x, aff, _row1(aff, 64), int(relu), t16, 1, g,
                  nq, p, _code(x.dtype), dx, dt, daff, ws)
        return dx, daff, None, dt.to(tdt), None


def patch_transform_supported(p, c):
    return 1 <= p <= 64 and c == 64


def patch_transform(act, t_raw, p):
    """act: Act with 64 channels; t_raw [Q, 64, 64] (fc3 output, identity not yet added) -> [Q*p, 64] bf16."""
    aff = act.affine
    if aff is None and act.relu:
        aff = torch.cat([torch.ones((1, 64), device=act.raw.device), torch.zeros((1, 64), device=act.raw.device)])
    return _PatchTransform.apply(act.raw, aff, act.relu, t_raw, p)


class _PatchAttn(torch.autograd.Function):
    """pooled[q] = sum_j softmax_j(h[q,j] . v) h[q,j] over the k <= 64 rows of every group, h [Q, k, 256] bf16 -> [Q, 256] fp32: logits, softmax
    and pooling in one kernel each way, h read once (pps_attn_train.hip)."""

    @staticmethod
    def forward(ctx, h, v):
        _lib.need_device('train_ops', h, v)
        h = _low(h)
        v32 = _f32(v)
        q, k, c = h.shape
        pooled = _empty32(h.device, q, c)
        _lib.call('pps_patch_attn_fwd', h, v32, q, k, c, _code(h.dtype), pooled)
        ctx.save_for_backward(h, v32)
        ctx.vdtype = v.dtype
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        h, v32 = ctx.saved_tensors
        q, k, c = h.shape
        dpooled = dpooled.float().contiguous()
        dh = torch.empty_like(h)
        part = _empty32(h.device, _lib.lib().pps_patch_attn_partials(q), c)
        _lib.call('pps_patch_attn_bwd', h, v32, dpooled, q, k, c, _code(h.dtype), dh, part)
        return dh, sum_rows(part).to(ctx.vdtype)


def patch_attn_supported(k, c):
    return 1 <= k <= 64 and c == 256


def patch_attn(h, v):
    return _PatchAttn.apply(h, v)


class _ActMax(torch.autograd.Function):
    """max over the p rows of every group of act(raw) = relu?(raw * scale + shift) WITHOUT the activated tensor: the activation is monotone
    per channel, so the extremum of the raw rows (max where scale >= 0, min otherwise) is activated instead (pps_rows_extrema_bf16)."""

    @staticmethod
    def forward(ctx, raw, affine, relu, groups, p):
        _lib.need_device('train_ops', raw)
        raw = _low(raw)
        out, ext, arg, scale, live = _extrema_act(raw, affine, relu, groups, p)
        ctx.save_for_backward(ext, arg, scale, live)
        ctx.meta = (groups, p, raw.shape[1], raw.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        ext, arg, scale, live = ctx.saved_tensors
        groups, p, c, rdt = ctx.meta
        daff, dval = _extrema_act_bwd(dout, ext, scale, live, scale is not None and ctx.needs_input_grad[1])
        draw = torch.zeros((groups, p, c), device=dout.device, dtype=rdt)
        draw.scatter_(1, arg.long().unsqueeze(1), dval.to(rdt).unsqueeze(1))
        return draw.view(groups * p, c), daff, None, None, None


def act_max(act, groups, p):
    """[groups * p, C] stored activation -> [groups, C] fp32: max over the p rows of every group of the ACTIVATED values."""
    return _ActMax.apply(act.raw, act.affine, act.relu, groups, p)


def rows_layer_supported(rows, cin, cout):
    return rows >= 1 and bool(_lib.lib().pps_rows_layer_supported(int(cin), int(cout)))


def rows_layer_max_supported(rows, cin, cout, groups, p):
    return rows == groups * p and bool(_lib.lib().pps_rows_layer_pooled_supported(int(cin), int(cout), int(p)))


def rows_layer_max(act, w, b, bn, relu, groups, p):
    """act_max(rows_layer(act, w, b, bn, relu), groups, p) as one autograd node (see _RowsLayerMax): -> [groups, cout] fp32."""
    return _RowsLayerMax.apply(act.raw, act.affine, act.relu, w, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                               bool(relu), int(groups), int(p))


def rows_layer(act, w, b, bn=None, relu=False):
    """act: Act (input in its stored form); w [cout, cin], b [cout] or None; bn: BatchNorm1d holder whose batch statistics are taken on the
    output (train mode), or None.  -> Act(raw output, affine of bn or None, relu)."""
    if bn is not None:
        y, aff = _RowsLayer.apply(act.raw, act.affine, act.relu, w, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
    else:
        y, aff = _RowsLayer.apply(act.raw, act.affine, act.relu, w, b, None, None, None, None, None, None)
    return Act(y, aff, relu)


class _RowsLayerPatchAttn(torch.autograd.Function):
    """rows_layer with BatchNorm statistics (conv3 / bn3 of PointNet) followed by the single-head attention pooling over the p rows of every group
    (AttentionPoco, source/base/nn.py:84-96, on the RAW layer output: logit = raw . (w_q * scale) + const, and softmax ignores the constant) as
    ONE node.  The raw output is stored (both backward passes need it), but its gradient -- a[q, j] dpooled[q, :] + dl[q, j] v, rank two per group
    -- is never a tensor: pps_patch_attn_bwd_weights returns (a, dl) per row and pps_rows_layer_bwd_rank2 rebuilds the rows on load in the
    input-gradient and the weight-gradient kernel (1 M x 256 bf16 = 512 MB per step: written once and read twice otherwise).
    Returns (pooled raw rows [groups, cout] fp32, out_affine [2, cout]): the caller applies the BatchNorm's affine to the pooled rows (the
    weights of a group sum to 1)."""

    @staticmethod
    def forward(ctx, x, in_affine, in_relu, w, b, gamma, beta, running_mean, running_var, momentum, eps, wq, groups, p):
        _lib.need_device('train_ops', x, w, wq)
        saved, out_affine = _rows_fwd(x, in_affine, in_relu, w, b, (gamma, beta, running_mean, running_var, momentum, eps))
        y = saved[5]
        wq32 = _f32(wq).reshape(-1)
        v = wq32 * out_affine[0]                                                     # the logit's weights on the raw output
        pooled = _empty32(y.device, groups, y.shape[1])
        _lib.call('pps_patch_attn_fwd', y, v, groups, p, y.shape[1], _code(y.dtype), pooled)
        ctx.save_for_backward(*saved, v, wq32, out_affine)
        ctx.meta = _rows_meta(in_relu, w, b)
        ctx.query = (wq.dtype, tuple(wq.shape), groups, p)
        return pooled, out_affine

    @staticmethod
    def backward(ctx, dpooled, g_affine):
        saved, (v, wq32, out_affine) = ctx.saved_tensors[:6], ctx.saved_tensors[6:]
        qdt, qshape, groups, p = ctx.query
        y = saved[5]
        rows, cout = y.shape
        dev = y.device
        dpooled = torch.zeros((groups, cout), device=dev, dtype=torch.float32) if dpooled is None else dpooled.float().contiguous()
        a, dl = _empty32(dev, rows), _empty32(dev, rows)
        part = _empty32(dev, _lib.lib().pps_patch_attn_partials(groups), cout)
        _lib.call('pps_patch_attn_bwd_weights', y, v, dpooled, groups, p, cout, _code(y.dtype), a, dl, part)
        dv = sum_rows(part)
        # v = w_q * scale: d w_q = dv * scale, and the scale of the layer's own BatchNorm gets dv * w_q on top of what its consumers hand back
        dwq = (dv * out_affine[0]).reshape(qshape).to(qdt)
        g_affine = torch.zeros((2, cout), device=dev, dtype=torch.float32) if g_affine is None else g_affine.float().clone()
        g_affine[0] += dv * wq32
        return _rows_bwd(ctx, 'rank2', (a, dl, dpooled, v, p), saved, ctx.meta, g_affine) + (None, None, None, None, dwq, None, None)


def rows_layer_patch_attn_supported(cin, cout, p, rows):
    return bool(_lib.lib().pps_rows_layer_pooled_supported(cin, cout, p)) and patch_attn_supported(p, cout) and rows % p == 0 and rows * p < 1 << 32


def rows_layer_patch_attn(act, w, b, bn, wq, groups, p):
    """act: Act; w [cout, cin]; bn: BatchNorm1d holder (train() statistics on the output); wq: weight of the attention's fc_query [1, cout].
    -> (pooled RAW rows [groups, cout] fp32, affine [2, cout] of bn)."""
    return _RowsLayerPatchAttn.apply(act.raw, act.affine, act.relu, w, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, wq,
                                     groups, p)


def _query_attn_bwd(y3, qy, dpooled, wq32, k, dwq, dbq, ws):
    """Backward of (fc_query, attention pooling) on the stored raw output y3 of fc3 -> d y3 [Q*k, 256]; dwq / dbq are filled.  y3 has two
    consumers.  The pooling's gradient relu'(y3) * a[q, j] * dpooled[q, c] is one multiply per element, so it is NOT stored: pps_attn_pool_bwd_weights
    returns a [Q, k] and the input-gradient kernel of fc_query rebuilds the product where it adds the two gradients (pps_rows_layer_bwd_attn) --
    the [Q*k, 256] tensor (655 MB at 50 x 2000 x 64 rows) is neither written nor read.  PPS_ATTN_GRAD=stored: the pooling gradient goes through
    memory (pps_attn_pool_bwd + dx_add; also taken when rows * k does not fit the kernel's 32-bit row / k)."""
    rows, c = y3.shape
    heads = wq32.shape[0]
    code = _code(y3.dtype)
    dqy, dy3 = torch.empty_like(qy), torch.empty_like(y3)
    if os.environ.get('PPS_ATTN_GRAD', 'rebuilt') != 'stored' and rows * k < 1 << 32:
        a = _empty32(y3.device, rows)
        _lib.call('pps_attn_pool_bwd_weights', qy, y3, dpooled, rows // k, k, heads, c, code, 1, dqy, a)
        _lib.call('pps_rows_layer_bwd_attn', y3, dqy, rows, c, heads, code, wq32, a, dpooled, k, dy3, dwq, dbq, ws)
        return dy3
    _lib.call('pps_attn_pool_bwd', qy, y3, dpooled, rows // k, k, heads, c, code, 1, dqy, dy3)
    _lib.call('pps_rows_layer_bwd', y3, qy, dqy, rows, c, heads, code, None, None, 1, wq32, None, None, None, dy3, dy3, None, dwq, dbq, None, None, ws)
    return dy3


class _QueryAttnPool(torch.autograd.Function):
    """The end of the interpolation head on the stored (pre-ReLU) output y3 of fc3 [Q*k, 256]:  qy = fc_query(relu(y3)),  pooled[q] = sum_j mean_h
    softmax_j(qy) relu(y3)[q, j]  as ONE autograd node: y3 has two consumers, and their two gradients are summed inside the input-gradient
    kernel of fc_query (dx_add) instead of by a separate pass over [Q*k, 256]."""

    @staticmethod
    def forward(ctx, y3, wq, bq, k):
        _lib.need_device('train_ops', y3, wq)
        (y3, _, w32, _, _, qy), _ = _rows_fwd(y3, None, True, wq, bq)
        rows, c = y3.shape
        heads = w32.shape[0]
        pooled = torch.empty((rows // k, c), device=y3.device, dtype=y3.dtype)
        _lib.call('pps_attn_pool_fwd', qy, y3, rows // k, k, heads, c, _code(y3.dtype), 1, pooled)
        ctx.save_for_backward(y3, w32, qy)
        ctx.meta = (k, bq is not None, wq.dtype, None if bq is None else bq.dtype)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        y3, w32, qy = ctx.saved_tensors
        k, has_b, wdt, bdt = ctx.meta
        rows, c = y3.shape
        heads = w32.shape[0]
        dev = y3.device
        dpooled = dpooled.to(y3.dtype).contiguous()
        dw = _empty32(dev, heads, c)
        db = _empty32(dev, heads) if has_b else None
        ws = _ws(_lib.lib().pps_rows_layer_ws_bytes(c, heads), dev)
        dy3 = _query_attn_bwd(y3, qy, dpooled, w32, k, dw, db, ws)
        return dy3, dw.to(wdt), None if db is None else db.to(bdt), None


def query_attn_pool(y3, wq, bq, k):
    """y3 [Q*k, 256] stored BEFORE its ReLU, fc_query weights [heads, 256] -> pooled [Q, 256] bf16."""
    return _QueryAttnPool.apply(y3, wq, bq, k)


class _HeadChain(torch.autograd.Function):
    """head_input -> fc2 -> fc3 -> fc_query -> attention pooling of the interpolation head as ONE autograd node whose forward is the fused chain
    kernel (pps_head_chain_fwd: the rows pass through the three layers in registers, the raw outputs the backward needs are written once) followed
    by pps_attn_pool_fwd.  The backward pass is the sequence of backward entries the separate nodes (_QueryAttnPool, _RowsLayer x 2, _HeadInput)
    run, on the same saved tensors."""

    @staticmethod
    def forward(ctx, table, ids, pts, query, k, wx, w2, b2, w3, b3, wq, bq):
        _lib.need_device('train_ops', table, ids, pts, query, wx, w2, w3, wq)
        table = _low(table)
        ids = ids.contiguous()
        pts32, q32, wx32, w2_32, w3_32, wq32 = _f32(pts), _f32(query), _f32(wx), _f32(w2), _f32(w3), _f32(wq)
        nq, c, heads = q32.shape[0], table.shape[1], wq32.shape[0]
        h1, y2, y3, qy = _head_chain_fwd(table, ids, pts32, q32, k, wx32, w2_32, _f32(b2), w3_32, _f32(b3), wq32, _f32(bq))
        pooled = torch.empty((nq, c), device=table.device, dtype=table.dtype)
        _lib.call('pps_attn_pool_fwd', qy, y3, nq, k, heads, c, _code(table.dtype), 1, pooled)
        ctx.save_for_backward(ids, pts32, q32, w2_32, w3_32, wq32, h1, y2, y3, qy)
        ctx.meta = (table.shape[0], k, wx.dtype, tuple(wx.shape), w2.dtype, w3.dtype, wq.dtype, None if b2 is None else b2.dtype,
                    None if b3 is None else b3.dtype, None if bq is None else bq.dtype)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        ids, pts32, q32, w2_32, w3_32, wq32, h1, y2, y3, qy = ctx.saved_tensors
        n, k, wxdt, wxshape, w2dt, w3dt, wqdt, b2dt, b3dt, bqdt = ctx.meta
        rows, c = y3.shape
        heads = wq32.shape[0]
        dev, dt = y3.device, y3.dtype
        code = _code(dt)
        dpooled = dpooled.to(dt).contiguous()
        # attention pooling + fc_query: the two gradients of y3 are summed inside fc_query's input-gradient kernel
        dwq, dbq = _empty32(dev, heads, c), (_empty32(dev, heads) if bqdt is not None else None)
        ws = _ws(_lib.lib().pps_rows_layer_ws_bytes(c, c), dev)        # (the largest of the three layers)
        dy3 = _query_attn_bwd(y3, qy, dpooled, wq32, k, dwq, dbq, ws)
        # fc3
        dy2 = torch.empty_like(y2)
        dw3, db3 = _empty32(dev, c, c), (_empty32(dev, c) if b3dt is not None else None)
        _lib.call('pps_rows_layer_bwd', y2, y3, dy3, rows, c, c, code, None, None, 1, w3_32, None, None, None, dy2, None, None, dw3, db3, None, None, ws)
        del dy3
        # fc2
        dh1 = torch.empty_like(h1)
        dw2, db2 = _empty32(dev, c, c), (_empty32(dev, c) if b2dt is not None else None)
        _lib.call('pps_rows_layer_bwd', h1, y2, dy2, rows, c, c, code, None, None, 1, w2_32, None, None, None, dh1, None, None, dw2, db2, None, None, ws)
        del dy2
        # head input: d table by the segmented sum of the gather, d wx
        dtable, dwx = _head_input_bwd(dh1, ids, pts32, q32, n, k, wxshape, wxdt, ctx.needs_input_grad[0], ctx.needs_input_grad[5])
        cast = lambda t, d: None if (t is None or d is None) else t.to(d)
        return (dtable, None, None, None, None, dwx, dw2.to(w2dt), cast(db2, b2dt), dw3.to(w3dt), cast(db3, b3dt), dwq.to(wqdt), cast(dbq, bqdt))


def _head_chain_fwd(table, ids, pts32, q32, k, wx32, w2_32, b2_32, w3_32, b3_32, wq32, bq32):
    """The one launch of pps_head_chain_fwd -> (h1, y2, y3 [Q*k, C], qy [Q*k, heads]) in table's type.  The kernel writes whole 256-row units
    (unconditional stores): padded storage, views of the rows -- the padding is never read, so it is not cleared."""
    nq, c, heads = q32.shape[0], table.shape[1], wq32.shape[0]
    dev, dt = table.device, table.dtype
    rows = nq * k
    pad = (rows + 255) // 256 * 256
    h1, y2, y3 = (torch.empty((pad, c), device=dev, dtype=dt)[:rows] for _ in range(3))
    qy = torch.empty((pad, heads), device=dev, dtype=dt)[:rows]
    ws = _ws(_lib.lib().pps_head_chain_ws_bytes(), dev)
    _lib.call('pps_head_chain_fwd', table, ids, pts32, q32, nq, k, _code(dt), wx32, w2_32, b2_32, w3_32, b3_32, wq32, bq32, h1, y2, y3, qy, ws)
    return h1, y2, y3, qy


def head_chain_supported(c, heads, k):
    return c == 256 and heads == 64 and 1 <= k <= 64


_head_chain_checked = {}


def head_chain_trusted(dtype):
    """First-use self-check of the one-kernel head chain, once per process and storage type: a fixed synthetic case (2003 queries x 64
    neighbours on a 10 000-row table; a partial last row unit) through pps_head_chain_fwd and through the separate launches it replaces
    (pps_head_input_fwd + pps_rows_layer_fwd x 3): h1 must be EQUAL, y2 / y3 / qy within four units of the storage type's last place on the
    tensor's scale (the accumulation order inside an MFMA may move a value across a rounding boundary), the chain itself equal on a second launch.  False -> the
    caller keeps to the separate launches (also hand-written HIP kernels) and a warning says so once.  Not run while a stream is being captured
    (the eager warm-up steps of a fit come first); PPS_HEAD_CHAIN_CHECK=0 skips it."""
    hit = _head_chain_checked.get(dtype)
    if hit is not None:
        return hit
    if os.environ.get('PPS_HEAD_CHAIN_CHECK', '1') == '0' or torch.cuda.is_current_stream_capturing():
        return True
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator().manual_seed(20260930)
    r = lambda *sh, scale=1.0: (torch.randn(*sh, generator=g) * scale).to(dev)
    nq, k, n = 2003, 64, 10000
    table = r(n, 256).to(dtype)
    ids = torch.randint(0, n, (nq * k,), generator=g).to(dev)
    pts, query = (torch.rand(n, 3, generator=g) - 0.5).to(dev), (torch.rand(nq, 3, generator=g) - 0.5).to(dev)
    wx, w2, w3, wq = r(256, 3, scale=0.5), r(256, 256, scale=1 / 16), r(256, 256, scale=1 / 16), r(64, 256, scale=1 / 8)
    b2, b3, bq = r(256, scale=0.1), r(256, scale=0.1), r(64, scale=0.1)
    rows = nq * k
    with torch.no_grad(), torch.autocast('cuda', dtype=dtype):
        a = _head_chain_fwd(table, ids, pts, query, k, wx, w2, b2, w3, b3, wq, bq)
        b = _head_chain_fwd(table, ids, pts, query, k, wx, w2, b2, w3, b3, wq, bq)
        h1 = head_input(table, ids, pts, query, k, wx)
        y2 = rows_layer(Act(h1, None, True), w2, b2, None, True)
        y3 = rows_layer(y2, w3, b3, None, True)
        qy = rows_layer(y3, wq, bq, None, True)
    ref = (h1.view(rows, 256), y2.raw.view(rows, 256), y3.raw.view(rows, 256), qy.raw.view(rows, 64))
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    ok = all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[0], ref[0])
    for x, y in zip(a[1:], ref[1:]):                 # (a value that crosses a rounding boundary in one layer moves the next layer's sums by a few ulp of
        ok = ok and float((x.float() - y.float()).abs().max()) <= 4.0 * ulp * float(y.float().abs().max())      # their TERMS: the bar is on the tensor's scale)
    _head_chain_checked[dtype] = ok
    if not ok:
        print('ppsurf_amd: the one-kernel head chain FAILED its first-use self-check ({}); the interpolation head runs as separate launches in this '
              'process (PPS_HEAD_CHAIN=0 selects that form outright)'.format(dtype))
    return ok


def head_chain(table, ids, pts, query, k, wx, fc2, fc3, fc_query):
    """pooled [Q, 256] of the interpolation head from the per-point table: fc2 / fc3 / fc_query are (weight [out, 256], bias or None) pairs."""
    return _HeadChain.apply(table, ids, pts, query, k, wx, fc2[0], fc2[1], fc3[0], fc3[1], fc_query[0], fc_query[1])


def attn_pool_supported(k, heads, c):
    return 1 <= k <= 64 and 1 <= heads <= 64 and c <= 256


def attn_pool(qy, h, relu_h=False):
    """qy [Q,k,64] attention logits, h [Q,k,C] -> pooled [Q,C] (dtype of h).  relu_h: h is the stored PRE-activation, relu(h) is pooled."""
    return _AttnPool.apply(qy, h, relu_h)


def bn_supported(rows, c):
    return c % 4 == 0 and c <= 1024 and 256 % (c // 4) == 0


def bn_act(x, weight, bias, running_mean, running_var, momentum, eps, relu):
    """Train-mode BatchNorm1d over the rows of x [rows, c] (batch statistics, running statistics updated in place) with an
    optional fused ReLU; x fp32 or bf16 (kept), statistics and gradients of the affine parameters in fp32."""
    return _BnAct.apply(x, weight, bias, running_mean, running_var, momentum, eps, relu)


def gather_rows(x, idx):
    return _GatherRows.apply(x, idx)


def neighbour_max(x, idx):
    """A maximum of 16-bit values is one of them: the result goes back to the type it came in (the op computes in fp32), so that the residual
    sum it feeds stays a same-type addition (a bf16 + fp32 addition runs ATen's slow mixed-type kernel and promotes everything downstream)."""
    return _NeighbourMax.apply(x, idx)                    # 16-bit storage in, the same storage out (pps_gather_max_arg_16): no cast kernels


def neighbour_contract(x, idx, g):
    return _NeighbourContract.apply(x, idx, g)
