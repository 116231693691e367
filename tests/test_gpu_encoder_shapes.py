"""Shape sweep of the inference encoder kernels (csrc/pps_fkaconv.hip) against exact and float64 references (tests/encoder_spec.py).

1. rows_gemm / rows_linear / gather_max, EXACT: small-integer operands, so every float32 summation order gives the int64 result.
2. Containment, EXACT: a kernel writes only its rows (sentinel tails behind `out` and the workspace) and reads only the rows its index
   tables name (NaN in every other row of x, pts, in1 and in2 must not change a bit of the output).
3. The FKAConv layer at ragged shapes against the oracle in float64.
4. Residual blocks and the whole network on a 333-point cloud (levels 333, 83, 20, 5, 1) against the oracle in float64.

Tolerance of 3 and 4, per case:  max|gpu - oracle64| <= R * E32 + 2^-23 * max|oracle64|,  E32 = max|oracle32 - oracle64| on the same
inputs (the error the reference's own float32 arithmetic makes), the second term one float32 ulp of the largest output; and the
absolute bar 1e-4 of test_gpu_encoder.py on top.

R is twice the largest ratio max|gpu - oracle64| / E32 measured on the MI355X (the kernels use __expf and keep the InstanceNorm mean and
rstd in float32, so a few times E32 was expected; the cap was 16), taken per group so that the one outlier does not loosen the rest:
R_K1 = 10.82 for the layer at K = 1 ('single', 2 x 5.41) and R = 4.52 for every other case (2 x 2.26):

    case (n, m, k, cin, cout)            relu: error   E32      ratio    silu: error   E32      ratio
    single      (1, 1, 1, 1, 1) x 16     8.14e-07  9.06e-07   0.90       1.02e-06  1.89e-07   5.41
    m1_k7       (9, 1, 7, 3, 8)          1.51e-06  1.91e-06   0.79       2.99e-06  1.83e-06   1.63
    m15_k2      (40, 15, 2, 16, 31)      1.05e-06  9.87e-07   1.06       1.02e-06  2.21e-06   0.46
    m16_k16     (40, 16, 16, 16, 32)     7.26e-06  5.76e-06   1.26       6.23e-06  4.61e-06   1.35
    m17_k15     (40, 17, 15, 24, 33)     6.56e-06  8.83e-06   0.74       6.55e-06  8.58e-06   0.76
    m257_cin40  (300, 257, 16, 40, 96)   8.73e-06  1.23e-05   0.71       8.85e-06  1.13e-05   0.78
    cin512      (64, 33, 16, 512, 64)    2.37e-05  1.10e-05   2.15       2.44e-05  1.08e-05   2.26
    repeats     (5, 3, 16, 16, 16)       6.61e-06  5.79e-06   1.14       7.24e-06  4.26e-06   1.70
    self        (21, 21, 6, 5, 7)        3.30e-06  3.27e-06   1.01       2.99e-06  5.04e-06   0.59
    m17_k15, silu, folded BatchNorm + ReLU                               6.23e-06  6.76e-06   0.92
    RB_same  (333 -> 333, silu)                                          9.53e-07  1.19e-06   0.80
    RB_down  (333 -> 83, silu)                                           1.90e-06  2.44e-06   0.78
    ENC_silu_fixed (333 points)                                          1.77e-06  3.67e-06   0.48
    ENC_relu_poco  (333 points)          2.75e-06  2.63e-06   1.04

(largest outputs: 1.9 to 2.9 for 'single', 3.4 to 25 for the other layer cases, 1.6 to 6.3 for the blocks and networks).  'single' is
16 draws of its one-output shape judged together (encoder_spec.LAYER_DRAWS).  Its silu ratio stands apart from all others.  K = 1
is the one shape at which the layer skips its InstanceNorms, so the unnormalised fc1 outputs go straight into __expf; that this is the
cause has not been measured.  The K = 1 layer inside the networks (ids44) is held to R with everything else.
"""
import numpy as np
import pytest
import torch

import encoder_spec as S
from golden_util import filled_sd
from ppsurf_amd import _lib
from ppsurf_amd.decoder import pack_dense
from ppsurf_amd.encoder import FKAConvParams, ResidualBlockParams, EncoderPlan, LinearParams, gather_max

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
R = 4.52                                # 2 x 2.26 (cin512, silu): every case but the next line's, see the table above
R_K1 = 10.82                            # 2 x 5.41 ('single', silu): the layer alone at K = 1
ATOL = 1e-4                             # the bar of test_gpu_encoder.py
SENTINEL = -12345.5
TAIL_ROWS, WS_TAIL_BYTES = 64, 4096


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pm(t):
    """[1,C,N] channel-first tensor -> point-major device tensor [N,C]."""
    return t[0].T.contiguous().to(DEV)


@pytest.fixture
def entries(monkeypatch):
    """Names of the C ABI entries called while the fixture is live."""
    seen, real = [], _lib.call

    def call(name, *args, **kw):
        seen.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------------------------------------------------
def run_linear(case):
    sd = {'L.weight': case['w'][:, :, None]}
    if case['bias'] is not None:
        sd['L.bias'] = case['bias']
    lin = LinearParams(sd, 'L', DEV)
    out = lin(dev(case['in1']), idx1=dev(case['idx1']), in2=dev(case['in2']), idx2=dev(case['idx2']), residual=dev(case['residual']),
              relu=case['relu'])
    return out.cpu().numpy()


def check_linear_exact(cases, entry, entries):
    for case in cases:
        assert S.exact_bound(case) < 2 ** 24
        del entries[:]
        out = run_linear(case)
        assert [e for e in entries if e.startswith('pps_rows_')] == [entry]
        ref = S.linear_reference(case)
        bad = out != ref
        assert out.shape == ref.shape and not bad.any(), \
            'm {m} c1 {c1} c2 {c2} cout {cout} options {opts:05b}: {n} wrong outputs, first at (row, column) {at}'.format(
                n=int(bad.sum()), at=tuple(np.argwhere(bad)[0]), **{k: case[k] for k in ('m', 'c1', 'c2', 'cout', 'opts')})


@pytest.mark.parametrize('c1,c2', S.ROWS_GEMM_CHANNELS + (S.ROWS_GEMM_LONG,))
def test_rows_gemm_exact(c1, c2, entries):
    """rows_gemm_kernel<2> at every (M, Cout) around the 16-row MFMA tile, the 64-row workgroup and the 32-wide output packing."""
    cases = S.rows_gemm_cases(c1, c2)
    assert all(S.rows_gemm_template(c['m'], c['cout']) == 2 for c in cases)
    check_linear_exact(cases, 'pps_rows_gemm_f32', entries)


@pytest.mark.parametrize('m,c1,c2,cout,nob', S.ROWS_GEMM_WIDE)
def test_rows_gemm_exact_around_the_wide_template(m, c1, c2, cout, nob, entries):
    """launch_rows_gemm takes rows_gemm_kernel<4> when gx * (obt / 4) >= 256 and obt % 4 == 0, with gx = ceil(M / 64) row tiles and
    obt = 2 * ceil(Cout / 32) packed output blocks:
      M = 16389, Cout = 64:  gx = 257, obt = 4 -> 257 * 1 >= 256, 4 % 4 == 0          -> <4>, one output tile
      M = 8133, Cout = 128:  gx = 128, obt = 8 -> 128 * 2 >= 256, 8 % 4 == 0          -> <4>, two output tiles (ob0 = 0, 4)
      M = 16389, Cout = 96:  gx = 257, obt = 6 -> 257 * 1 >= 256 but 6 % 4 == 2       -> <2>, three output tiles
    (the arithmetic is asserted on the CPU in test_encoder_spec_cpu.py)."""
    assert S.rows_gemm_template(m, cout) == nob
    check_linear_exact(S.rows_gemm_wide_cases(m, c1, c2, cout), 'pps_rows_gemm_f32', entries)


@pytest.mark.parametrize('c2', S.ROWS_LINEAR_C2)
@pytest.mark.parametrize('c1', S.ROWS_LINEAR_C1)
def test_rows_linear_exact(c1, c2, entries):
    check_linear_exact(S.rows_linear_cases(c1, c2), 'pps_rows_linear_f32', entries)


def test_gather_max_exact():
    for m in S.GATHER_MAX_M:
        for k in S.GATHER_MAX_K:
            for c in S.GATHER_MAX_C:
                x, ids = S.gather_max_case(m, k, c)
                out = gather_max(dev(x), dev(ids)).cpu().numpy()
                assert np.array_equal(out, x[ids].max(axis=1)), (m, k, c)


# ---------------------------------------------------------------------------------------------------------------------
# 2. containment, at M around the 16-point tile of the FKAConv kernels, padded K and Cin off the 16-channel pass; rows_linear gets
#    c1 = Cin, rows_gemm c1 = 16 Cin, the width at which the layer feeds it its F matrix.
# ---------------------------------------------------------------------------------------------------------------------
CONTAIN_M, CONTAIN_K, CONTAIN_CIN = (1, 15, 17), (1, 7, 16), (3, 24)
contain = pytest.mark.parametrize('m,cin', [(m, c) for m in CONTAIN_M for c in CONTAIN_CIN])


def bits(t):
    return t.cpu().numpy().view(np.int32)


def guarded_out(m, cout):
    """([m + TAIL_ROWS, cout] buffer full of the sentinel, checker): the kernel gets the buffer's address as its [m, cout] output."""
    buf = torch.full((m + TAIL_ROWS, cout), SENTINEL, dtype=torch.float32, device=DEV)

    def check():
        torch.cuda.synchronize()
        assert (buf[m:] == SENTINEL).all(), 'rows behind the {} output rows were written'.format(m)
        assert torch.isfinite(buf[:m]).all() and (buf[:m] != SENTINEL).all()
        return bits(buf[:m])
    return buf, check


def check_linear_containment(entry, m, c1, c2, cout, weights):
    """Both gathers from tables of 2m + 3 rows, once with bias, residual and ReLU and once with NULL bias and residual and no
    activation; then again with NaN in every row of in1 and in2 that idx1 / idx2 do not name.  Integer operands: exact."""
    for opts in (S.ALL_OPTIONS, S.IDX1 | S.IDX2):
        case = S.linear_case(m, c1, c2, cout, opts, table_rows=2 * m + 3)
        w, got = weights(case['w']), []
        for in1, in2 in ((case['in1'], case['in2']), (S.poison_unnamed(case['in1'], case['idx1']), S.poison_unnamed(case['in2'], case['idx2']))):
            out, check = guarded_out(m, cout)
            _lib.call(entry, dev(in1), dev(case['idx1']), c1, dev(in2), dev(case['idx2']), c2, w, dev(case['bias']), dev(case['residual']),
                      int(case['relu']), m, cout, out)
            got.append(check())
        assert np.array_equal(got[0], got[1])
        assert np.array_equal(got[0].view(np.float32), S.linear_reference(case))


@contain
def test_rows_gemm_writes_its_rows_and_reads_named_rows(m, cin):
    check_linear_containment('pps_rows_gemm_f32', m, 16 * cin, 16, 33, lambda w: dev(pack_dense(w)))


@contain
def test_rows_linear_writes_its_rows_and_reads_named_rows(m, cin):
    check_linear_containment('pps_rows_linear_f32', m, cin, 5, 65, lambda w: dev(w.T))


@contain
def test_gather_max_writes_its_rows_and_reads_named_rows(m, cin):
    for k in CONTAIN_K:
        rng = np.random.default_rng([3, m, cin, k])
        x, ids = rng.standard_normal((40, cin)).astype(np.float32), S.sparse_ids(rng, 40, (m, k))
        got = []
        for a in (x, S.poison_unnamed(x, ids)):
            out, check = guarded_out(m, cin)
            _lib.call('pps_gather_max_f32', dev(a), dev(ids), m, k, cin, out)
            got.append(check())
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0].view(np.float32), x[ids].max(axis=1))


@contain
def test_fkaconv_writes_its_rows_and_workspace_and_reads_named_rows(m, cin):
    """Once as the residual blocks use the layer (folded BatchNorm, bias, ReLU epilogue) and once bare (NULL bias, act_out 0: no
    maximum that could swallow a NaN)."""
    n, cout = 40, 33
    sd = S.layer_state_dict(cin, cout, bn='bn')
    ws_bytes = _lib.lib().pps_fkaconv_ws_bytes(m, cin)
    for bn in ('bn', None):
        layer = FKAConvParams(sd, 'L', DEV, 'silu', bn=bn, relu_out=bn is not None)
        assert (layer.bias is None) == (bn is None) and layer.act_out == (1 if bn else 0)
        for k in CONTAIN_K:
            rng = np.random.default_rng([4, m, cin, k])
            x, ids = rng.standard_normal((n, cin)).astype(np.float32), S.sparse_ids(rng, n, (m, k))
            pts = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
            sup = dev(rng.uniform(-0.5, 0.5, (m, 3)).astype(np.float32))
            got = []
            for a, p in ((x, pts), (S.poison_unnamed(x, ids), S.poison_unnamed(pts, ids))):
                out, check = guarded_out(m, cout)
                ws = torch.full((ws_bytes + WS_TAIL_BYTES,), 0xA5, dtype=torch.uint8, device=DEV)
                _lib.call('pps_fkaconv_fwd_f32', dev(a), dev(p), sup, dev(ids), n, m, k, cin, cout, layer.geo, layer.wpack, layer.bias,
                          layer.act_out, out, ws)
                got.append(check())
                assert (ws[ws_bytes:] == 0xA5).all(), 'bytes behind the {} workspace bytes were written (m {}, k {}, cin {})'.format(ws_bytes, m, k, cin)
            assert np.array_equal(got[0], got[1]), (m, k, cin, bn)
            case = dict(x=x, pts=pts, sup=sup.cpu().numpy(), ids=ids)
            np.testing.assert_allclose(got[0].view(np.float32), S.oracle_layer(sd, 'L', case, 'silu', torch.float64, bn=bn), rtol=0, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------------
# 3. and 4. against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def check_against_oracle(tag, got, fn, r=R):
    ref, e32 = S.reference_error(fn)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    top = float(np.abs(ref).max())
    print('{}: max|gpu - oracle64| {:.3e}  E32 {:.3e}  ratio {:.2f}  ulp(max|out|) {:.3e}  max|out| {:.3e}'.format(
        tag, err, e32, err / e32 if e32 else float('inf'), 2.0 ** -23 * top, top))
    assert err <= S.tolerance(ref, e32, r), tag
    assert err <= ATOL, tag


def run_layer(layer, cases):
    """The draws of a case one launch sequence each, stacked along the rows."""
    return np.concatenate([layer(dev(c['x']), dev(c['pts']), dev(c['sup']), dev(c['ids'])).cpu().numpy() for c in cases], axis=0)


@pytest.mark.parametrize('act', ['relu', 'silu'])
@pytest.mark.parametrize('name', list(S.LAYER_CASES))
def test_fkaconv_layer_vs_float64_oracle(name, act):
    n, m, k, cin, cout = S.LAYER_CASES[name]
    sd, cases = S.layer_state_dict(cin, cout), S.layer_draws(name)
    out = run_layer(FKAConvParams(sd, 'L', DEV, act), cases)
    check_against_oracle('layer {} {}'.format(name, act), out, lambda dt: S.oracle_layer_draws(sd, 'L', cases, act, dt), R_K1 if k == 1 else R)


def test_fkaconv_layer_with_folded_batchnorm_and_relu():
    """The layer as ResidualBlockParams uses it: BatchNorm folded into the packed weights and the bias, ReLU in the GEMM epilogue."""
    name = 'm17_k15'
    n, m, k, cin, cout = S.LAYER_CASES[name]
    sd, case = S.layer_state_dict(cin, cout, bn='bn'), S.layer_case(name)
    out = run_layer(FKAConvParams(sd, 'L', DEV, 'silu', bn='bn', relu_out=True), [case])
    assert out.min() == 0 and (out > 0).any()
    check_against_oracle('layer {} silu + bn + relu'.format(name), out, lambda dt: S.oracle_layer(sd, 'L', case, 'silu', dt, bn='bn'))


def ragged_device_inputs():
    """Device tensors of the 333-point cloud as EncoderPlan.forward takes them.  K is what kNN gives: the product's spatial.knn clamps
    k to the number of SOURCE points exactly as the oracle's does, so ids33 / ids34 come with K = 5 and ids44 with K = 1 (where the layer
    skips its InstanceNorms) -- the tables are passed on as they are, nothing is padded to 16."""
    d = S.ragged_cloud()
    ids = {k: (pm(v).reshape(-1) if k in ('ids43', 'ids32', 'ids21', 'ids10') else v[0].contiguous().to(DEV))
           for k, v in d.items() if k.startswith('ids')}
    assert [ids[k].shape[1] for k in ('ids22', 'ids23', 'ids33', 'ids34', 'ids44')] == [16, 16, 5, 5, 1]
    return pm(d['pts']), [pm(d['support{}'.format(i)]) for i in (1, 2, 3, 4)], ids


@pytest.mark.parametrize('key,down', [('RB_same', False), ('RB_down', True)])
def test_residual_block_vs_float64_oracle_at_ragged_sizes(key, down):
    d = S.ragged_cloud()
    pts, sups, ids = ragged_device_inputs()
    sd = filled_sd(key + '.')
    block = ResidualBlockParams(sd, key, DEV, 'silu')
    out = block(pm(d['x16']), pts, sups[0] if down else pts, ids['ids01' if down else 'ids00']).cpu().numpy()
    check_against_oracle(key, out, lambda dt: S.oracle_block(sd, key, down, 'silu', dt))


@pytest.mark.parametrize('key,act,fixed', [('ENC_silu_fixed', 'silu', True), ('ENC_relu_poco', 'relu', False)])
def test_network_vs_float64_oracle_at_ragged_sizes(key, act, fixed):
    pts, sups, ids = ragged_device_inputs()
    sd = filled_sd(key + '.')
    out = EncoderPlan(sd, DEV, prefix=key, act=act, fixed=fixed).forward(pts, sups, ids).cpu().numpy()
    check_against_oracle(key, out, lambda dt: S.oracle_network(sd, key, act, fixed, dt))
