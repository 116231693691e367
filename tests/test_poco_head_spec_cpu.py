"""The POCO head spec itself (tests/poco_head_spec.py) and the algebra of PocoDecoderPlan (fc1 split, packing order, bias offsets,
composed tail, f16x3 image), checked on the CPU."""
import numpy as np
import pytest
import torch

import emulate
import poco_head_spec as S
from ppsurf_amd.decoder import PocoDecoderPlan


def numpy_head(sd, case):
    """interp_attention (poco_model.py:381-419) restated in plain float64 numpy: gather, concatenate, three ReLU layers, softmax over k
    per head, mean over the heads, weighted sum of fc_value, fc8."""
    wb = lambda name: (sd['projection.{}.weight'.format(name)].numpy().astype(np.float64).reshape(sd['projection.{}.bias'.format(name)].shape[0], -1),
                       sd['projection.{}.bias'.format(name)].numpy().astype(np.float64))
    idx = case['idx']
    lat, pts, qry = (case[k].astype(np.float64) for k in ('latents', 'cloud', 'query'))
    x = np.concatenate([lat[0].T[idx], qry[:, None, :] - pts[idx]], axis=2)                     # [q,k,c+3]
    for name in ('fc1', 'fc2', 'fc3'):
        w, b = wb(name)
        x = np.maximum(x @ w.T + b, 0.0)
    wq, bq = wb('fc_query')
    wv, bv = wb('fc_value')
    logit = x @ wq.T + bq                                                                       # [q,k,64]
    e = np.exp(logit - logit.max(axis=1, keepdims=True))
    att = (e / e.sum(axis=1, keepdims=True)).mean(axis=2)                                       # [q,k]
    pooled = np.einsum('qk,qkc->qc', att, x @ wv.T + bv)
    w8, b8 = wb('fc8')
    return pooled @ w8.T + b8


@pytest.mark.parametrize('c', S.LATENT_SIZES)
def test_packed_images_reproduce_the_float64_oracle(c):
    """emulate.poco_head replays the head from PocoDecoderPlan's packed images in float64.  What separates it from the oracle is the
    float32 rounding of the images -- of the composed tail fc8 . fc_value above all (measured: up to 2.1e-7 at outputs up to 5.7) --
    so the bound is 1e-6 * max(1, max|ref|)."""
    worst = 0.0
    for nout in (1, 2, 8):
        for k in (1, 17, 64):
            case = S.build_case('k{}'.format(k), c)                 # the inputs of the case; the parameters are drawn per nout
            sd = S.head_state_dict(c, nout, seed=7 * c + nout)
            plan = PocoDecoderPlan(sd, 'cpu', dtype='f32')
            assert plan.dtype == 'f32' and plan.w16 is None and (plan.c, plan.nout) == (c, nout)
            cb = c // 16
            assert plan.w.shape[0] == 64 * cb + 512 * cb * cb + 1024 * cb and plan.b.shape[0] == 2 * c + 64 and plan.tail.shape[0] == nout * (c + 1)
            got = emulate.poco_head(plan.w.numpy(), plan.b.numpy(), plan.tail.numpy(), plan.g_w.numpy(), plan.g_b.numpy(), c, nout,
                                    case['latents'][0], case['cloud'], case['query'], case['idx'])
            ref = S.oracle(sd, case, torch.float64)
            assert got.shape == ref.shape == (case['q'], nout)
            err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            print('c {} nout {} k {}: max|replay - oracle64| {:.2e}, max|out| {:.2f}'.format(c, nout, k, err, top))
            assert err <= 1e-6 * max(1.0, top)
            worst = max(worst, err)
    assert worst > 0


@pytest.mark.parametrize('c', S.LATENT_SIZES)
def test_f16x3_image_reproduces_the_dense_layers(c):
    """plan.w16 as f16 (hi + lo) gives fc2, fc3 and fc_query back to 2^-21 of the largest weight, in the order the kernel reads them."""
    sd = S.head_state_dict(c, 2, seed=c)
    plan = PocoDecoderPlan(sd, 'cpu', dtype='f16x3')
    assert plan.dtype == 'f16x3'
    img = plan.w16.numpy().view(np.float16).astype(np.float64)
    at = 0
    for name, out in (('fc2', c), ('fc3', c), ('fc_query', 64)):
        w = sd['projection.{}.weight'.format(name)].numpy().reshape(out, c).astype(np.float64)
        part = img[at:at + 2 * out * c].reshape(out // 16, c // 32, 2, 64, 8)
        at += 2 * out * c
        rec = np.zeros((out, c))
        for l in range(64):
            for j in range(8):
                rec[(l & 15)::16, (16 * (j >> 2) + 4 * (l >> 4) + (j & 3))::32] = part[:, :, 0, l, j] + part[:, :, 1, l, j]
        assert np.abs(rec - w).max() <= np.abs(w).max() * 2.0 ** -21, name
        assert np.abs(part[:, :, 1]).max() > 0                       # random weights do have a lo part
    assert at == img.shape[0]


@pytest.mark.parametrize('c', S.LATENT_SIZES)
def test_float64_oracle_equals_plain_numpy(c):
    """The cast of `oracle` reaches every tensor: in float64 it agrees with a restatement in numpy to 1e-12."""
    for name in ('k1', 'k17', 'nout3', 'repeats', 'clamp', 'scale25'):
        case = S.build_case(name, c)
        ref = S.oracle(case['sd'], case, torch.float64)
        assert ref.shape == (case['q'], case['nout'])
        np.testing.assert_allclose(ref, numpy_head(case['sd'], case), rtol=0, atol=1e-12 * max(1.0, float(np.abs(ref).max())))


def test_cases_hold_what_the_kernel_branches_on():
    assert {S.CASES[n][2] for n in S.K_SWEEP} == {1, 2, 15, 16, 17, 31, 33, 48, 49, 63, 64}
    assert {S.CASES[n][3] for n in S.CASES} == {1, 2, 3, 8} and {S.CASES[n][2] for n in S.STRIDE} == {1, 17, 64}
    assert all(S.CASES[n][1] is None for n in S.STRIDE) and S.STRIDE_Q_CPU == 2 * 8 * 256 + 3
    for c in S.LATENT_SIZES:
        for name, (n, q, k, nout, scale, kind) in S.CASES.items():
            if name in S.STRIDE and (c, name) != (32, 'stride_k17'):
                continue                                             # the large cases are built once, for the reference-error test
            case = S.build_case(name, c)
            q = q or S.STRIDE_Q_CPU
            assert case['cloud'].shape == (n, 3) and case['query'].shape == (q, 3) and case['latents'].shape == (1, c, n)
            assert case['idx'].shape == (q, k) and case['idx'].dtype == np.int64 and case['idx'].min() >= 0 and case['idx'].max() < n
            assert case['sd']['projection.fc8.weight'].shape == (nout, c, 1, 1)
            assert all(case[key].dtype == np.float32 for key in ('cloud', 'query', 'latents'))
            assert case is S.build_case(name, c)
        rep = S.build_case('repeats', c)
        assert (rep['idx'] == rep['idx'][:, :1]).all() and np.array_equal(rep['query'], rep['cloud'][rep['idx'][:, 0]])
        assert np.array_equal(np.sort(S.build_case('clamp', c)['idx'], axis=1), np.tile(np.arange(9), (5, 1)))
        assert abs(np.abs(S.build_case('scale25', c)['latents']).max() / np.abs(S.build_case('k64', c)['latents']).max() - 25) < 5
        for name in ('k17', 'k64', 'stride_k17') if c == 32 else ('k17', 'k64'):          # rows left for the containment test to poison
            case = S.build_case(name, c)
            bad = S.poison_unnamed(case['cloud'], case['idx'])
            assert np.isnan(bad).any() and not np.isnan(bad[case['idx']]).any()
            assert np.isnan(S.poison_unnamed(case['latents'][0], case['idx'], axis=1)).all(axis=0).sum() == np.isnan(bad).all(axis=1).sum()
    assert S.build_case('stride_k1', 32, q=19)['q'] == 19


@pytest.mark.parametrize('c', S.LATENT_SIZES)
def test_reference_error_is_finite_and_nonzero(c):
    """E32 per case, printed so that the table in test_gpu_poco_head.py can be checked against it."""
    for name, (n, q, k, nout, scale, kind) in S.CASES.items():
        case = S.build_case(name, c)
        ref, e32 = S.reference_error(case)
        top = float(np.abs(ref).max())
        print('c {} {:10s} q {:4d} k {:2d} nout {}: E32 {:.2e}  max|out| {:.2f}'.format(c, name, case['q'], k, nout, e32, top))
        assert ref.shape == (case['q'], nout) and np.isfinite(ref).all() and top > 0
        assert np.isfinite(e32) and 0 < e32 < 1e-5 * top                # float32 arithmetic, not a different function
        assert S.reference_error(case)[0] is ref                         # cached
        assert S.tolerance(ref, e32, 1) > e32


@pytest.mark.parametrize('q', [50, S.STRIDE_Q_CPU])
@pytest.mark.parametrize('nout', [1, 8])
@pytest.mark.parametrize('c', S.LATENT_SIZES)
def test_integer_case_is_exact_in_float32(c, nout, q):
    case, ref, largest = S.integer_case(c, nout, seed=1, q=q)
    print('c {} nout {} q {}: largest intermediate {}, largest output {}, partial sums below {}'.format(
        c, nout, q, largest, np.abs(ref).max(), case['partial_sum_bound']))
    assert 8 * largest < 2 ** 21 and 8 * largest < 65504          # hi + lo of f16x3 carry it exactly, and the range guard stays down
    assert 8 * case['partial_sum_bound'] * (1 + 2.0 ** -9) < 2 ** 24          # float32 accumulators hold every partial sum, hi and lo parts added in any order
    assert np.array_equal(8 * ref, np.rint(8 * ref)) and np.abs(ref).max() <= case['partial_sum_bound'] and np.abs(ref).max() > 8
    for key in ('cloud', 'query'):
        assert np.array_equal(8 * case[key], np.rint(8 * case[key])) and np.abs(case[key]).max() <= 2
    for name, v in case['sd'].items():
        assert set(np.unique(v.numpy())) <= ({-1.0, 0.0, 1.0} if name.endswith('weight') else {-2.0, -1.0, 0.0, 1.0, 2.0})
    assert case['idx'].shape == (q, 1) and case['idx'].max() < case['n'] // 2
    assert np.array_equal(S.oracle(case['sd'], case, torch.float32), ref)
    assert np.array_equal(S.oracle(case['sd'], case, torch.float64), ref)
    plan = PocoDecoderPlan(case['sd'], 'cpu', dtype='f16x3')          # ternary weights have no lo part
    img = plan.w16.numpy().view(np.float16).reshape(-1, 2, 64, 8)
    assert plan.dtype == 'f16x3' and not img[:, 1].any() and img[:, 0].any()
