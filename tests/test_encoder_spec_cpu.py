"""The encoder spec itself (tests/encoder_spec.py): its references and case generators, checked on the CPU."""
import numpy as np
import pytest
import torch

import encoder_spec as S
from golden_util import load_golden, filled_sd
from oracle import ppsurf_oracle as O


def all_exact_cases():
    for c1, c2 in S.ROWS_GEMM_CHANNELS + (S.ROWS_GEMM_LONG,):
        yield from S.rows_gemm_cases(c1, c2)
    for m, c1, c2, cout, _ in S.ROWS_GEMM_WIDE:
        yield from S.rows_gemm_wide_cases(m, c1, c2, cout)
    for c1 in S.ROWS_LINEAR_C1:
        for c2 in S.ROWS_LINEAR_C2:
            yield from S.rows_linear_cases(c1, c2)


def test_integer_reference_equals_float64_matmul_and_stays_exact_in_float32():
    worst = 0
    for case in all_exact_cases():
        bound = S.exact_bound(case)
        assert bound < 2 ** 24, (case['m'], case['c1'], case['c2'], case['cout'])
        for name in ('in1', 'in2', 'w', 'bias', 'residual'):
            if case[name] is not None:
                assert case[name].dtype == np.float32 and np.abs(case[name]).max() <= 4 and np.array_equal(case[name], np.rint(case[name]))
        ref = S.linear_reference(case)
        assert ref.dtype == np.int64 and ref.shape == (case['m'], case['cout'])
        assert np.array_equal(ref, S.linear_reference(case, np.float64))
        if case['m'] <= 257:          # a float32 product in the CPU's own summation order gives the same integers
            a32 = S.gathered_operand(case, np.float32) @ case['w'].T
            a64 = S.gathered_operand(case, np.int64) @ case['w'].astype(np.int64).T
            assert np.array_equal(a32, a64)
        assert np.abs(ref).max() <= bound
        worst = max(worst, int(np.abs(ref).max()))
    assert worst > 1000          # the long contraction is in the sweep and does not cancel to nothing


def test_sweeps_hold_what_the_kernels_branch_on():
    for c1, c2 in S.ROWS_GEMM_CHANNELS:
        cases = S.rows_gemm_cases(c1, c2)
        assert {(c['m'], c['cout']) for c in cases} == {(m, o) for m in S.ROWS_GEMM_M for o in S.ROWS_GEMM_COUT}
        assert all(S.rows_gemm_template(c['m'], c['cout']) == 2 for c in cases)
        opts = {c['opts'] for c in cases}
        assert opts == (set(range(32)) if c2 else {o for o in range(32) if not o & S.IDX2})
        if c2:          # the broadcast second operand: one row, every index 0
            assert any(c['idx2'] is not None and c['in2'].shape[0] == 1 and not c['idx2'].any() for c in cases)
        assert any(c['idx1'] is not None and len(set(c['idx1'])) < c['m'] for c in cases)          # repeated gathered rows
    long_cases = S.rows_gemm_cases(*S.ROWS_GEMM_LONG)
    assert {(c['m'], c['cout']) for c in long_cases} == {(17, 33), (17, 64), (70, 33), (70, 64)} and long_cases[0]['c1'] == 8192
    # the arithmetic of launch_rows_gemm for the three shapes around the rows_gemm_kernel<4> threshold
    assert [(m, cout, S.rows_gemm_template(m, cout)) for m, _, _, cout, _ in S.ROWS_GEMM_WIDE] == [(16389, 64, 4), (8133, 128, 4), (16389, 96, 2)]
    assert [nob for *_, nob in S.ROWS_GEMM_WIDE] == [4, 4, 2]
    assert S.rows_gemm_template(16320, 64) == 2 and S.rows_gemm_template(16321, 64) == 4          # gx = 255 | 256
    for c1 in S.ROWS_LINEAR_C1:
        for c2 in S.ROWS_LINEAR_C2:
            assert {(c['m'], c['cout']) for c in S.rows_linear_cases(c1, c2)} == {(m, o) for m in S.ROWS_LINEAR_M for o in S.ROWS_LINEAR_COUT}


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    if torch.is_tensor(a):
        return a.dtype == b.dtype and torch.equal(a, b)
    return a == b


def test_generators_are_deterministic():
    assert same(S.linear_case(65, 32, 80, 33, S.ALL_OPTIONS), S.linear_case(65, 32, 80, 33, S.ALL_OPTIONS))
    assert not same(S.linear_case(65, 32, 80, 33, S.ALL_OPTIONS), S.linear_case(64, 32, 80, 33, S.ALL_OPTIONS))
    for a, b in zip(S.rows_linear_cases(37, 21), S.rows_linear_cases(37, 21)):
        assert same(a, b)
    assert same(S.gather_max_case(77, 9, 37), S.gather_max_case(77, 9, 37))
    for name, (n, m, k, cin, cout) in S.LAYER_CASES.items():
        assert same(S.layer_case(name), S.layer_case(name))
        assert same(S.layer_state_dict(cin, cout, bn='bn'), S.layer_state_dict(cin, cout, bn='bn'))
        c = S.layer_case(name)
        assert c['x'].shape == (n, cin) and c['pts'].shape == (n, 3) and c['sup'].shape == (m, 3) and c['ids'].shape == (m, k)
        assert c['ids'].min() >= 0 and c['ids'].max() < n
    c = S.layer_case('self')
    assert np.array_equal(c['sup'], c['pts']) and np.array_equal(c['ids'][:, 0], np.arange(21))
    assert all(len(set(row)) < 16 for row in S.layer_case('repeats')['ids'])


def test_poison_covers_every_unnamed_row():
    rng = np.random.default_rng(5)
    for m, k in ((1, 1), (17, 16)):
        table = rng.standard_normal((40, 3)).astype(np.float32)
        ids = S.sparse_ids(rng, 40, (m, k))
        named = np.zeros(40, dtype=bool)
        named[ids.reshape(-1)] = True
        assert 0 < named.sum() <= 20
        bad = S.poison_unnamed(table, ids)
        assert np.isnan(bad[~named]).all() and np.array_equal(bad[named], table[named]) and not np.isnan(table).any()
    case = S.linear_case(1, 48, 16, 33, S.ALL_OPTIONS, table_rows=5)
    bad = S.poison_unnamed(case['in1'], case['idx1'])
    assert case['in1'].shape[0] == 5 and np.isnan(bad).all(axis=1).sum() == 4 and not np.isnan(bad[case['idx1'][0]]).any()
    with pytest.raises(AssertionError):
        S.poison_unnamed(table, np.arange(40))


def test_float64_oracle_reproduces_the_layer_fixture():
    g = load_golden('fkaconv_layer')
    t = lambda a: torch.from_numpy(a).to(torch.float64) if a.dtype != np.int64 else torch.from_numpy(a)
    for act in ('relu', 'silu'):
        p = 'L_{}'.format(act)
        sd = S.cast_sd(filled_sd(p + '.'), torch.float64)
        out = O.fkaconv_layer(sd, p, t(g['x']), t(g['pts']), t(g['sup']), t(g['ids']), act)
        assert out.dtype == torch.float64
        np.testing.assert_allclose(out.numpy(), g['out_' + act], rtol=0, atol=1e-4)
        out1 = O.fkaconv_layer(sd, p, t(g['xs']), t(g['sup']), t(g['pts']), t(g['ids1']), act)
        np.testing.assert_allclose(out1.numpy(), g['out_k1_' + act], rtol=0, atol=1e-4)


@pytest.mark.parametrize('name', list(S.LAYER_CASES))
def test_layer_reference_error_is_finite_and_nonzero(name):
    n, m, k, cin, cout = S.LAYER_CASES[name]
    cases = S.layer_draws(name)
    assert len(cases) == (16 if name == 'single' else 1) and not any(same(cases[0], c) for c in cases[1:])
    for act in ('relu', 'silu'):
        sd = S.layer_state_dict(cin, cout)
        ref, e32 = S.reference_error(lambda dt: S.oracle_layer_draws(sd, 'L', cases, act, dt))
        assert ref.shape == (len(cases) * m, cout) and np.isfinite(ref).all() and np.abs(ref).max() > 0
        assert np.isfinite(e32) and e32 > 0
        assert e32 < 1e-5 * np.abs(ref).max()          # float32 arithmetic, not a different function
        assert S.tolerance(ref, e32, 1) > 2.0 ** -23 * np.abs(ref).max()


def test_folded_batchnorm_reference():
    n, m, k, cin, cout = S.LAYER_CASES['m17_k15']
    sd, case = S.layer_state_dict(cin, cout, bn='bn'), S.layer_case('m17_k15')
    ref, e32 = S.reference_error(lambda dt: S.oracle_layer(sd, 'L', case, 'silu', dt, bn='bn'))
    assert np.isfinite(e32) and e32 > 0 and ref.min() == 0 and ref.max() > 0
    s64 = S.cast_sd(sd, torch.float64)
    plain = O.fkaconv_layer(s64, 'L', *(S.channel_first(case[k], torch.float64) for k in ('x', 'pts', 'sup')), torch.from_numpy(case['ids']).unsqueeze(0), 'silu')
    bn = torch.nn.functional.batch_norm(plain, s64['bn.running_mean'], s64['bn.running_var'], s64['bn.weight'], s64['bn.bias'], False, 0.0, 1e-5)
    np.testing.assert_allclose(ref, S.point_major(torch.relu(bn)), rtol=0, atol=1e-12)


def test_ragged_cloud_levels_and_reference_error():
    d = S.ragged_cloud()
    assert tuple(d[k].shape[2] for k in ('pts', 'support1', 'support2', 'support3', 'support4')) == S.RAGGED_LEVELS
    # kNN clamps k to the number of source points (oracle and product alike), never to the number of supports
    assert [d[k].shape[1:] for k in ('ids00', 'ids01', 'ids22', 'ids23', 'ids33', 'ids34', 'ids44')] == \
        [(333, 16), (83, 16), (20, 16), (5, 16), (5, 5), (1, 5), (1, 1)]
    assert d['ids10'].shape == (1, 333, 1) and d['ids43'].shape == (1, 5, 1)
    for key, down in (('RB_same', False), ('RB_down', True)):
        sd = filled_sd(key + '.')
        ref, e32 = S.reference_error(lambda dt: S.oracle_block(sd, key, down, 'silu', dt))
        assert ref.shape == ((83, 32) if down else (333, 16)) and np.isfinite(e32) and 0 < e32 < 1e-5 * np.abs(ref).max()
    for key, act, fixed in (('ENC_silu_fixed', 'silu', True), ('ENC_relu_poco', 'relu', False)):
        sd = filled_sd(key + '.')
        ref, e32 = S.reference_error(lambda dt: S.oracle_network(sd, key, act, fixed, dt))
        assert ref.shape[0] == 333 and np.isfinite(e32) and 0 < e32 < 1e-4 * np.abs(ref).max()
