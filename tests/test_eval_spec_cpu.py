"""The evaluation specifications themselves (tests/eval_spec.py), checked on the CPU: the fp32 twin of atan2_fast against fp64 arctan2, the
fp32 twin of the winding sweep against winding_spec_bounded at every slice cut, four broken sweeps that the same check must reject, and
reduce_spec on hand-counted inputs."""
import numpy as np
import pytest

import eval_spec as E


def _atan2_sweep():
    """2^21 angles over all four quadrants at magnitudes 1e-9 .. 1e2, the angles where atan2_fast changes branch, and the signed zeros."""
    n = 1 << 21
    rng = np.random.default_rng(0)
    th = np.concatenate([np.linspace(-np.pi, np.pi, n // 2), rng.choice([-1.0, 1.0], n // 2) * rng.uniform(2.3, 2.7, n // 2)])
    mag = 10.0 ** rng.uniform(-9, 2, n)
    y, x = (mag * np.sin(th)).astype(np.float32), (mag * np.cos(th)).astype(np.float32)
    m = np.float32(10.0) ** np.arange(-9, 3, dtype=np.float32)
    z = np.zeros_like(m)
    edge_y = np.concatenate([m, m, -m, -m, z, -z, z, -z, m, -m, m, -m, [0.0, -0.0]]).astype(np.float32)      # |y| = |x|; y = +-0; x = +-0; (0, 0)
    edge_x = np.concatenate([m, -m, m, -m, m, m, -m, -m, z, z, -z, -z, [0.0, 0.0]]).astype(np.float32)
    return np.concatenate([y, edge_y]), np.concatenate([x, edge_x])


def test_atan2_twin_against_arctan2():
    """Measured: max |atan2_fast_twin - arctan2| = 3.26e-7 rad over this sweep (the same over 3.3e7 further random points), at 2.52 rad,
    where float32(pi) - r is rounded at magnitude 2.5 (half an ulp there is 1.19e-7, float32(pi) is off by 8.7e-8).  On [0, 1] alone --
    the polynomial, one quotient, no reflection -- it is 1.34e-7 (6.4e-8 for the polynomial evaluated in fp64).  ATAN2_TWIN_MAX = 3.3e-7
    stands for the measured figure in the winding bound; ATAN2_A adds 2^-23 for the device's reciprocal.
    The twin treats x = -0 as +0 (x < 0 is false), so atan2_fast(+-0, -0) is +-0 where IEEE says +-pi; (det, den) = (0, -0) has h = 0, an
    infinite bound.  The reference here is arctan2(y, x + 0)."""
    y, x = _atan2_sweep()
    assert y.shape[0] >= 1000000
    got = E.atan2_fast_twin(y, x)
    assert got.dtype == np.float32
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64) + 0.0)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(err.max())
    print('max |twin - arctan2| = {:.3e} rad at {:.4f} rad'.format(worst, ref[err.argmax()]))
    assert 3.0e-7 < worst <= E.ATAN2_TWIN_MAX                    # the recorded figure is the measured one, neither stale nor padded
    assert E.ATAN2_A == E.ATAN2_TWIN_MAX + 2.0 ** -23
    assert np.array_equal(np.signbit(got), np.signbit(y))        # the sign of y, for zeros too
    # the polynomial on [0, 1] alone: what "max error" in a header can mean at best
    t = np.linspace(0.0, 1.0, 1000001).astype(np.float32)
    e01 = np.abs(E.atan2_fast_twin(t, np.ones_like(t)).astype(np.float64) - np.arctan(t.astype(np.float64))).max()
    print('on [0, 1]: {:.3e} rad'.format(e01))
    assert 1.2e-7 < e01 < 1.5e-7
    # exact values at the special points
    sp = E.atan2_fast_twin(np.float32([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), np.float32([0.0, 0.0, -1.0, -1.0, 0.0, -0.0]))
    assert sp.tolist() == [0.0, -0.0, np.float32(np.pi), -np.float32(np.pi), np.float32(np.pi / 2), -np.float32(np.pi / 2)]


def test_atan2_mutants_are_wrong_somewhere():
    y, x = [a[:1 << 20] for a in _atan2_sweep()]                 # the half that is uniform in the angle
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64) + 0.0)
    for mutant in ('no_swap', 'half_pi'):
        err = np.abs(E.atan2_fast_twin(y, x, mutant).astype(np.float64) - ref)
        assert err.max() > 0.1 and (err <= E.ATAN2_TWIN_MAX).mean() > 0.4, mutant    # wrong in some octants only: a median does not see it


def _cuts(case):
    m, nf = case['pts'].shape[0], case['faces'].shape[0]
    return sorted({E.sweep_per_slice(m, nf), nf, 1})             # the planner's cut, one slice, nf slices


@pytest.mark.parametrize('name', E.WINDING_CASES)
def test_winding_twin_within_the_bound_at_every_cut(name):
    """The fp32 replay of the kernel lies within the derived bound of the fp64 winding number on every query whose bound is below
    WINDING_CAP, wherever the slices are cut.  Measured max(err / bound): 0.112 (one_face) down to 0.015 (ico320) at the planner's cut --
    the bound is a worst case over ~60 roundings per face, the replay's errors are random."""
    case = E.winding_case(name)
    assert np.isinf(case['bound'][case['planted']]).mean() > 0.9       # the planted queries are what the bound calls undefined
    for per in _cuts(case):
        ratio = E.check_winding(case, E.winding_f32_twin(case['verts'], case['faces'], case['pts'], per))
        print('{}: {} faces per slice, max err / bound {:.4f}'.format(name, per, ratio))
        assert 0.0 < ratio <= 1.0


def test_planner_cuts_are_the_ones_the_cases_are_named_for():
    assert [E.sweep_per_slice(3060, nf) for nf in (1, 63, 64, 65, 313, 320, 500)] == [1, 63, 64, 33, 63, 64, 63]
    assert [-(-nf // E.sweep_per_slice(3060, nf)) for nf in (64, 65, 313, 320)] == [1, 2, 5, 5] and 313 - 4 * 63 == 61
    assert E.sweep_per_slice(20000, 302792) == -(-302792 // 820)   # 20 item blocks: ceil(16384 / 20) = 820 slices


@pytest.mark.parametrize('mutant', ['skip_last_face', 'no_swap', 'half_pi', 'tail_lane'])
@pytest.mark.parametrize('name', ['ico65', 'ico313', 'abc500'])
def test_winding_check_rejects_a_broken_sweep(name, mutant):
    """Each defect touches fewer than half of the queries or moves them by less than the old 1e-3 sign band sees, and is rejected by
    check_winding on a query with a finite bound."""
    case = E.winding_case(name)
    per = E.sweep_per_slice(case['pts'].shape[0], case['faces'].shape[0])
    got = E.winding_f32_twin(case['verts'], case['faces'], case['pts'], per, mutant)
    held = case['bound'] < E.WINDING_CAP
    assert (held & (np.abs(got - case['w']) > case['bound'])).any()
    with pytest.raises(AssertionError, match='beyond their bound'):
        E.check_winding(case, got)


def test_one_missing_face_moves_w_by_more_than_the_bound():
    """The bound is tight enough to see one face: without face 0, 62 or 312 of the open 313-face mesh, w moves by more than the bound on
    at least 95 % of the queries that have one (measured 98.9 % and more).  A face of 3.5e-3 area at distance 0.8 subtends 4.4e-4 cos(t) of
    the sphere against a bound of about 4e-5, so only a query that sees the face edge-on, |cos(t)| < 0.1, cannot tell."""
    case = E.winding_case('ico313')
    held = case['bound'] < E.WINDING_CAP
    for drop in (0, 62, 312):
        w = E.winding_spec(case['verts'], np.delete(case['faces'], drop, axis=0), case['pts'])
        assert (np.abs(w - case['w']) > case['bound'])[held].mean() >= 0.95, drop


def test_winding_spec_bounded_is_winding_spec():
    case = E.winding_case('ico320')
    free = ~case['planted']
    np.testing.assert_allclose(case['w'][free], E.winding_spec(case['verts'], case['faces'], case['pts'])[free], rtol=0, atol=1e-13)
    assert np.abs(case['w'][free] - np.round(case['w'][free])).max() < 1e-12          # a closed mesh: an integer
    assert E.WINDING_K == np.ceil(np.hypot(E.WINDING_K_DET, E.WINDING_K_DEN))


def test_reduce_spec_on_hand_counted_inputs():
    """reduce_spec against counts made by hand: |w| > 0.5 strictly (+-0.5 is outside, -0.7 inside), a NaN cosine neither summed nor
    counted, zero normals give pi / 2, |cosine| > 1 is clamped on both sides."""
    f32 = np.float32
    nr = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1.001], [np.nan, 0, 0]], dtype=f32)
    ng = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 1.001], [0, 0, -1.001]], dtype=f32)
    face_rec = np.array([0, 0, 0, 1, 2, 2, 3], dtype=np.int32)
    face_gt = np.array([4, 3, 2, 1, 0], dtype=np.int32)                       # gt sample j lies on face 4 - j
    nn_rg = np.array([4, 3, 2, 0, 1, 0, 4], dtype=np.int64)                   # -> gt faces 0 1 2 4 3 4 0
    w_rec = np.array([0.7, 0.5, -0.5, -0.7, 0.51, 0.0])
    w_gt = np.array([-0.7, 0.9, 0.6, 0.5, -0.5, 0.2])
    out, bound = E.reduce_spec(f32([4, 0, 0.25, 1, 1, 1, 1]), f32([9, 16]), nn_rg, face_rec, face_gt, nr, ng, w_rec, w_gt)
    assert out[0] == 2 + 0 + 0.5 + 4 and out[1] == 7
    assert out[2:6].tolist() == [1, 2, 2, 1]                                  # TP, FP (rec only), FN (gt only), TN
    assert out[7] == 6 and abs(out[6] - (0 + np.pi + np.pi / 2 + np.pi / 2 + 0 + np.pi)) < 1e-15
    assert (bound[2:6] == 0).all() and bound[7] == 0 and 0 < bound[0] < 1e-14 and bound[6] > 0
    none, _ = E.reduce_spec(None, None, None, None, None, None, None, w_rec, w_gt)
    assert none.tolist() == [0, 0, 1, 2, 2, 1, 0, 0]
    # the crafted inputs of the GPU test reach every special row
    d = E.reduce_inputs(513, 700, 777)
    a = d['normal_rec'].astype(np.float64)[d['face_rec']]
    b = d['normal_gt'].astype(np.float64)[d['face_gt'][d['nn_rg']]]
    cs = (a * b).sum(axis=1)
    assert np.isnan(cs).sum() >= 2 and (cs > 1).any() and (cs < -1).any() and (cs == 0).any()
    out, bound = E.reduce_spec(**d)
    assert out[7] == 513 - np.isnan(cs).sum() and (out[2:6] > 0).all() and out[2:6].sum() == 777
    assert 0 < bound[6] < 1e-2
