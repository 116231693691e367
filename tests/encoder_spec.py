"""Cases and references for the shape-swept tests of the inference encoder kernels (csrc/pps_fkaconv.hip).

CPU only (numpy, torch, the oracle).  Two kinds of reference:

* EXACT: rows_gemm / rows_linear on small integers.  Inputs, weights, bias and residual are integers in [-4, 4] stored as float32, so
  every partial sum of a contraction of length K is an integer of magnitude <= 16 K + 8 < 2^24 and every float32 summation order gives
  the int64 result bit for bit (`exact_bound`).
* FLOAT64: the oracle's FKAConv layer / residual block / network evaluated in float64, with the tolerance taken from the error the
  SAME oracle makes in float32 on the SAME inputs (`reference_error`, `tolerance`).
"""
import itertools

import numpy as np
import torch

from oracle import ppsurf_oracle as O

# ---------------------------------------------------------------------------------------------------------------------
# exact cases: out = relu?( [in1[idx1] | in2[idx2]] @ W.T + bias + residual )
# ---------------------------------------------------------------------------------------------------------------------
IDX1, IDX2, BIAS, RES, RELU = 1, 2, 4, 8, 16          # option bits of a case
ALL_OPTIONS = IDX1 | IDX2 | BIAS | RES | RELU


def ints(rng, shape):
    return rng.integers(-4, 5, shape).astype(np.float32)


def rows_gemm_template(m, cout):
    """NOB of the rows_gemm_kernel<NOB> that launch_rows_gemm picks for m rows and cout outputs (restated from pps_fkaconv.hip)."""
    obt = ((cout + 31) // 32) * 2          # 16-wide output blocks of the packed weight image (outputs padded to 32)
    gx = (m + 63) // 64                    # row tiles
    return 4 if gx * (obt // 4) >= 256 and obt % 4 == 0 else 2


def linear_case(m, c1, c2, cout, opts, zero_idx2=False, table_rows=None):
    """One integer-valued case; deterministic in its arguments.  Gathers draw from tables with fewer rows than m has (repeated rows),
    or with table_rows rows (rows that no index names); zero_idx2: in2 is one row that every output row reads (the cv5 broadcast of
    EncoderPlan.forward)."""
    if c2 == 0:
        opts &= ~IDX2
    rng = np.random.default_rng([m, c1, c2, cout, opts, int(zero_idx2)])
    case = dict(m=m, c1=c1, c2=c2, cout=cout, opts=opts, idx1=None, in2=None, idx2=None, bias=None, residual=None, relu=bool(opts & RELU))
    if opts & IDX1:
        n1 = table_rows or m // 2 + 2
        case['in1'], case['idx1'] = ints(rng, (n1, c1)), rng.integers(0, n1, m)
    else:
        case['in1'] = ints(rng, (m, c1))
    if c2:
        if opts & IDX2:
            n2 = 1 if zero_idx2 else table_rows or m // 3 + 2
            case['in2'], case['idx2'] = ints(rng, (n2, c2)), rng.integers(0, n2, m)
        else:
            case['in2'] = ints(rng, (m, c2))
    case['w'] = ints(rng, (cout, c1 + c2))
    if opts & BIAS:
        case['bias'] = ints(rng, (cout,))
    if opts & RES:
        case['residual'] = ints(rng, (m, cout))
    return case


def poison_unnamed(table, ids):
    """A copy of `table` with NaN in EVERY row that `ids` does not name (there must be some)."""
    unnamed = np.setdiff1d(np.arange(table.shape[0]), ids)
    assert unnamed.size > 0
    out = table.copy()
    out[unnamed] = np.nan
    return out


def sparse_ids(rng, n, shape):
    """ids of `shape` into a random half of the n rows of a table, so that many rows stay unnamed however many ids are drawn."""
    rows = rng.choice(n, max(1, n // 2), replace=False)
    return rows[rng.integers(0, rows.shape[0], shape)]


def exact_bound(case):
    """Largest magnitude any partial sum of the case can reach, in whatever order it is added up."""
    return 16 * (case['c1'] + case['c2']) + 4 + 4


def gathered_operand(case, dtype):
    a = case['in1'][case['idx1']] if case['idx1'] is not None else case['in1']
    if case['in2'] is not None:
        a = np.concatenate([a, case['in2'][case['idx2']] if case['idx2'] is not None else case['in2']], axis=1)
    assert a.shape == (case['m'], case['c1'] + case['c2'])
    return a.astype(dtype)


def linear_reference(case, dtype=np.int64):
    out = gathered_operand(case, dtype) @ case['w'].astype(dtype).T
    if case['bias'] is not None:
        out = out + case['bias'].astype(dtype)
    if case['residual'] is not None:
        out = out + case['residual'].astype(dtype)
    return np.maximum(out, 0) if case['relu'] else out


ROWS_GEMM_M = (1, 15, 16, 17, 63, 64, 65, 257)
ROWS_GEMM_COUT = (1, 16, 31, 32, 33, 64, 96, 128)
ROWS_GEMM_CHANNELS = ((16, 0), (48, 0), (16, 16), (32, 80))
ROWS_GEMM_LONG = (8192, 0)                               # the K = 8192 contraction of resnetb41.cv1 (Cin = 512)
ROWS_GEMM_LONG_M, ROWS_GEMM_LONG_COUT = (17, 70), (33, 64)
# (m, c1, c2, cout, NOB): the shapes at which launch_rows_gemm leaves the default rows_gemm_kernel<2> -- or just does not
ROWS_GEMM_WIDE = (
    (16389, 16, 0, 64, 4),      # gx = ceil(16389/64) = 257, obt = 2*ceil(64/32) = 4: 257 * (4/4) = 257 >= 256 and 4 % 4 == 0 -> <4>
    (8133, 16, 16, 128, 4),     # gx = ceil(8133/64) = 128, obt = 8: 128 * (8/4) = 256 >= 256 and 8 % 4 == 0 -> <4>, blockIdx.y in {0, 1}
    (16389, 16, 0, 96, 2),      # gx = 257, obt = 6: 257 * (6/4 = 1) >= 256 but 6 % 4 != 0 -> stays on <2>
)

ROWS_LINEAR_C1, ROWS_LINEAR_C2 = (1, 3, 37), (0, 21)
ROWS_LINEAR_COUT = (1, 45, 64, 65)
ROWS_LINEAR_M = (1, 31, 32, 33, 500)

GATHER_MAX_M, GATHER_MAX_K, GATHER_MAX_C = (1, 77, 257), (1, 9, 16, 300), (1, 37, 256)


def rows_gemm_cases(c1, c2):
    """Every (M, Cout) of the sweep at one channel pair, four option sets each; over one pair all 32 option sets occur."""
    if (c1, c2) == ROWS_GEMM_LONG:
        return [linear_case(m, c1, c2, cout, opts) for m in ROWS_GEMM_LONG_M for cout in ROWS_GEMM_LONG_COUT
                for opts in (0, IDX1 | BIAS | RES | RELU)]
    p = ROWS_GEMM_CHANNELS.index((c1, c2))
    cases = []
    for i, (m, cout) in enumerate(itertools.product(ROWS_GEMM_M, ROWS_GEMM_COUT)):
        for opts in sorted({(5 * i + 13 * j + 3 * p) % 32 & (ALL_OPTIONS if c2 else ~IDX2) for j in range(4)}):
            cases.append(linear_case(m, c1, c2, cout, opts, zero_idx2=bool(opts & IDX2) and i % 3 == 0))
    return cases


def rows_gemm_wide_cases(m, c1, c2, cout):
    return [linear_case(m, c1, c2, cout, 0), linear_case(m, c1, c2, cout, ALL_OPTIONS)]


def rows_linear_cases(c1, c2):
    cases = []
    for i, (m, cout) in enumerate(itertools.product(ROWS_LINEAR_M, ROWS_LINEAR_COUT)):
        for opts in sorted({(7 * i + 11 * j + 5 * c1) % 32 & (ALL_OPTIONS if c2 else ~IDX2) for j in range(3)}):
            cases.append(linear_case(m, c1, c2, cout, opts, zero_idx2=bool(opts & IDX2) and i % 3 == 0))
    return cases


def gather_max_case(m, k, c, n=61):
    rng = np.random.default_rng([m, k, c])
    return rng.standard_normal((n, c)).astype(np.float32), rng.integers(0, n, (m, k))


# ---------------------------------------------------------------------------------------------------------------------
# the FKAConv layer against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
# name -> (n, m, k, cin, cout)
LAYER_CASES = {
    'single': (1, 1, 1, 1, 1),
    'm1_k7': (9, 1, 7, 3, 8),
    'm15_k2': (40, 15, 2, 16, 31),
    'm16_k16': (40, 16, 16, 16, 32),
    'm17_k15': (40, 17, 15, 24, 33),
    'm257_cin40': (300, 257, 16, 40, 96),
    'cin512': (64, 33, 16, 512, 64),
    'repeats': (5, 3, 16, 16, 16),          # 16 neighbours out of 5 points: every neighbourhood repeats points
    'self': (21, 21, 6, 5, 7),              # sup == pts, ids[m, 0] == m: a neighbour at distance 0
}
# 'single' has ONE output, so the E32 of one draw is one sample of a rounding error (0.0004 to 16 ulp of the output over the first
# draws) instead of the maximum over many outputs.  The case is therefore 16 draws of its inputs, run one by one and judged together:
# error, E32 and the largest output are maxima over all draws, as they are over the rows of every other case.
LAYER_DRAWS = {'single': 16}


def layer_state_dict(cin, cout, p='L', bn=None, seed=0):
    """Random FKAConvLayer parameters {p.name: float32 tensor}; bn: name of a BatchNorm1d (running statistics) that follows the layer."""
    rng = np.random.default_rng([cin, cout, seed])
    nrm = rng.standard_normal
    sd = {
        p + '.cv.weight': nrm((cout, cin, 1, 16)) / np.sqrt(16 * cin),
        p + '.fc1.weight': nrm((16, 3, 1, 1)),
        p + '.fc2.weight': nrm((16, 32, 1, 1)) / 4,
        p + '.fc3.weight': nrm((16, 32, 1, 1)) / 4,
        p + '.bn1.weight': rng.uniform(0.5, 1.5, 16), p + '.bn1.bias': 0.3 * nrm(16),
        p + '.bn2.weight': rng.uniform(0.5, 1.5, 16), p + '.bn2.bias': 0.3 * nrm(16),
        p + '.norm_radius': np.array([0.3]), p + '.alpha': np.array([1.3]), p + '.beta': np.array([0.7]),
    }
    if bn is not None:
        sd.update({bn + '.weight': rng.uniform(0.5, 1.5, cout), bn + '.bias': 0.3 * nrm(cout),
                   bn + '.running_mean': 0.3 * nrm(cout), bn + '.running_var': rng.uniform(0.5, 1.5, cout)})
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}


def layer_case(name, draw=0):
    """Point-major float32 inputs of a layer case: x [n,cin], pts [n,3], sup [m,3], ids int64 [m,k] (random, so neighbours repeat)."""
    n, m, k, cin, cout = LAYER_CASES[name]
    rng = np.random.default_rng([n, m, k, cin, cout] + ([draw] if draw else []))
    pts = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    ids = rng.integers(0, n, (m, k))
    if name == 'self':
        sup = pts.copy()
        ids[:, 0] = np.arange(m)
    else:
        sup = rng.uniform(-0.5, 0.5, (m, 3)).astype(np.float32)
    return dict(x=rng.standard_normal((n, cin)).astype(np.float32), pts=pts, sup=sup, ids=ids)


def layer_draws(name):
    return [layer_case(name, d) for d in range(LAYER_DRAWS.get(name, 1))]


def cast_sd(sd, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def channel_first(a, dtype):
    """[N,C] numpy -> [1,C,N] tensor, the oracle's layout."""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(dtype).unsqueeze(0)


def point_major(t):
    """[1,C,N] tensor -> [N,C] float64 numpy."""
    return t[0].T.contiguous().to(torch.float64).numpy()


def oracle_layer(sd, p, case, act, dtype, bn=None):
    """The oracle's layer (+ BatchNorm and ReLU as ResidualBlock applies them, if bn) in `dtype` -> [m,cout] float64."""
    s = cast_sd(sd, dtype)
    out = O.fkaconv_layer(s, p, channel_first(case['x'], dtype), channel_first(case['pts'], dtype), channel_first(case['sup'], dtype),
                          torch.from_numpy(case['ids']).unsqueeze(0), act)
    if bn is not None:
        scale = s[bn + '.weight'] / torch.sqrt(s[bn + '.running_var'] + O.BN_EPS)
        out = torch.relu((out - s[bn + '.running_mean'].view(1, -1, 1)) * scale.view(1, -1, 1) + s[bn + '.bias'].view(1, -1, 1))
    return point_major(out)


def oracle_layer_draws(sd, p, cases, act, dtype, bn=None):
    """The draws of a case stacked along the rows."""
    return np.concatenate([oracle_layer(sd, p, c, act, dtype, bn) for c in cases], axis=0)


def reference_error(fn):
    """(reference, E32): fn(torch.float64) and the largest deviation from it of fn(torch.float32), the same arithmetic in the
    precision the kernels store their results in."""
    ref = fn(torch.float64)
    e32 = float(np.abs(fn(torch.float32) - ref).max())
    return ref, e32


def tolerance(ref, e32, r):
    """r times the reference's own float32 error, plus one float32 ulp of the largest output."""
    return r * e32 + 2.0 ** -23 * float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# residual block and network on one cloud whose level sizes are all off the tile sizes
# ---------------------------------------------------------------------------------------------------------------------
RAGGED_LEVELS = (333, 83, 20, 5, 1)

_ragged = None


def ragged_cloud():
    """The oracle's `data` dict (float32, [1,3,n] layout, 13 id tables) of a 333-point cloud with nested random support levels.
    The id tables come from the oracle's kNN, which clamps k to the number of SOURCE points: ids33 and ids34 have K = 5, ids44 K = 1."""
    global _ragged
    if _ragged is None:
        rng = np.random.default_rng(333)
        pts = rng.uniform(-0.5, 0.5, (RAGGED_LEVELS[0], 3)).astype(np.float32)
        order = rng.permutation(RAGGED_LEVELS[0])
        cf = lambda a: channel_first(a, torch.float32)
        data = O.fkaconv_ids_from_supports(cf(pts), [cf(pts[order[:n]]) for n in RAGGED_LEVELS[1:]])
        data['pts'] = cf(pts)
        data['x16'] = cf(rng.standard_normal((RAGGED_LEVELS[0], 16)).astype(np.float32))       # input of the residual-block cases
        _ragged = data
    return _ragged


def cast_data(data, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in data.items()}


def oracle_block(sd, p, down, act, dtype):
    d = cast_data(ragged_cloud(), dtype)
    sup, ids = (d['support1'], d['ids01']) if down else (d['pts'], d['ids00'])
    return point_major(O.residual_block(cast_sd(sd, dtype), p, d['x16'], d['pts'], sup, ids, act))


def oracle_network(sd, p, act, fixed, dtype):
    return point_major(O.fkaconv_network(cast_sd(sd, dtype), p, cast_data(ragged_cloud(), dtype), act, fixed))
