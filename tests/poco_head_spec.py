"""Cases and references for the tests of POCO's projection head (interp_small_kernel in csrc/pps_decode.hip, decoder.PocoDecoderPlan).

CPU only (numpy, torch, the oracle).  Two kinds of reference:

* EXACT (`integer_case`): k = 1, ternary weights, integer biases and latents, coordinates on the 1/8 grid.  The softmax over one
  neighbour is exactly 1, so the output is fc8(fc_value(h3)) of small multiples of 1/8, which every float32 summation order (and the
  hi + lo split of 'f16x3') reproduces bit for bit.
* FLOAT64 (`oracle`, `reference_error`): the oracle's interp_attention in float64, with the tolerance taken from the error the SAME
  oracle makes in float32 on the SAME inputs (`tolerance`).
"""
import functools

import numpy as np
import torch

from oracle import ppsurf_oracle as O
from ppsurf_amd.synthetic import make_cloud, make_latents

HEADS = 64
LATENT_SIZES = (32, 64)
STRIDE_Q_CPU = 4099                 # 2 * 8 * 256 + 3: what the GPU test fills in on a 256-CU device


def head_state_dict(c, nout, seed):
    """Random float32 parameters of projection.{fc1,fc2,fc3,fc_query,fc_value,fc8}: N(0, 1.4^2 / fan_in) weights, N(0, 0.1^2) biases."""
    rng = np.random.default_rng(seed)
    shapes = {'fc1': (c, c + 3), 'fc2': (c, c), 'fc3': (c, c), 'fc_query': (HEADS, c), 'fc_value': (c, c), 'fc8': (nout, c)}
    sd = {}
    for name, (o, i) in shapes.items():
        sd['projection.{}.weight'.format(name)] = torch.from_numpy((rng.standard_normal((o, i, 1, 1)) * (1.4 / np.sqrt(i))).astype(np.float32))
        sd['projection.{}.bias'.format(name)] = torch.from_numpy((rng.standard_normal(o) * 0.1).astype(np.float32))
    return sd


# name -> (n, q, k, nout, latent_scale, kind); q None: filled in by the caller (2 * 8 * CU count + 3, so that every workgroup of the
# grid-stride loop runs a second iteration and some a third).  kind 'knn': neighbours from the oracle's kNN; 'repeats': see build_case.
CASES = {}
for _k in (1, 2, 15, 16, 17, 31, 33, 48, 49, 63, 64):          # around the 16 rows of a wave: waves 1..3 masked entirely for k <= 16, 32, 48
    CASES['k{}'.format(_k)] = (3000, 67, _k, 2, 1.0, 'knn')
for _o in (1, 3, 8):
    CASES['nout{}'.format(_o)] = (3000, 67, 17, _o, 1.0, 'knn')
CASES['q1'] = (3000, 1, 64, 2, 1.0, 'knn')
CASES['q2'] = (3000, 2, 64, 2, 1.0, 'knn')
for _k in (1, 17, 64):
    CASES['stride_k{}'.format(_k)] = (3000, None, _k, 2, 1.0, 'knn')
CASES['repeats'] = (3000, 67, 16, 2, 1.0, 'repeats')
CASES['clamp'] = (9, 5, 9, 2, 1.0, 'knn')                       # a cloud of k points: every query names all of them
CASES['scale25'] = (3000, 67, 64, 2, 25.0, 'knn')                # |latent| as the real encoder produces it
K_SWEEP = tuple(n for n in CASES if n[0] == 'k')
STRIDE = tuple(n for n in CASES if n.startswith('stride'))


@functools.lru_cache(maxsize=None)
def build_case(name, c, q=None):
    """Inputs of one case, deterministic in its arguments: sd, cloud [n,3], query [q,3], latents [1,c,n] (float32), idx int64 [q,k].

    Queries are cloud points of the half x < 0 plus a small offset, so the far side of the cloud is named by no neighbour table
    (the containment test poisons those rows).  'repeats': every query IS a cloud point (relative coordinates 0) and its row of idx
    holds that point's id sixteen times."""
    n, q0, k, nout, scale, kind = CASES[name]
    q = q0 if q0 is not None else (STRIDE_Q_CPU if q is None else q)
    seed = 1000 * c + sorted(CASES).index(name)
    rng = np.random.default_rng(seed)
    cloud = make_cloud(n, seed=seed)
    near = np.flatnonzero(cloud[:, 0] < 0)
    sel = near[rng.integers(0, near.shape[0], q)]
    if kind == 'repeats':
        query, idx = cloud[sel].copy(), np.repeat(sel[:, None], k, axis=1).astype(np.int64)
    else:
        query = (cloud[sel] + rng.normal(0, 0.01, (q, 3))).astype(np.float32)
        idx = O.knn_point_major(cloud, query, k)
    lat = make_latents(c, n, seed=seed) * np.float32(scale)
    return dict(name=name, c=c, n=n, q=q, k=k, nout=nout, sd=head_state_dict(c, nout, seed), cloud=cloud, query=query, latents=lat, idx=idx)


def oracle_on(sd, latents, cloud, query, idx, dtype):
    """O.interp_attention with the parameters and every input cast to `dtype` -> point-major [q,nout] float64 numpy."""
    s = {k: v.to(dtype) for k, v in sd.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    out = O.interp_attention(s, 'projection', t(latents), torch.from_numpy(idx).unsqueeze(0), t(cloud.T).unsqueeze(0), t(query.T).unsqueeze(0))
    assert out.dtype == dtype
    return out[0].T.contiguous().to(torch.float64).numpy()


def oracle(sd, case, dtype):
    return oracle_on(sd, case['latents'], case['cloud'], case['query'], case['idx'], dtype)


_errors = {}


def reference_error(case):
    """(ref64, E32) of a build_case: the float64 oracle and the largest deviation from it of the float32 oracle.  Cached per case
    (the 'f32' and 'f16x3' runs share it); callers must not modify ref64."""
    key = (case['name'], case['c'], case['q'])
    if key not in _errors:
        ref = oracle(case['sd'], case, torch.float64)
        _errors[key] = (ref, float(np.abs(oracle(case['sd'], case, torch.float32) - ref).max()))
    return _errors[key]


def tolerance(ref, e32, r):
    """r times the reference's own float32 error, plus one float32 ulp of the largest output."""
    return r * e32 + 2.0 ** -23 * float(np.abs(ref).max())


def poison_unnamed(table, ids, axis=0):
    """A copy of `table` with NaN in EVERY row (axis 0) or column (axis 1) that `ids` does not name (there must be some)."""
    unnamed = np.setdiff1d(np.arange(table.shape[axis]), ids)
    assert unnamed.size > 0
    out = table.copy()
    out[(slice(None),) * axis + (unnamed,)] = np.nan
    return out


# ---------------------------------------------------------------------------------------------------------------------
# exact case
# ---------------------------------------------------------------------------------------------------------------------
def integer_case(c, nout, seed, q=50, n=200):
    """Operands of the exact test at k = 1 and its exact result.

    Weights are ternary {-1, 0, 1} at density 0.5, biases and latents integers in [-2, 2], cloud and query coordinates multiples of
    1/8 in [-2, 2]; idx [q,1] is random.  ReLU layers are positively homogeneous, so the head is evaluated in int64 on coordinates,
    latents and biases scaled by 8 and divided by 8 at the end (exact in float64).

    Returns (case, ref [q,nout] float64, largest): `largest` is the largest magnitude among the operands and the activations of fc1,
    fc2 and fc3, the values the 'f16x3' kernel splits into hi + lo and watches with its range guard (the attention logits, the
    pooled feature and the tail stay in float32); case['partial_sum_bound'] bounds every partial sum of every contraction in ANY
    order (sum of |weight| * |input| + |bias| per layer, the composed tail included), the result with them."""
    rng = np.random.default_rng([c, nout, seed, q])
    shapes = {'fc1': (c, c + 3), 'fc2': (c, c), 'fc3': (c, c), 'fc_query': (HEADS, c), 'fc_value': (c, c), 'fc8': (nout, c)}
    sd, w, b = {}, {}, {}
    for name, (o, i) in shapes.items():
        w[name] = (2 * rng.integers(0, 2, (o, i)) - 1) * (rng.random((o, i)) < 0.5)
        b[name] = rng.integers(-2, 3, o)
        sd['projection.{}.weight'.format(name)] = torch.from_numpy(w[name].astype(np.float32).reshape(o, i, 1, 1))
        sd['projection.{}.bias'.format(name)] = torch.from_numpy(b[name].astype(np.float32))
    cloud8, query8 = rng.integers(-16, 17, (n, 3)), rng.integers(-16, 17, (q, 3))
    lat = rng.integers(-2, 3, (1, c, n))
    idx = rng.integers(0, n // 2, (q, 1))                       # the upper half of the table stays unnamed
    case = dict(name='integer', c=c, n=n, q=q, k=1, nout=nout, sd=sd, cloud=(cloud8 / 8.0).astype(np.float32), query=(query8 / 8.0).astype(np.float32),
                latents=lat.astype(np.float32), idx=idx.astype(np.int64))
    largest, bound = 0, 0

    def layer(name, x, relu=True):
        nonlocal largest, bound
        bound = max(bound, int((np.abs(x) @ np.abs(w[name]).T + 8 * np.abs(b[name])).max()))
        y = x @ w[name].T + 8 * b[name]
        if relu:
            largest = max(largest, int(np.abs(x).max()), int(np.abs(y).max()))
        return np.maximum(y, 0) if relu else y
    x = np.concatenate([8 * lat[0].T[idx[:, 0]], query8 - cloud8[idx[:, 0]]], axis=1)          # [q, c+3], times 8
    h3 = layer('fc3', layer('fc2', layer('fc1', x)))
    layer('fc_query', h3, relu=False)                                                          # softmax over one neighbour: 1
    out = layer('fc8', layer('fc_value', h3, relu=False), relu=False)
    tail_w, tail_b = w['fc8'] @ w['fc_value'], w['fc8'] @ b['fc_value'] + b['fc8']             # what PocoDecoderPlan composes
    assert np.array_equal(out, h3 @ tail_w.T + 8 * tail_b)
    bound = max(bound, int((np.abs(h3) @ np.abs(tail_w).T + 8 * np.abs(tail_b)).max()))
    assert out.dtype == np.int64 and largest <= bound and np.abs(out).max() <= bound
    case['partial_sum_bound'] = bound / 8.0
    return case, out / 8.0, largest / 8.0
