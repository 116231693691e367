"""numpy restatements of the evaluation kernels (ppsurf_amd/csrc/pps_eval.hip) and meshes with known answers, for the tests."""
import numpy as np

_GAMMA, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix64(x):
    """splitmix64 finaliser of x + golden gamma, uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        z = np.asarray(x, dtype=np.uint64) + _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def sample_spec(corners, prefix, n, seed, stream_id):
    """The sampler of the header comment of pps_eval.hip (generator: pps_rng.h): (points f32 [n,3], face ids int64 [n]) from corners
    f32 [nf,9] and the fp64 inclusive area prefix."""
    corners = np.asarray(corners, dtype=np.float32)
    prefix = np.asarray(prefix, dtype=np.float64)
    key = mix64(mix64(np.uint64(seed)) ^ np.uint64(stream_id))
    ctr = np.arange(n, dtype=np.uint64) << np.uint64(2)
    u = (mix64(key ^ ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r1 = (mix64(key ^ (ctr | np.uint64(1))) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    r2 = (mix64(key ^ (ctr | np.uint64(2))) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    total = prefix[-1]
    face = np.searchsorted(prefix, u * total, side='right')
    face = np.where(face == prefix.shape[0], np.searchsorted(prefix, total, side='left'), face)
    fold = (r1 + r2) > np.float32(1.0)
    r1 = np.where(fold, np.float32(1.0) - r1, r1).astype(np.float32)
    r2 = np.where(fold, np.float32(1.0) - r2, r2).astype(np.float32)
    c = corners[face]
    v0, e1, e2 = c[:, 0:3], c[:, 3:6] - c[:, 0:3], c[:, 6:9] - c[:, 0:3]
    pts = (r1[:, None] * e1 + r2[:, None] * e2) + v0
    return pts.astype(np.float32), face


def face_stats_spec(verts, faces):
    """(area [nf], unit normal [nf,3], corners [nf,9]) in fp64."""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(cr, axis=1)
    normal = np.where(ln[:, None] > 0, cr / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    return 0.5 * ln, normal, v.reshape(-1, 9)


def winding_spec(verts, faces, pts, chunk=64):
    """Generalised winding number in fp64 by brute force: sum_f 2 atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi."""
    tri = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    pts = np.asarray(pts, dtype=np.float64)
    out = np.empty(pts.shape[0])
    for s in range(0, pts.shape[0], chunk):
        p = pts[s:s + chunk, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        la, lb, lc = [np.linalg.norm(x, axis=2) for x in (a, b, c)]
        det = np.einsum('qfi,qfi->qf', a, np.cross(b, c))
        den = la * lb * lc + np.einsum('qfi,qfi->qf', a, b) * lc + np.einsum('qfi,qfi->qf', b, c) * la + np.einsum('qfi,qfi->qf', c, a) * lb
        out[s:s + chunk] = np.arctan2(det, den).sum(axis=1) / (2.0 * np.pi)
    return out


# ---- the winding number with its own error bound ---------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24                                            # unit roundoff of fp32
WINDING_K_DET, WINDING_K_DEN = 8.0, 53.0                      # roundings of det and den in units of EPS32 * |a||b||c| (winding_spec_bounded)
WINDING_K = 54.0                                              # ceil(hypot(8, 53) = 53.6): the radius of the error disc of (det, den)
ATAN2_TWIN_MAX = 3.3e-7                                       # largest |atan2_fast_twin - arctan2| in fp64 (measured: test_eval_spec_cpu.py)
ATAN2_A = ATAN2_TWIN_MAX + 2.0 ** -23                         # + the device's 1-ulp v_rcp_f32: t off by <= 2^-22 relative, t atan'(t) <= 1/2
WINDING_CAP = 2e-4                                            # a query is held to its bound where the bound is below this

SWEEP_TILE, SWEEP_BLOCK, SWEEP_MIN_SLICE, SWEEP_TARGET_BLOCKS = 1024, 256, 64, 16384     # keep in step with pps_sweep.h


def sweep_per_slice(m, nf):
    """Faces per slice of the planner (sweep_slices and sweep_launch of pps_sweep.h) for m items and nf faces."""
    blocks = (m + SWEEP_TILE - 1) // SWEEP_TILE
    s = min((SWEEP_TARGET_BLOCKS + blocks - 1) // blocks, (nf + SWEEP_MIN_SLICE - 1) // SWEEP_MIN_SLICE)
    per = (nf + s - 1) // s
    slices = (nf + per - 1) // per
    return (nf + slices - 1) // slices


def winding_spec_bounded(verts, faces, pts, chunk=128):
    """(w, bound), both fp64 [m]: winding_spec of the fp32-rounded inputs, and a bound on |w_kernel - w| for the fp32 sweep of
    pps_eval.hip (WindingOp, atan2_fast, winding_sum_kernel).  The bound is counted from the kernel's operations, never fitted to its output.

    Per face the kernel computes (det, den) in fp32 and takes atan2_fast of them.  With u = EPS32, M = |a||b||c|, h = hypot(det, den) and
    first-order rounding analysis (every (1 + d) has |d| <= u; products of a component each of a, b and c sum to at most M by Cauchy-Schwarz):
      inputs   a = corner - query is rounded per component, so each of a, b, c moves by <= u times its length.  det is trilinear:
               <= 3 u M.  Each of the four terms of den is 1-Lipschitz in each vector up to the other two lengths: <= 4 * 3 u M = 12 u M.
      det      fma(ax, X, fma(ay, Y, az * Z)) with X = fma(by, cz, -(bz * cy)) etc: the rounded products bz*cy, bx*cz, by*cx times their a
               component sum to <= u M; the three fma roundings of X, Y, Z (u |X| each) to <= u |a||b x c| <= u M; az * Z, the inner fma and
               the outer fma one u M each: 5 u M.                                                         K_det = 3 + 5 = 8
      lengths  sum of three squares by two fmas and a product, all terms positive: 3 u relative, halved by the root: 1.5 u; the bare
               v_sqrt_f32 is good to 1 ulp <= 2 u: 3.5 u per length.
      dots     fma(ax, bx, fma(ay, by, az * bz)): 3 u sum|a_i b_i| <= 3 u |a||b|.
      den      fma(la * lb, lc, fma(ab, lc, fma(bc, la, ca * lb))): la lb lc carries 3 * 3.5 u + u (the product la * lb) = 11.5 u M;
               ca * lb carries 3 + 3.5 + 1 (its product) = 7.5 u M; bc * la and ab * lc sit inside fmas: 6.5 u M each; the three fma
               roundings act on partial sums of two, three and four terms: (2 + 3 + 4) u M.
                                                                                    K_den = 12 + 11.5 + 7.5 + 6.5 + 6.5 + 9 = 53
    The computed v' = (det', den') lies within (K_det, K_den) u M of the exact v = (det, den), so in a disc of radius rho = K u M,
    K = ceil(hypot(K_det, K_den)) = 54 (the ceiling covers the second-order terms, < 54^2 u relative).  The angle between v and v' has
    sine |v x v'| / (|v||v'|) <= (|den| K_det + |det| K_den) u M / (h (h - rho)), so
      face bound = asin((|den| K_det + |det| K_den) u M / (h (h - rho))) + A,      A = ATAN2_A, the absolute error of atan2_fast itself.
    (u there times 1 + 2^-16, which covers the second-order terms of K_det and K_den, < 54 u relative each).
    By Cauchy-Schwarz the first term is at most K u M / (h - rho), the disc's angle; it is smaller where |det| << |den|, as for every face
    far from the query, because an error of den along v does not turn v.  The bound is infinite where the angle is not defined to that
    accuracy: the disc reaches the origin (K u M >= h; h == 0 for a query on a corner) or the branch cut of atan2 (den < 0 and
    |det| <= K u M: a query in a face's plane inside the face or on an edge).

    Per query: the sum of the face bounds, plus nf * u * sum(|angle| + face bound) for the fp32 accumulation in face order (n additions of
    terms x_i lose at most (n - 1) u sum|x_i| however they are grouped into slices, so this holds for any slice cut; the fp64 sum over the
    slices and the final product add ~1e-16), all divided by 2 pi."""
    tri = np.asarray(verts, dtype=np.float32).astype(np.float64)[np.asarray(faces)]
    pts = np.asarray(pts, dtype=np.float32).astype(np.float64)
    nf = tri.shape[0]
    w, bound = np.empty(pts.shape[0]), np.empty(pts.shape[0])
    for s in range(0, pts.shape[0], chunk):
        p = pts[s:s + chunk, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        la, lb, lc = [np.sqrt((x * x).sum(axis=2)) for x in (a, b, c)]
        det = (a * np.cross(b, c)).sum(axis=2)
        den = la * lb * lc + (a * b).sum(axis=2) * lc + (b * c).sum(axis=2) * la + (c * a).sum(axis=2) * lb
        ang = np.arctan2(det, den)
        rho, h = WINDING_K * EPS32 * (la * lb * lc), np.hypot(det, den)
        undefined = (rho >= h) | ((den < 0) & (np.abs(det) <= rho))
        cross = (np.abs(den) * WINDING_K_DET + np.abs(det) * WINDING_K_DEN) * (EPS32 * (1.0 + 2.0 ** -16)) * (la * lb * lc)
        with np.errstate(divide='ignore', invalid='ignore'):
            sin = np.where(undefined, 1.0, cross / np.where(undefined, 1.0, h * (h - rho)))
            fb = np.where(undefined | (sin >= 1.0), np.inf, np.arcsin(np.minimum(sin, 1.0)) + ATAN2_A)
        tot = fb.sum(axis=1)
        w[s:s + chunk] = ang.sum(axis=1) / (2.0 * np.pi)
        bound[s:s + chunk] = (tot + nf * EPS32 * (np.abs(ang).sum(axis=1) + tot)) / (2.0 * np.pi)
    return w, bound


def _fma32(a, b, c):
    """fmaf of fp32 arrays: the product is exact in fp64, the sum is rounded to fp64 and then to fp32 (a double rounding at most)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


# keep in step with pps_eval.hip (atan2_fast)
_ATAN_COEF = [np.float32(x) for x in (-0.004054495599120855, 0.02186269313097, -0.05591193586587906, 0.09642168134450912, -0.13908617198467255,
                                      0.19946563243865967, -0.33329859375953674, 0.9999993443489075)]


def atan2_fast_twin(y, x, mutant=None):
    """atan2_fast of pps_eval.hip in numpy fp32: the degree-15 odd polynomial on [0, 1] by Horner with fmaf, and the three reflections
    (swap, x < 0, sign of y).  The reciprocal is numpy's correctly rounded 1 / x where the device has the 1-ulp v_rcp_f32 (ATAN2_A).
    mutant 'no_swap' leaves the swap reflection out, 'half_pi' reflects x < 0 with pi / 2 in place of pi."""
    y, x = np.asarray(y, dtype=np.float32), np.asarray(x, dtype=np.float32)
    ax, ay = np.abs(x), np.abs(y)
    swap = ay > ax
    mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
    with np.errstate(over='ignore', under='ignore'):
        t = mn * (np.float32(1.0) / (mx + np.float32(1e-30)))
        s = t * t
        p = _ATAN_COEF[0]
        for coef in _ATAN_COEF[1:]:
            p = _fma32(p, s, coef)
        r = t * p
    if mutant != 'no_swap':
        r = np.where(swap, np.float32(1.5707963267948966) - r, r)
    r = np.where(x < 0, np.float32(1.5707963267948966 if mutant == 'half_pi' else 3.141592653589793) - r, r)
    return np.copysign(r, y).astype(np.float32)


def winding_f32_twin(verts, faces, pts, per_slice, mutant=None):
    """WindingOp and winding_sum_kernel of pps_eval.hip replayed in numpy fp32 (fmaf as _fma32, numpy's correctly rounded sqrt for
    v_sqrt_f32): fp32 partial sums per slice of `per_slice` faces in face order, fp64 sum over the slices in slice order, / 2 pi -> fp64 [m].
    Mutants, each a defect a median over the queries lets through: 'skip_last_face' (a slice stops one face early), 'no_swap' and 'half_pi'
    (atan2_fast_twin), 'tail_lane' (the items of the last, partly filled row of SWEEP_BLOCK lanes all carry item m - 1)."""
    f32 = np.float32
    tri = np.asarray(verts, dtype=f32)[np.asarray(faces)]
    q = np.asarray(pts, dtype=f32)
    m, nf = q.shape[0], tri.shape[0]
    if mutant == 'tail_lane' and m % SWEEP_BLOCK:
        q = q.copy()
        q[m - m % SWEEP_BLOCK:] = q[m - 1]
    px, py, pz = q[:, 0], q[:, 1], q[:, 2]
    total = np.zeros(m, dtype=np.float64)
    for f0 in range(0, nf, per_slice):
        f1 = min(f0 + per_slice, nf)
        acc = np.zeros(m, dtype=f32)
        for f in range(f0, f1 - 1 if mutant == 'skip_last_face' else f1):
            c = tri[f].reshape(9)
            ax, ay, az = c[0] - px, c[1] - py, c[2] - pz
            bx, by, bz = c[3] - px, c[4] - py, c[5] - pz
            cx, cy, cz = c[6] - px, c[7] - py, c[8] - pz
            la = np.sqrt(_fma32(ax, ax, _fma32(ay, ay, az * az)))
            lb = np.sqrt(_fma32(bx, bx, _fma32(by, by, bz * bz)))
            lc = np.sqrt(_fma32(cx, cx, _fma32(cy, cy, cz * cz)))
            det = _fma32(ax, _fma32(by, cz, -bz * cy), _fma32(ay, _fma32(bz, cx, -bx * cz), az * _fma32(bx, cy, -by * cx)))
            ab = _fma32(ax, bx, _fma32(ay, by, az * bz))
            bc = _fma32(bx, cx, _fma32(by, cy, bz * cz))
            ca = _fma32(cx, ax, _fma32(cy, ay, cz * az))
            den = _fma32(la * lb, lc, _fma32(ab, lc, _fma32(bc, la, ca * lb)))
            acc = acc + atan2_fast_twin(det, den, mutant)
        total += acc.astype(np.float64)
    return total * (1.0 / (2.0 * 3.141592653589793))


# ---- queries for the winding tests -----------------------------------------------------------------------------------------------------------------
def winding_queries(verts, faces, m, seed, extent=0.5, sphere=False):
    """m query points f32 [m,3]: a third (for m > 1) within +-0.02 of the surface -- a uniform point of a random face, moved along the face
    normal -- the rest uniform in the cube of half side `extent`.  The first k rows do not depend on m."""
    rng = np.random.default_rng(seed)
    mm = max(m, 3)
    tri = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    pts = (rng.random((mm, 3)) - 0.5) * 2.0 * extent
    face = rng.integers(0, tri.shape[0], mm)
    r = rng.random((mm, 2))
    off = rng.uniform(-0.02, 0.02, mm)
    fold = r.sum(axis=1) > 1.0
    r[fold] = 1.0 - r[fold]
    t = tri[face]
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    near = t[:, 0] + r[:, :1] * e1 + r[:, 1:] * e2 + off[:, None] * nrm
    pick = np.arange(mm) % 3 == 2
    pts[pick] = near[pick]
    if sphere:                                                # another third on a sphere around the mesh
        d = rng.standard_normal((mm, 3))
        ring = tri.reshape(-1, 3).mean(axis=0) + 0.4 * d / np.linalg.norm(d, axis=1, keepdims=True)
        pick = np.arange(mm) % 3 == 1
        pts[pick] = ring[pick]
    return pts[:m].astype(np.float32)


def degenerate_queries(verts, faces, n, seed):
    """Up to 3 n queries f32 where the solid angle of some face is undefined: on vertices, on edge midpoints and on face centroids."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, dtype=np.float32)
    f = np.asarray(faces)
    pick = rng.integers(0, f.shape[0], n)
    t = v[f[pick]].astype(np.float64)
    return np.concatenate([t[:, 0], 0.5 * (t[:, 0] + t[:, 1]), t.mean(axis=1)]).astype(np.float32)


WINDING_CASES = ('one_face', 'two_faces', 'corner3', 'ico63', 'ico64', 'ico65', 'ico320', 'ico313', 'abc500')
_CASES = {}


def winding_mesh(name):
    """(verts f32, faces int64) of a winding case: the smallest meshes that reach every path of the sweep.  one face (w is a single
    atan2_fast), two faces sharing an edge, three faces that each carry their own copy of one corner, the 63 / 64 / 65-face prefixes of
    icosphere(1, 0.3) (one slice against two, SWEEP_MIN_SLICE = 64), icosphere(2, 0.3) closed (5 slices of 64) and its open 313-face
    prefix (5 slices of 63, the last with 61), and the first 500 faces of an ABC ground-truth fixture for its slivers."""
    tri = np.array([[0.2, 0.0, 0.01], [-0.1, 0.17, -0.02], [-0.1, -0.15, 0.03], [0.15, 0.2, 0.1]])
    if name == 'one_face':
        v, f = tri[:3], np.array([[0, 1, 2]])
    elif name == 'two_faces':
        v, f = tri, np.array([[0, 1, 2], [1, 0, 3]])
    elif name == 'corner3':
        apex, ring = np.array([0.01, -0.02, 0.2]), tri[:3]
        v = np.concatenate([[apex, ring[k], ring[(k + 1) % 3]] for k in range(3)])
        f = np.arange(9).reshape(3, 3)
    elif name.startswith('ico'):
        n = int(name[3:])
        v, f = icosphere(1 if n <= 80 else 2, 0.3)
        f = f[:n]
    else:
        import os
        from ppsurf_amd import meshio
        gt = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'abc_minimal_gt', '03_meshes')
        # the first fixture: by the reference alone its bound stays under WINDING_CAP for all but 0.4 % of the queries.  The other two
        # leave 1.5 % and 2.1 % over it (queries next to the prolonged long edge of a sliver, where det and den both cancel to 1e-4 |a||b||c|
        # and fp32 does not define the angle), more than check_winding accepts as unchecked.
        v, f = meshio.read_ply_mesh(os.path.join(gt, sorted(os.listdir(gt))[0]))
        f = f[:500]
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int64)


def winding_case(name, m=3000):
    """The inputs and the reference of a winding case, computed once and shared (treat the arrays as read-only): a dict of verts, faces,
    pts f32 [m + planted, 3] (winding_queries, then the planted degenerate queries), planted bool, w and bound (winding_spec_bounded)."""
    if (name, m) not in _CASES:
        v, f = winding_mesh(name)
        pts = winding_queries(v, f, m, seed=len(name) + f.shape[0], sphere=f.shape[0] < 4)
        deg = degenerate_queries(v, f, 20, seed=1)
        planted = np.arange(m + deg.shape[0]) >= m
        pts = np.concatenate([pts, deg])
        w, bound = winding_spec_bounded(v, f, pts)
        _CASES[(name, m)] = dict(verts=v, faces=f, pts=pts, planted=planted, w=w, bound=bound)
    return _CASES[(name, m)]


def check_winding(case, w_got):
    """The assertions every winding case makes of an fp64 [m] result; returns max(err / bound) over the queries held to their bound.
    From the reference alone, first: at most 1 % of the queries that are not planted have a bound above WINDING_CAP (so the cap cannot
    hide a failure).  Then |w_got - w| <= bound wherever bound < WINDING_CAP, and the inside mask agrees wherever ||w| - 0.5| > bound.
    Of the planted queries only: finite, |w| <= (nf + 1) / 2."""
    w, bound, planted = case['w'], case['bound'], case['planted']
    held = bound < WINDING_CAP
    assert (~held[~planted]).mean() <= 0.01, 'the reference leaves {:.2%} of the queries unchecked'.format((~held[~planted]).mean())
    assert np.isfinite(w_got).all() and (np.abs(w_got) <= (case['faces'].shape[0] + 1) / 2).all()
    err = np.abs(w_got - w)
    bad = held & ~(err <= bound)
    assert not bad.any(), '{} of {} queries beyond their bound, worst err / bound {:.3g}'.format(bad.sum(), held.sum(), (err[held] / bound[held]).max())
    clear = np.abs(np.abs(w) - 0.5) > bound
    assert np.array_equal((np.abs(w_got) > 0.5)[clear], (np.abs(w) > 0.5)[clear])
    return float((err[held] / bound[held]).max())


# ---- the reduction -----------------------------------------------------------------------------------------------------------------------------------
def reduce_spec(d2_rg, d2_gr, nn_rg, face_rec, face_gt, normal_rec, normal_gt, w_rec, w_gt):
    """(sums, bound), both fp64 [8]: reduce_kernel of pps_eval.hip by plain numpy sums -- sum sqrt(d2_rg), sum sqrt(d2_gr), TP, FP, FN, TN,
    sum arccos(clip(cosine)), number of non-NaN cosines -- and what the kernel may differ by.  The counts are exact (bound 0).  A sum of n
    fp64 terms in another order differs by at most n 2^-53 sum|term| (+ 2 for the last bit of sqrt / acos themselves).  The kernel's cosine
    is an fp32 dot product, three products and two additions, off by at most delta = 3 * 2^-24 * sum|a_i b_i| from the exact one, and acos
    is steep at +-1, so each term of the arccos sum may move by acos(clip(cs - delta)) - acos(clip(cs + delta)), clip to [-1, 1].
    d2_rg / d2_gr and the normal group may be None (mesh_metrics passes None for a mesh without area)."""
    out, bound = np.zeros(8), np.zeros(8)
    for k, d2 in ((0, d2_rg), (1, d2_gr)):
        if d2 is not None:
            term = np.sqrt(np.asarray(d2, dtype=np.float32).astype(np.float64))
            out[k], bound[k] = term.sum(), (term.shape[0] + 2) * 2.0 ** -53 * term.sum()
    in_rec, in_gt = np.abs(np.asarray(w_rec, dtype=np.float64)) > 0.5, np.abs(np.asarray(w_gt, dtype=np.float64)) > 0.5
    out[2:6] = [(in_rec & in_gt).sum(), (in_rec & ~in_gt).sum(), (~in_rec & in_gt).sum(), (~in_rec & ~in_gt).sum()]
    if normal_rec is not None:
        a = np.asarray(normal_rec, dtype=np.float32).astype(np.float64)[np.asarray(face_rec)]
        b = np.asarray(normal_gt, dtype=np.float32).astype(np.float64)[np.asarray(face_gt)[np.asarray(nn_rg)]]
        cs = (a * b).sum(axis=1)
        ok = ~np.isnan(cs)
        cs, delta = cs[ok], 3.0 * EPS32 * np.abs(a * b).sum(axis=1)[ok]
        term = np.arccos(np.clip(cs, -1.0, 1.0))
        slack = np.arccos(np.clip(cs - delta, -1.0, 1.0)) - np.arccos(np.clip(cs + delta, -1.0, 1.0))
        out[6], out[7] = term.sum(), ok.sum()
        bound[6] = slack.sum() + (term.shape[0] + 2) * 2.0 ** -53 * term.sum()
    return out, bound


def reduce_inputs(n_rec, n_gt, mq, seed=0):
    """Crafted inputs of the reduction (host arrays by the argument names of reduce_spec; n_gt >= 100): unit normals with equal and opposite
    pairs (cosines at +-1, where acos is steep), exact zeros (degenerate faces), rows scaled by 1.001 with an equal and an opposite partner
    (|cosine| > 1: the clamp on both sides), NaN rows on either side (skipped, not counted); the special rows are reached by the first
    twelve samples and by the last one.  Winding numbers on all four confusion cells, at exactly +-0.5 (outside), just above 0.5 and at
    -0.7 (inside)."""
    rng = np.random.default_rng(seed)
    nfr, nfg = 37, 53
    nr, ng = rng.standard_normal((nfr, 3)), rng.standard_normal((nfg, 3))
    nr, ng = nr / np.linalg.norm(nr, axis=1, keepdims=True), ng / np.linalg.norm(ng, axis=1, keepdims=True)
    ng[0:nfr:4] = nr[0:nfr:4]
    ng[1:nfr:8] = -nr[1:nfr:8]
    nr[3], ng[5] = 0.0, 0.0
    nr[7:10] *= 1.001
    ng[8], ng[9] = nr[8] / 1.001, -nr[9] / 1.001
    nr[11], ng[13] = np.nan, np.nan
    face_rec = rng.integers(0, nfr, n_rec).astype(np.int32)
    face_gt = rng.integers(0, nfg, n_gt).astype(np.int32)
    nn_rg = rng.integers(0, n_gt, n_rec).astype(np.int64)
    k = min(n_rec, 12)
    nn_rg[:k] = (7 * np.arange(k) + 3) % n_gt
    face_rec[:k] = [3, 7, 8, 9, 11, 0, 4, 1, 9, 8, 12, 16][:k]
    face_gt[nn_rg[:k]] = [0, 7, 8, 9, 2, 5, 4, 1, 13, 8, 12, 16][:k]
    if n_rec > 12:
        nn_rg[-1], face_rec[-1], face_gt[n_gt - 1] = n_gt - 1, 9, 9
    d2_rg = (rng.random(n_rec) ** 4).astype(np.float32)
    d2_gr = (rng.random(n_gt) ** 4).astype(np.float32)
    d2_rg[::5] = 0.0
    cells = np.array([[0.7, 0.9], [1.0, 0.2], [0.1, -0.7], [0.3, 0.4], [0.5, 0.5], [-0.5, 0.51], [-0.7, -0.5], [np.nextafter(0.5, 1), -0.7]])
    w = cells[rng.integers(0, cells.shape[0], mq)] if mq else np.zeros((0, 2))
    if mq >= cells.shape[0]:
        w[:cells.shape[0]] = cells
    return dict(d2_rg=d2_rg, d2_gr=d2_gr, nn_rg=nn_rg, face_rec=face_rec, face_gt=face_gt, normal_rec=nr.astype(np.float32),
                normal_gt=ng.astype(np.float32), w_rec=np.ascontiguousarray(w[:, 0]), w_gt=np.ascontiguousarray(w[:, 1]))


def icosphere(subdiv, radius=1.0):
    """Subdivided icosahedron on a sphere of `radius`, faces counter-clockwise seen from outside -> (verts f64 [nv,3], faces int64 [nf,3])."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = f
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = verts[i] + verts[j]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return np.array(verts) * radius, np.array(faces, dtype=np.int64)


def mesh_volume(verts, faces):
    """Signed volume of a closed triangle mesh (positive for outward faces)."""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    return float(np.einsum('fi,fi->f', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def ply_header_counts(path):
    """{element name: count} from a PLY header."""
    counts = {}
    with open(path, 'rb') as f:
        for line in f:
            tok = line.decode('ascii', 'replace').split()
            if tok and tok[0] == 'element':
                counts[tok[1]] = int(tok[2])
            if tok and tok[0] == 'end_header':
                break
    return counts
