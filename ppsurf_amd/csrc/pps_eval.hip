// Evaluation of a reconstruction against its ground-truth mesh (source/base/metrics.py:120-323): face statistics, area-weighted surface
// sampling, the generalised winding number of query points (inside / outside for IoU and F1) and the deterministic fp64 sums of the four
// metrics.  The reference runs trimesh / pysdf / pykdtree on the CPU in a process pool; the 1-NN searches of the Chamfer and normal-error
// steps reuse the kNN kernels of pps_knn.hip (k = 1).
//
// Surface sampling (restated in numpy by tests/eval_spec.py; keep the two in step), generator and its conversions as in pps_rng.h:
//   u53       = unit53(bits(i << 2)),  r1, r2 = unit24(bits(i << 2 | 1)), unit24(bits(i << 2 | 2))           sample index i
//   face      = upper bound of t = u53 * total in the inclusive fp64 prefix of the face areas (first j with prefix[j] > t, i.e.
//               searchsorted(prefix, t, side='right')); if t rounds up to total, the first j with prefix[j] == total (the last face of
//               positive area).  A face of zero area is never drawn.
//   if r1 + r2 > 1 (fp32): r1, r2 = 1 - r1, 1 - r2              (trimesh's parallelogram fold)
//   point     = (r1 * e1 + r2 * e2) + v0, e1 = v1 - v0, e2 = v2 - v0, fp32 without contraction (trimesh's order of operations)
// Sample i depends on (seed, stream_id, i) only: the first k samples of a draw of n are the draw of k.
//
// The winding number is one operation of the sliced face sweep of pps_sweep.h.
#include <math.h>

#include "pps_common.h"
#include "pps_rng.h"
#include "pps_sweep.h"
#include "../../include/ppsurf_amd.h"

namespace {

// area = 0.5 |e1 x e2|, unit normal (e1 x e2) / |e1 x e2| (0 for a degenerate face), corners v0 v1 v2 face-major [nf, 9].  A face with an
// index outside [0, nv) reads no vertex and gets area 0, normal 0 and corners 0.
__global__ __launch_bounds__(256) void face_stats_kernel(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces, int64_t nf,
                                                         float* __restrict__ area, float* __restrict__ normal, float* __restrict__ corners) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    float v[9];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = 0.f;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = verts[3 * (int64_t)i0 + k];
            v[3 + k] = verts[3 * (int64_t)i1 + k];
            v[6 + k] = verts[3 * (int64_t)i2 + k];
        }
    }
    const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
    const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    area[f] = 0.5f * len;
    const float inv = len > 0.f ? 1.f / len : 0.f;
    normal[3 * f] = cx * inv;
    normal[3 * f + 1] = cy * inv;
    normal[3 * f + 2] = cz * inv;
#pragma unroll
    for (int k = 0; k < 9; ++k) corners[9 * f + k] = v[k];
}

__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ corners, const double* __restrict__ prefix, int64_t nf, int64_t n,
                                                     uint64_t key, float* __restrict__ pts, int32_t* __restrict__ face) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t ctr = (uint64_t)i << 2;
    const double u = unit53(rng_bits(key, ctr));
    float r1 = unit24(rng_bits(key, ctr | 1));
    float r2 = unit24(rng_bits(key, ctr | 2));
    const double total = prefix[nf - 1];
    const double t = u * total;
    int64_t lo = 0, hi = nf;                                  // upper bound: first j with prefix[j] > t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (prefix[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo == nf) {                                           // t rounded up to total: first j with prefix[j] == total
        lo = 0, hi = nf - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (prefix[mid] >= total) hi = mid; else lo = mid + 1;
        }
    }
    if (r1 + r2 > 1.f) {
        r1 = 1.f - r1;
        r2 = 1.f - r2;
    }
    const float* c = corners + 9 * lo;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float e1 = c[3 + k] - c[k], e2 = c[6 + k] - c[k];
        pts[3 * i + k] = (r1 * e1 + r2 * e2) + c[k];
    }
    face[i] = (int32_t)lo;
}

// atan2(y, x) with a degree-15 odd polynomial for atan on [0, 1] and one v_rcp_f32 -- ocml's atan2f spends twice the instructions on a
// correctly rounded division and on special cases that cannot occur here (x, y finite).  Error against atan2 in fp64, measured on the
// numpy fp32 restatement of this function (tests/eval_spec.py, atan2_fast_twin; keep the coefficients in step): the polynomial alone
// 6.4e-8 rad evaluated in fp64; quotient and polynomial in fp32 on [0, 1] 1.3e-7 rad; the whole atan2 with its reflections 3.3e-7 rad, worst
// near 2.52 rad, where float32(pi) - r is rounded at magnitude 2.5.  v_rcp_f32 (1 ulp) adds at most 2^-23 rad: 4.5e-7 rad in all, the
// figure the tests allow per face.  x = -0 counts as +0: atan2_fast(+-0, -0) = +-0.
__device__ __forceinline__ float atan2_fast(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const bool swap = ay > ax;
    const float mx = swap ? ay : ax, mn = swap ? ax : ay;
    const float t = mn * __builtin_amdgcn_rcpf(mx + 1e-30f);     // + 1e-30: 0 / 0 -> 0 (a query on a corner); no effect for mx >= 1e-22
    const float s = t * t;
    float p = -0.004054495599120855f;
    p = fmaf(p, s, 0.02186269313097f);
    p = fmaf(p, s, -0.05591193586587906f);
    p = fmaf(p, s, 0.09642168134450912f);
    p = fmaf(p, s, -0.13908617198467255f);
    p = fmaf(p, s, 0.19946563243865967f);
    p = fmaf(p, s, -0.33329859375953674f);
    p = fmaf(p, s, 0.9999993443489075f);
    float r = t * p;
    r = swap ? 1.5707963267948966f - r : r;
    r = x < 0.f ? 3.141592653589793f - r : r;
    return copysignf(r, y);
}

// Partial winding sums (pps_sweep.h): every query adds the half solid angles atan2(det, D) of the faces of its slice in face order, in fp32
// (Van Oosterom-Strackee: Omega_f = 2 atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a b c = corners - query).
// The lengths use the bare v_sqrt_f32 (1 ulp): sqrtf's correctly rounded expansion (denormal scaling + two correction steps) was about
// half of the loop.
struct WindingOp {
    const float* __restrict__ query;
    float* __restrict__ partial;
    struct Item { float px, py, pz, acc; };
    __device__ __forceinline__ Item load(int64_t q) const { return {query[3 * q], query[3 * q + 1], query[3 * q + 2], 0.f}; }
    __device__ __forceinline__ void face(const float* __restrict__ c, int32_t, Item (&it)[SWEEP_IPL]) const {
        const float c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6], c7 = c[7], c8 = c[8];
#pragma unroll
        for (int j = 0; j < SWEEP_IPL; ++j) {
            const float ax = c0 - it[j].px, ay = c1 - it[j].py, az = c2 - it[j].pz;
            const float bx = c3 - it[j].px, by = c4 - it[j].py, bz = c5 - it[j].pz;
            const float cx = c6 - it[j].px, cy = c7 - it[j].py, cz = c8 - it[j].pz;
            const float la = __builtin_amdgcn_sqrtf(fmaf(ax, ax, fmaf(ay, ay, az * az)));
            const float lb = __builtin_amdgcn_sqrtf(fmaf(bx, bx, fmaf(by, by, bz * bz)));
            const float lc = __builtin_amdgcn_sqrtf(fmaf(cx, cx, fmaf(cy, cy, cz * cz)));
            const float det = fmaf(ax, fmaf(by, cz, -bz * cy), fmaf(ay, fmaf(bz, cx, -bx * cz), az * fmaf(bx, cy, -by * cx)));
            const float ab = fmaf(ax, bx, fmaf(ay, by, az * bz));
            const float bc = fmaf(bx, cx, fmaf(by, cy, bz * cz));
            const float ca = fmaf(cx, ax, fmaf(cy, ay, cz * az));
            const float den = fmaf(la * lb, lc, fmaf(ab, lc, fmaf(bc, la, ca * lb)));
            it[j].acc += atan2_fast(det, den);
        }
    }
    __device__ __forceinline__ void store(const Item& it, int64_t k) const { partial[k] = it.acc; }
};

// w[q] = (sum over s in slice order of partial[s, q], fp64) / (2 pi)
__global__ __launch_bounds__(256) void winding_sum_kernel(const float* __restrict__ partial, int64_t slices, int64_t m, double* __restrict__ w) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    double s = 0.0;
    for (int64_t k = 0; k < slices; ++k) s += (double)partial[k * m + q];
    w[q] = s * (1.0 / (2.0 * 3.141592653589793));
}

constexpr int RED_BLOCK = 512;

// One workgroup: every thread sums a fixed strided subset in fp64, then a fixed-shape tree in LDS.  Bitwise reproducible.
__global__ __launch_bounds__(RED_BLOCK) void reduce_kernel(const float* __restrict__ d2_rg, int64_t n_rec, const float* __restrict__ d2_gr, int64_t n_gt,
                                                           const int64_t* __restrict__ nn_rg, const int32_t* __restrict__ face_rec,
                                                           const int32_t* __restrict__ face_gt, const float* __restrict__ nrm_rec,
                                                           const float* __restrict__ nrm_gt, const double* __restrict__ w_rec,
                                                           const double* __restrict__ w_gt, int64_t mq, double* __restrict__ out) {
    __shared__ double red[8][RED_BLOCK];
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < n_rec; i += RED_BLOCK) {
        v[0] += sqrt((double)d2_rg[i]);
        if (nrm_rec) {
            const float* a = nrm_rec + 3 * (int64_t)face_rec[i];
            const float* b = nrm_gt + 3 * (int64_t)face_gt[nn_rg[i]];
            double cs = (double)(a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
            if (cs == cs) {                                   // NaN skipped (np.nanmean)
                cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
                v[6] += acos(cs);
                v[7] += 1.0;
            }
        }
    }
    for (int64_t i = tid; i < n_gt; i += RED_BLOCK) v[1] += sqrt((double)d2_gr[i]);
    for (int64_t i = tid; i < mq; i += RED_BLOCK) {
        const bool in_rec = fabs(w_rec[i]) > 0.5, in_gt = fabs(w_gt[i]) > 0.5;
        v[2] += (in_rec && in_gt) ? 1.0 : 0.0;
        v[3] += (in_rec && !in_gt) ? 1.0 : 0.0;
        v[4] += (!in_rec && in_gt) ? 1.0 : 0.0;
        v[5] += (!in_rec && !in_gt) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int h = RED_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[k][tid] += red[k][tid + h];
        }
        __syncthreads();
    }
    if (tid < 8) out[tid] = red[tid][0];
}

}  // namespace

extern "C" {

int pps_eval_face_stats(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, float* area, float* normal, float* corners, void* stream) {
    if (nv < 0 || nf < 0) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!verts || !faces || !area || !normal || !corners) return PPS_ERR_ARG;
    hipLaunchKernelGGL(face_stats_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, faces, nf, area, normal, corners);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_eval_sample_surface(const float* corners, const double* area_prefix, int64_t nf, int64_t n, uint64_t seed, uint64_t stream_id,
                            float* out_pts, int32_t* out_face, void* stream) {
    if (nf < 1 || n < 0 || nf > INT32_MAX) return PPS_ERR_ARG;
    if (n == 0) return PPS_OK;
    if (!corners || !area_prefix || !out_pts || !out_face) return PPS_ERR_ARG;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, corners, area_prefix, nf, n,
                       rng_key(seed, stream_id), out_pts, out_face);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int64_t pps_eval_winding_slices(int64_t m, int64_t nf) { return sweep_slices(m, nf); }

// Unlike the other sweeps, this one insists on the planner's slice count: its fp32 partial sums depend on where the slices are cut.
int pps_eval_winding(const float* corners, int64_t nf, const float* query, int64_t m, int64_t slices, float* partial, double* out_w, void* stream) {
    if (nf < 1 || m < 0) return PPS_ERR_ARG;
    if (m == 0) return PPS_OK;
    if (slices != sweep_slices(m, nf)) return PPS_ERR_ARG;
    if (!corners || !query || !partial || !out_w) return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (!sweep_launch(corners, nf, m, slices, WindingOp{query, partial}, st)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(winding_sum_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const float*)partial, slices, m, out_w);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_eval_reduce(const float* d2_rg, int64_t n_rec, const float* d2_gr, int64_t n_gt, const int64_t* nn_rg, const int32_t* face_rec,
                    const int32_t* face_gt, const float* normal_rec, const float* normal_gt, const double* w_rec, const double* w_gt, int64_t mq,
                    double* out, void* stream) {
    if (n_rec < 0 || n_gt < 0 || mq < 0 || !out) return PPS_ERR_ARG;
    if ((n_rec > 0 && !d2_rg) || (n_gt > 0 && !d2_gr) || (mq > 0 && (!w_rec || !w_gt))) return PPS_ERR_ARG;
    const bool normals = normal_rec || normal_gt || nn_rg || face_rec || face_gt;
    if (normals && (!normal_rec || !normal_gt || !nn_rg || !face_rec || !face_gt || n_gt < 1)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(RED_BLOCK), 0, (hipStream_t)stream, d2_rg, n_rec, d2_gr, n_gt, nn_rg, face_rec, face_gt,
                       normals ? normal_rec : nullptr, normal_gt, w_rec, w_gt, mq, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
