// Evaluation of a reconstruction against its ground-truth mesh (source/base/metrics.py:120-323): face statistics, area-weighted surface
// sampling, the generalised winding number of query points (inside / outside for IoU and F1) and the deterministic fp64 sums of the four
// metrics.  The reference runs trimesh / pysdf / pykdtree on the CPU in a process pool; the 1-NN searches of the Chamfer and normal-error
// steps reuse the kNN kernels of pps_knn.hip (k = 1).
//
// Counter-based generator of the surface sampling (restated in numpy by tests/eval_spec.py; keep the two in step):
//     mix(x)    = splitmix64 finaliser of x + 0x9E3779B97F4A7C15:
//                   z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//                   return z ^ (z >> 31)                                                       (all uint64, wrapping)
//     key       = mix(mix(seed) ^ stream_id)
//     bits(i,d) = mix(key ^ ((uint64)i << 2 | d))            sample index i, draw d in {0, 1, 2}
//     u53       = (bits(i,0) >> 11) * 2^-53                  fp64 in [0, 1)
//     r1, r2    = (bits(i,1) >> 40) * 2^-24, (bits(i,2) >> 40) * 2^-24          fp32 in [0, 1)
//   face      = upper bound of t = u53 * total in the inclusive fp64 prefix of the face areas (first j with prefix[j] > t, i.e.
//               searchsorted(prefix, t, side='right')); if t rounds up to total, the first j with prefix[j] == total (the last face of
//               positive area).  A face of zero area is never drawn.
//   if r1 + r2 > 1 (fp32): r1, r2 = 1 - r1, 1 - r2              (trimesh's parallelogram fold)
//   point     = (r1 * e1 + r2 * e2) + v0, e1 = v1 - v0, e2 = v2 - v0, fp32 without contraction (trimesh's order of operations)
// Sample i depends on (seed, stream_id, i) only: the first k samples of a draw of n are the draw of k.
#include <math.h>

#include "pps_common.h"
#include "../../include/ppsurf_amd.h"

namespace {

constexpr int WIND_BLOCK = 256;
constexpr int WIND_QPL = 4;                                   // queries per lane, held in registers
constexpr int WIND_QBLOCK = WIND_BLOCK * WIND_QPL;            // queries per workgroup
constexpr int64_t WIND_TARGET_BLOCKS = 16384;                 // ~10 rounds of 256 CUs x 6 resident workgroups: a short tail
constexpr int64_t WIND_MIN_SLICE = 64;                        // faces per slice, at least

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

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
    const double u = (double)(mix64(key ^ ctr) >> 11) * 0x1.0p-53;
    float r1 = (float)(uint32_t)(mix64(key ^ (ctr | 1)) >> 40) * 0x1.0p-24f;
    float r2 = (float)(uint32_t)(mix64(key ^ (ctr | 2)) >> 40) * 0x1.0p-24f;
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

// atan2(y, x) with a degree-15 odd polynomial for atan on [0, 1] (max error 1.2e-7 rad in fp32) and one v_rcp_f32 -- ocml's atan2f spends
// twice the instructions on a correctly rounded division and on special cases that cannot occur here (x, y finite).
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

// Partial winding sums: workgroup (qb, s) adds, for WIND_QBLOCK queries, the half solid angles atan2(det, D) of the faces of slice s in face
// order (Van Oosterom-Strackee: Omega_f = 2 atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a b c = corners - query).
// The face index is wave-uniform, so the nine corner floats of a face are scalar loads shared by the wave; each lane keeps WIND_QPL
// queries and their fp32 sums in registers.  partial[s, q] = sum over slice s, no atomics.  The lengths use the bare v_sqrt_f32 (1 ulp):
// sqrtf's correctly rounded expansion (denormal scaling + two correction steps) was about half of the loop.
__global__ __launch_bounds__(WIND_BLOCK) void winding_partial_kernel(const float* __restrict__ corners, int64_t nf, const float* __restrict__ query,
                                                                     int64_t m, int64_t per_slice, float* __restrict__ partial) {
    const int64_t q0 = (int64_t)blockIdx.x * WIND_QBLOCK + threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.y * per_slice;
    const int64_t f1 = f0 + per_slice < nf ? f0 + per_slice : nf;
    float px[WIND_QPL], py[WIND_QPL], pz[WIND_QPL], acc[WIND_QPL];
#pragma unroll
    for (int j = 0; j < WIND_QPL; ++j) {
        int64_t q = q0 + (int64_t)j * WIND_BLOCK;
        q = q < m ? q : m - 1;
        px[j] = query[3 * q];
        py[j] = query[3 * q + 1];
        pz[j] = query[3 * q + 2];
        acc[j] = 0.f;
    }
    for (int64_t f = f0; f < f1; ++f) {
        const float* c = corners + 9 * f;
        const float c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6], c7 = c[7], c8 = c[8];
#pragma unroll
        for (int j = 0; j < WIND_QPL; ++j) {
            const float ax = c0 - px[j], ay = c1 - py[j], az = c2 - pz[j];
            const float bx = c3 - px[j], by = c4 - py[j], bz = c5 - pz[j];
            const float cx = c6 - px[j], cy = c7 - py[j], cz = c8 - pz[j];
            const float la = __builtin_amdgcn_sqrtf(fmaf(ax, ax, fmaf(ay, ay, az * az)));
            const float lb = __builtin_amdgcn_sqrtf(fmaf(bx, bx, fmaf(by, by, bz * bz)));
            const float lc = __builtin_amdgcn_sqrtf(fmaf(cx, cx, fmaf(cy, cy, cz * cz)));
            const float det = fmaf(ax, fmaf(by, cz, -bz * cy), fmaf(ay, fmaf(bz, cx, -bx * cz), az * fmaf(bx, cy, -by * cx)));
            const float ab = fmaf(ax, bx, fmaf(ay, by, az * bz));
            const float bc = fmaf(bx, cx, fmaf(by, cy, bz * cz));
            const float ca = fmaf(cx, ax, fmaf(cy, ay, cz * az));
            const float den = fmaf(la * lb, lc, fmaf(ab, lc, fmaf(bc, la, ca * lb)));
            acc[j] += atan2_fast(det, den);
        }
    }
    float* out = partial + (int64_t)blockIdx.y * m;
#pragma unroll
    for (int j = 0; j < WIND_QPL; ++j) {
        const int64_t q = q0 + (int64_t)j * WIND_BLOCK;
        if (q < m) out[q] = acc[j];
    }
}

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
    const uint64_t key = mix64(mix64(seed) ^ stream_id);
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, corners, area_prefix, nf, n, key, out_pts, out_face);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int64_t pps_eval_winding_slices(int64_t m, int64_t nf) {
    if (m < 1 || nf < 1) return -1;
    const int64_t qblocks = (m + WIND_QBLOCK - 1) / WIND_QBLOCK;
    int64_t s = (WIND_TARGET_BLOCKS + qblocks - 1) / qblocks;
    const int64_t smax = (nf + WIND_MIN_SLICE - 1) / WIND_MIN_SLICE;
    s = s < smax ? s : smax;
    const int64_t per = (nf + s - 1) / s;                     // no empty slice
    return (nf + per - 1) / per;
}

int pps_eval_winding(const float* corners, int64_t nf, const float* query, int64_t m, int64_t slices, float* partial, double* out_w, void* stream) {
    if (nf < 1 || m < 0) return PPS_ERR_ARG;
    if (m == 0) return PPS_OK;
    if (slices != pps_eval_winding_slices(m, nf)) return PPS_ERR_ARG;
    if (!corners || !query || !partial || !out_w) return PPS_ERR_ARG;
    const int64_t qblocks = (m + WIND_QBLOCK - 1) / WIND_QBLOCK;
    if (qblocks > INT32_MAX || slices > 65535) return PPS_ERR_ARG;
    const int64_t per = (nf + slices - 1) / slices;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(winding_partial_kernel, dim3((unsigned)qblocks, (unsigned)slices), dim3(WIND_BLOCK), 0, st, corners, nf, query, m, per, partial);
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
