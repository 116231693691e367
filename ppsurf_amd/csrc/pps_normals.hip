// Oriented normals for gfx950: per-vertex normals of a mesh and their blend onto the points of a scan.
//
// new capability: replaces nothing -- the reference writes positions only (source/poco_model.py:269 `mesh.export`).  Driven by
// ppsurf_amd/normals.py; restated in numpy by tests/normals_spec.py, which the kernels match bit for bit.
//
// Rule A, vertex normals: vertices V f32 [nv,3], faces int64 [nf,3], weight 'area' (0) or 'max' (1).
//   valid face    its three indices lie in [0, nv) and are pairwise distinct (face_valid of pps_faces.h).  Invalid faces take no part and are
//                 never read through.
//   incidence     a valid face t = (a, b, c) contributes the keys (a << 32) | t, (b << 32) | t, (c << 32) | t, an invalid one INT64_MAX three
//                 times (nv, nf <= 2^31 - 1).  The keys are distinct, so the sorted keys without the sentinel list every vertex's faces in
//                 ASCENDING FACE INDEX whatever the sort; a duplicated face sits in the row twice and counts twice.
//   per vertex i  in fp64 on the widened f32 coordinates, every operation rounded on its own (-ffp-contract=off): acc = (0, 0, 0); for the
//                 faces t of the row in order, with p the corner of t that equals i, n the next corner cyclically and q the one after:
//                   e1 = V[n] - V[i];  e2 = V[q] - V[i];
//                   g = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)         (the right-hand rule of the face's winding)
//                   area:  acc = acc + g                                                     (every face weighs in by its area)
//                   max:   d = ((e1x^2 + e1y^2) + e1z^2) * ((e2x^2 + e2y^2) + e2z^2);  d > 0 and finite: acc = acc + g / d (three
//                          divisions; Max 1999), otherwise the face adds nothing at this vertex
//                 L = sqrt((accx^2 + accy^2) + accz^2);  L > 0 and finite: out = f32(acc / L), a division per component, nearest-even;
//                 otherwise (0, 0, 0).  Non-finite values need no special case: the comparisons fail.  No valid face: (0, 0, 0).
// Rule B, point normals: idx int64 [m,k], d2 f32 [m,k] (the k nearest vertices, ops.KnnBlocks), normals N f32 [nv,3], eps.  Per row, columns
//   j = 0..k-1 in order, in fp64: a neighbour counts when 0 <= idx < nv;  w = 1 / (double(d2) + eps);  T_c = T_c + w * double(N[idx, c])
//   (a multiply, then an add);  normalised exactly as in rule A.
// Both are pure functions of their inputs: no float atomics, the order of every sum is the order of the sorted keys or of the columns.  The
// normals follow the winding; nothing is re-oriented.
//
// Between corner_keys and vertex the caller sorts the keys, drops the sentinel and takes the row offsets from a bincount of key >> 32; the
// face list is int32(key & 0xFFFFFFFF) (ppsurf_amd/normals.py).
//
// Shape: corner_keys_kernel one thread per face, three 8-byte stores.  vertex_kernel one thread per vertex and blend_kernel one thread per
// row: the sum of a row is sequential by rule, so a row is one lane's work (as pass_kernel of pps_smooth.hip).  Plain vector loads and stores,
// no LDS, no atomics.  Every offset, face index, corner and neighbour is range-checked before it becomes an address.
#include <math.h>

#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v < (double)INFINITY; }          // false for a NaN

// out[0..2] = f32(acc / L) when L = sqrt((ax^2 + ay^2) + az^2) is > 0 and finite, else zeros
__device__ __forceinline__ void store_unit(const double acc[3], float* __restrict__ out) {
    const double L = sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
    const bool ok = positive_finite(L);
    out[0] = ok ? (float)(acc[0] / L) : 0.0f;
    out[1] = ok ? (float)(acc[1] / L) : 0.0f;
    out[2] = ok ? (float)(acc[2] / L) : 0.0f;
}

__global__ __launch_bounds__(256) void corner_keys_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, int64_t* __restrict__ keys) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool valid = face_valid(a, b, c, nv);
    int64_t* k = keys + 3 * f;
    k[0] = valid ? (a << 32) | f : KEY_SENTINEL;
    k[1] = valid ? (b << 32) | f : KEY_SENTINEL;
    k[2] = valid ? (c << 32) | f : KEY_SENTINEL;
}

__global__ __launch_bounds__(256) void vertex_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                     const int64_t* __restrict__ offsets, const int32_t* __restrict__ inc, int64_t ni, int weight,
                                                     float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t o0 = offsets[i], o1 = offsets[i + 1];
    if (o0 >= 0 && o0 <= o1 && o1 <= ni) {                  // a row outside [0, ni] is skipped, never read
        const double xi[3] = {(double)verts[3 * i], (double)verts[3 * i + 1], (double)verts[3 * i + 2]};
        for (int64_t e = o0; e < o1; ++e) {                 // row order = ascending face index
            const int64_t t = inc[e];
            if (t < 0 || t >= nf) continue;
            const int64_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
            if (!face_valid(a, b, c, nv)) continue;
            int64_t n, q;
            if (a == i) { n = b; q = c; }
            else if (b == i) { n = c; q = a; }
            else if (c == i) { n = a; q = b; }
            else continue;                                  // a face that does not hold i
            const double e1[3] = {(double)verts[3 * n] - xi[0], (double)verts[3 * n + 1] - xi[1], (double)verts[3 * n + 2] - xi[2]};
            const double e2[3] = {(double)verts[3 * q] - xi[0], (double)verts[3 * q + 1] - xi[1], (double)verts[3 * q + 2] - xi[2]};
            double g[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            if (weight == 1) {
                const double d = ((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]) * ((e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]);
                if (!positive_finite(d)) continue;
                g[0] = g[0] / d;
                g[1] = g[1] / d;
                g[2] = g[2] / d;
            }
            acc[0] = acc[0] + g[0];
            acc[1] = acc[1] + g[1];
            acc[2] = acc[2] + g[2];
        }
    }
    store_unit(acc, out + 3 * i);
}

__global__ __launch_bounds__(256) void blend_kernel(const int64_t* __restrict__ idx, const float* __restrict__ d2, int64_t m, int k,
                                                    const float* __restrict__ normals, int64_t nv, double eps, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t* ti = idx + i * (int64_t)k;
    const float* di = d2 + i * (int64_t)k;
    double T[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
        const int64_t t = ti[j];
        const float d = di[j];
        if (t >= 0 && t < nv) {
            const double w = 1.0 / ((double)d + eps);
            T[0] = T[0] + w * (double)normals[3 * t];
            T[1] = T[1] + w * (double)normals[3 * t + 1];
            T[2] = T[2] + w * (double)normals[3 * t + 2];
        }
    }
    store_unit(T, out + 3 * i);
}

}  // namespace

extern "C" {

int ppsx_normals_corner_keys(const int64_t* faces, int64_t nf, int64_t nv, int64_t* keys, void* stream) {
    if (nf < 0 || nv < 0 || nv > (int64_t)INT32_MAX || nf > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !keys) return PPS_ERR_ARG;
    hipLaunchKernelGGL(corner_keys_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, keys);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_normals_vertex(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* inc, int64_t ni,
                        int weight, float* out, void* stream) {
    if (nv < 0 || nf < 0 || ni < 0 || nv > (int64_t)INT32_MAX || nf > (int64_t)INT32_MAX || (weight != 0 && weight != 1)) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    if (!verts || !offsets || !out || (nf > 0 && !faces) || (ni > 0 && !inc)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(vertex_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, faces, nf, offsets, inc,
                       ni, weight, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_normals_blend(const int64_t* idx, const float* d2, int64_t m, int k, const float* normals, int64_t nv, double eps, float* out,
                       void* stream) {
    if (m < 0 || nv < 0 || k < 1 || k > 256 || !(eps > 0.0)) return PPS_ERR_ARG;
    if (m == 0) return PPS_OK;
    if (!idx || !d2 || !out || (nv > 0 && !normals) || (m + 255) / 256 > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    hipLaunchKernelGGL(blend_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, d2, m, k, normals, nv, eps, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
