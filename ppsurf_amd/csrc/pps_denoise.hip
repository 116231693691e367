// Feature-preserving mesh denoising for gfx950: face normals, one Jacobi pass of the face-normal filter and one Jacobi pass of the vertex
// update.
//
// new capability: replaces nothing -- the reference has no mesh denoising.  Driven by ppsurf_amd/denoise.py; restated in numpy by
// tests/denoise_spec.py, which the kernels match bit for bit.  The algorithm is Sun, Rosin, Martin and Langbein, "Fast and Effective
// Feature-Preserving Mesh Denoising" (TVCG 2007): no transcendental function anywhere.
//
// Rule: vertices V f32 [nv,3], faces int64 [nf,3], threshold T (fp64, 0 <= T < 1), normal_iters, vertex_iters.  All arithmetic is fp64 on
// the widened f32 input, every operation rounded on its own (-ffp-contract=off).
//   valid face    its three indices lie in [0, nv) and are pairwise distinct (face_valid of pps_faces.h).  An invalid face has the normal
//                 (0, 0, 0) throughout, belongs to no neighbourhood and is never read through.
//   face normal   a valid face (a, b, c): e1 = x_b - x_a; e2 = x_c - x_a; n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);
//                 L = sqrt((nx^2 + ny^2) + nz^2);  L > 0 and finite: n / L, a division per component; otherwise (0, 0, 0).
//   N(i)          of a valid face i: the distinct valid faces that share at least one vertex with i, i included, in ASCENDING FACE INDEX =
//                 the duplicate-free union of the three incidence rows (topology.incidence_rows) of a, b and c.  A duplicated face is two.
//   normal pass   Jacobi, everything read from the old normals.  acc = (0, 0, 0); for j in N(i) in order:
//                   d = (n_i.x n_j.x + n_i.y n_j.y) + n_i.z n_j.z;  d > T:  w = (d - T) * (d - T);  acc_c = acc_c + w * n_j.c
//                 L = sqrt((accx^2 + accy^2) + accz^2);  L > 0 and finite: n_i' = acc / L; otherwise n_i' = n_i.
//                 normal_iters such passes, two buffers ping-ponged.
//   vertex pass   Jacobi too.  For vertex v and its valid faces k in ascending face index (its incidence row), cnt of them:
//                   c_k = ((x_a + x_b) + x_c) / 3.0 with a, b, c in the face's own order;  dv = c_k - x_v;
//                   t = (n_k.x dv.x + n_k.y dv.y) + n_k.z dv.z;  acc = acc + n_k * t
//                 x_v' = x_v + acc / double(cnt).  A vertex without a valid face keeps its value.  vertex_iters passes, all with the
//                 filtered normals: they are not recomputed in between.
//   output        rounded to f32 (nearest-even) once after the last pass by the caller.
// The result is a pure function of (V, F, T, normal_iters, vertex_iters): no atomics, the order of every sum is the ascending face index.
// It depends on the order of the faces through that order, not on the launch shape.
//
// Shape: one thread per face (face_normals_kernel, filter_kernel) or per vertex (vertex_kernel): the sums are sequential by rule, so a row
// is one lane's work, as in pass_kernel of pps_smooth.hip.  filter_kernel never materialises N(i): it merges the three ascending rows with
// three cursors, takes the smallest head and advances every cursor that shows it, so a face that sits in two or three rows is visited once.
// The cursors, ends and heads are nine named scalars, not arrays: an array indexed by "the row with the smallest head" would live in
// scratch.  Trip counts diverge (a wave runs as long as its largest neighbourhood) and every step waits for a dependent gather; these are
// latency-bound kernels and nothing here claims an occupancy or a bandwidth.  Plain vector loads and stores, no LDS, no atomics.  Every
// offset, face index and vertex index read from a table is range-checked before it becomes an address.
#include <math.h>

#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v < (double)INFINITY; }          // false for a NaN

__device__ __forceinline__ double dot3(const double p[3], const double q[3]) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

// out[0..2] = acc / L when L = sqrt((ax^2 + ay^2) + az^2) is > 0 and finite, else `otherwise`: store_unit of pps_normals.hip kept in fp64
__device__ __forceinline__ void store_unit_or(const double acc[3], const double otherwise[3], double* __restrict__ out) {
    const double L = sqrt(dot3(acc, acc));
    const bool ok = positive_finite(L);
    out[0] = ok ? acc[0] / L : otherwise[0];
    out[1] = ok ? acc[1] / L : otherwise[1];
    out[2] = ok ? acc[2] / L : otherwise[2];
}

__global__ __launch_bounds__(256) void face_normals_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                           double* __restrict__ normals) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const double zero[3] = {0.0, 0.0, 0.0};
    double g[3] = {0.0, 0.0, 0.0};
    if (face_valid(a, b, c, nv)) {
        const double xa[3] = {(double)verts[3 * a], (double)verts[3 * a + 1], (double)verts[3 * a + 2]};
        const double e1[3] = {(double)verts[3 * b] - xa[0], (double)verts[3 * b + 1] - xa[1], (double)verts[3 * b + 2] - xa[2]};
        const double e2[3] = {(double)verts[3 * c] - xa[0], (double)verts[3 * c + 1] - xa[1], (double)verts[3 * c + 2] - xa[2]};
        g[0] = e1[1] * e2[2] - e1[2] * e2[1];
        g[1] = e1[2] * e2[0] - e1[0] * e2[2];
        g[2] = e1[0] * e2[1] - e1[1] * e2[0];
    }
    store_unit_or(g, zero, normals + 3 * f);
}

// the row of vertex v as a cursor and its end; an empty one for a row outside [0, ni]
__device__ __forceinline__ void open_row(const int64_t* __restrict__ offsets, int64_t v, int64_t ni, int64_t& p, int64_t& end) {
    const int64_t o0 = offsets[v], o1 = offsets[v + 1];
    const bool ok = o0 >= 0 && o0 <= o1 && o1 <= ni;
    p = ok ? o0 : 0;
    end = ok ? o1 : 0;
}

__device__ __forceinline__ int64_t head_of(const int32_t* __restrict__ inc, int64_t p, int64_t end) { return p < end ? (int64_t)inc[p] : KEY_SENTINEL; }

__global__ __launch_bounds__(256) void filter_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, const int64_t* __restrict__ offsets,
                                                     const int32_t* __restrict__ inc, int64_t ni, const double* __restrict__ normals, double T,
                                                     double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const int64_t a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
    if (!face_valid(a, b, c, nv)) {                          // no neighbourhood, and its rows are never opened
        out[3 * i] = 0.0;
        out[3 * i + 1] = 0.0;
        out[3 * i + 2] = 0.0;
        return;
    }
    const double n[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    int64_t pa, ea, pb, eb, pc, ec;
    open_row(offsets, a, ni, pa, ea);
    open_row(offsets, b, ni, pb, eb);
    open_row(offsets, c, ni, pc, ec);
    int64_t ha = head_of(inc, pa, ea), hb = head_of(inc, pb, eb), hc = head_of(inc, pc, ec);
    double acc[3] = {0.0, 0.0, 0.0};
    for (;;) {                                               // at most (ea - pa) + (eb - pb) + (ec - pc) turns: every turn advances a cursor
        int64_t j = ha < hb ? ha : hb;
        j = hc < j ? hc : j;
        if (j == KEY_SENTINEL) break;                        // all three rows are used up
        if (ha == j) { ++pa; ha = head_of(inc, pa, ea); }    // every row that shows j moves on: j is visited once
        if (hb == j) { ++pb; hb = head_of(inc, pb, eb); }
        if (hc == j) { ++pc; hc = head_of(inc, pc, ec); }
        if (j < 0 || j >= nf) continue;                      // no face: skipped, never read
        const double m[3] = {normals[3 * j], normals[3 * j + 1], normals[3 * j + 2]};
        const double d = dot3(n, m);
        if (d > T) {                                         // false for a NaN
            const double w = (d - T) * (d - T);
            acc[0] = acc[0] + w * m[0];
            acc[1] = acc[1] + w * m[1];
            acc[2] = acc[2] + w * m[2];
        }
    }
    store_unit_or(acc, n, out + 3 * i);
}

__global__ __launch_bounds__(256) void vertex_kernel(const double* __restrict__ x, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                     const double* __restrict__ normals, const int64_t* __restrict__ offsets,
                                                     const int32_t* __restrict__ inc, int64_t ni, double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const double xv[3] = {x[3 * v], x[3 * v + 1], x[3 * v + 2]};
    double r[3] = {xv[0], xv[1], xv[2]};
    const int64_t o0 = offsets[v], o1 = offsets[v + 1];
    if (o0 >= 0 && o0 <= o1 && o1 <= ni) {                  // a row outside [0, ni] is skipped, never read
        double acc[3] = {0.0, 0.0, 0.0};
        int64_t cnt = 0;
        for (int64_t e = o0; e < o1; ++e) {                 // row order = ascending face index
            const int64_t k = inc[e];
            if (k < 0 || k >= nf) continue;
            const int64_t a = faces[3 * k], b = faces[3 * k + 1], c = faces[3 * k + 2];
            if (!face_valid(a, b, c, nv) || (a != v && b != v && c != v)) continue;          // an invalid face, or one that does not hold v
            const double nk[3] = {normals[3 * k], normals[3 * k + 1], normals[3 * k + 2]};
            double dv[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double ck = ((x[3 * a + q] + x[3 * b + q]) + x[3 * c + q]) / 3.0;
                dv[q] = ck - xv[q];
            }
            const double t = dot3(nk, dv);
            acc[0] = acc[0] + nk[0] * t;
            acc[1] = acc[1] + nk[1] * t;
            acc[2] = acc[2] + nk[2] * t;
            ++cnt;
        }
        if (cnt > 0) {
            const double d = (double)cnt;
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q] = xv[q] + acc[q] / d;
        }
    }
    out[3 * v] = r[0];
    out[3 * v + 1] = r[1];
    out[3 * v + 2] = r[2];
}

bool counts_ok(int64_t nv, int64_t nf, int64_t ni) {
    return nv >= 0 && nf >= 0 && ni >= 0 && nv <= (int64_t)INT32_MAX && nf <= (int64_t)INT32_MAX;
}

}  // namespace

extern "C" {

int ppsx_denoise_face_normals(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, double* normals, void* stream) {
    if (!counts_ok(nv, nf, 0)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !normals || (nv > 0 && !verts)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(face_normals_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, faces, nf, normals);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_denoise_filter_pass(const int64_t* faces, int64_t nf, int64_t nv, const int64_t* offsets, const int32_t* inc, int64_t ni,
                             const double* normals, double threshold, double* out, void* stream) {
    if (!counts_ok(nv, nf, ni) || !(threshold >= 0.0 && threshold < 1.0)) return PPS_ERR_ARG;          // a NaN threshold fails both
    if (nf == 0) return PPS_OK;
    if (!faces || !normals || !out || normals == out || (nv > 0 && !offsets) || (ni > 0 && !inc)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, offsets, inc, ni,
                       normals, threshold, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_denoise_vertex_pass(const double* x, int64_t nv, const int64_t* faces, int64_t nf, const double* normals, const int64_t* offsets,
                             const int32_t* inc, int64_t ni, double* out, void* stream) {
    if (!counts_ok(nv, nf, ni)) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    if (!x || !offsets || !out || x == out || (nf > 0 && (!faces || !normals)) || (ni > 0 && !inc)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(vertex_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, nv, faces, nf, normals, offsets,
                       inc, ni, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
