// Taubin lambda|mu smoothing for gfx950: half-edge keys of a mesh and one Jacobi pass over its vertices.
//
// new capability: replaces nothing -- the reference has no smoothing.  Driven by ppsurf_amd/smooth.py; restated in numpy by
// tests/smooth_spec.py, which the kernels match bit for bit.
//
// Rule: vertices V f32 [nv,3], faces int64 [nf,3], iters >= 0, lam, mu (fp64).
//   valid face    its three indices lie in [0, nv) and are pairwise distinct (face_valid of pps_faces.h).  Invalid faces take no part and are
//                 never read through.
//   half-edges    a valid face (a, b, c) contributes a->b, b->a, b->c, c->b, c->a, a->c.  The multiplicity c(i->j) is the number of times
//                 i->j occurs = the number of valid faces that hold the edge {i, j} (a duplicated face counts twice).
//   border        an edge of multiplicity 1 is a border edge; a vertex with at least one border half-edge is a border vertex.
//   neighbours    an interior vertex takes every distinct j with a half-edge i->j; a border vertex only those j whose half-edge i->j is a
//                 border edge (VCG's rule: a border relaxes along itself).  Edges of three or more faces are interior edges.  A vertex
//                 without a valid face has no neighbours and keeps its bytes.
//   pass(s)       a Jacobi step, everything read from the old positions.  For every vertex with |N| > 0, per component in fp64:
//                 acc = 0.0; acc = acc + x_j for j in N(i) in ASCENDING j; m = acc / double(|N|) (a division); x_i' = x_i + s * (m - x_i).
//                 Every operation rounded on its own (-ffp-contract=off).
//   iteration     pass(lam), then pass(mu).  The state is fp64: the widened f32 input, rounded to f32 (nearest-even) once after the last
//                 iteration by the caller.
// The result is a pure function of (V, F, iters, lam, mu): no float atomics, and the summation order is the order of the sorted keys.
//
// Between the two kernels the caller sorts the keys, takes the distinct ones with their counts and drops the sentinel: the distinct keys in
// ascending order ARE the adjacency rows with ascending neighbours, the counts are the multiplicities (ppsurf_amd/smooth.py).
//
// Shape: half_edges_kernel one thread per face, six 8-byte stores.  pass_kernel one thread per vertex: the sum of a row is sequential by
// rule, so a vertex is one lane's work; it walks its row twice (once over mult for the border flag, once over nbr / mult / x for the sum).
// Plain vector loads and stores, no LDS, no atomics.  Every offset and neighbour read is range-checked before it becomes an address.
#include <math.h>

#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

__global__ __launch_bounds__(256) void half_edges_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, int64_t* __restrict__ keys) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool valid = face_valid(a, b, c, nv);
    int64_t* k = keys + 6 * f;
    k[0] = valid ? (a << 32) | b : KEY_SENTINEL;
    k[1] = valid ? (b << 32) | a : KEY_SENTINEL;
    k[2] = valid ? (b << 32) | c : KEY_SENTINEL;
    k[3] = valid ? (c << 32) | b : KEY_SENTINEL;
    k[4] = valid ? (c << 32) | a : KEY_SENTINEL;
    k[5] = valid ? (a << 32) | c : KEY_SENTINEL;
}

__global__ __launch_bounds__(256) void pass_kernel(const double* __restrict__ x, int64_t nv, const int64_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ nbr, const int32_t* __restrict__ mult, int64_t ne, double s,
                                                   double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const double xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
    double r[3] = {xi[0], xi[1], xi[2]};
    const int64_t o0 = offsets[i], o1 = offsets[i + 1];
    if (o0 >= 0 && o0 <= o1 && o1 <= ne) {                  // a row outside [0, ne] is skipped, never read
        bool border = false;
        for (int64_t e = o0; e < o1; ++e) border = border || mult[e] == 1;
        double acc[3] = {0.0, 0.0, 0.0};
        int64_t cnt = 0;
        for (int64_t e = o0; e < o1; ++e) {                 // row order = ascending neighbour
            const int64_t j = nbr[e];
            if (j < 0 || j >= nv || (border && mult[e] != 1)) continue;
            acc[0] = acc[0] + x[3 * j];
            acc[1] = acc[1] + x[3 * j + 1];
            acc[2] = acc[2] + x[3 * j + 2];
            ++cnt;
        }
        if (cnt > 0) {
            const double d = (double)cnt;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double m = acc[k] / d;
                r[k] = xi[k] + s * (m - xi[k]);
            }
        }
    }
    out[3 * i] = r[0];
    out[3 * i + 1] = r[1];
    out[3 * i + 2] = r[2];
}

}  // namespace

extern "C" {

int ppsx_smooth_half_edges(const int64_t* faces, int64_t nf, int64_t nv, int64_t* keys, void* stream) {
    if (nf < 0 || nv < 0 || nv > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    const int64_t blocks = (nf + 255) / 256;
    if (!faces || !keys || blocks > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    hipLaunchKernelGGL(half_edges_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, keys);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_smooth_pass(const double* x, int64_t nv, const int64_t* offsets, const int32_t* nbr, const int32_t* mult, int64_t ne, double s,
                     double* out, void* stream) {
    if (nv < 0 || ne < 0 || !isfinite(s)) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    const int64_t blocks = (nv + 255) / 256;
    if (!x || !offsets || !out || x == out || (ne > 0 && (!nbr || !mult)) || blocks > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    hipLaunchKernelGGL(pass_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, nv, offsets, nbr, mult, ne, s, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
