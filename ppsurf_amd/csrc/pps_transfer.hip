// Colour transfer from a scan to a mesh for gfx950: inverse-squared-distance blend of the colours of the k nearest scan points (DESIGN.md
// section 14).
//
// new capability: replaces nothing -- the reference writes uncoloured meshes (source/poco_model.py:269 `mesh.export`).  Driven by
// ppsurf_amd/transfer.py; restated in numpy by tests/transfer_spec.py, which the kernel matches bit for bit.
//
// Per vertex i, channels c = 0..3, neighbours j = 0..k-1 IN COLUMN ORDER, all in fp64, each operation rounded on its own (-ffp-contract=off:
// the multiply and the add of T are two instructions):
//   t = idx[i,j];  skipped unless 0 <= t < n  (a skipped neighbour adds nothing, not even a zero)
//   w = 1.0 / (double(d2[i,j]) + eps);  S = S + w;  T[c] = T[c] + w * double(rgba[t,c])
//   S == 0 -> out[i,:] = 0;  otherwise out[i,c] = u8(min(255, max(0, floor(T[c] / S + 0.5))))
// With eps = 1e-30 a vertex that sits on a scan point (d2 = 0) weighs it 1e30 against at most ~1e12 for the others and takes its colour
// exactly; nothing is ever infinite.
//
// Shape: the fixed order of the sums makes the row the unit of work -- one lane owns one vertex and walks its k columns; a reduction across
// lanes would change the order.  The RGBA row makes each gather one dword load and each result one dword store, 64 consecutive dwords per
// wave.  A lane's row of idx (8 k bytes) and of d2 (4 k bytes) is contiguous, so the cache lines a wave touches at column j serve its next
// columns too; the columns are unrolled by four to keep four independent gathers in flight per lane.  The index test is the bounds guard:
// nothing is read outside rgba.  No atomics, no LDS; 256 threads per workgroup, a few dozen VGPRs, so occupancy is bounded by the grid
// (m / 64 waves), not by registers.
#include "pps_common.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

__device__ __forceinline__ uint32_t to_u8(double t, double s) {
    const double y = floor(t / s + 0.5);
    return y > 0.0 ? (y < 255.0 ? (uint32_t)y : 255u) : 0u;          // a NaN goes to 0
}

__global__ __launch_bounds__(256) void blend_rgba_kernel(const int64_t* __restrict__ idx, const float* __restrict__ d2, int64_t m, int k,
                                                         const uint32_t* __restrict__ rgba, int64_t n, double eps, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t* ti = idx + i * (int64_t)k;
    const float* di = d2 + i * (int64_t)k;
    double S = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0, T3 = 0.0;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
        const int64_t t = ti[j];
        const float d = di[j];
        if (t >= 0 && t < n) {
            const uint32_t px = rgba[t];                              // little-endian: byte c of the row is bits 8 c .. 8 c + 7
            const double w = 1.0 / ((double)d + eps);
            S = S + w;
            T0 = T0 + w * (double)(px & 0xFFu);
            T1 = T1 + w * (double)((px >> 8) & 0xFFu);
            T2 = T2 + w * (double)((px >> 16) & 0xFFu);
            T3 = T3 + w * (double)(px >> 24);
        }
    }
    uint32_t q = 0u;
    if (S != 0.0) q = to_u8(T0, S) | (to_u8(T1, S) << 8) | (to_u8(T2, S) << 16) | (to_u8(T3, S) << 24);
    out[i] = q;
}

}  // namespace

extern "C" {

int ppsx_blend_rgba_u8(const int64_t* idx, const float* d2, int64_t m, int k, const uint8_t* rgba, int64_t n, double eps, uint8_t* out,
                       void* stream) {
    if (m < 0 || n < 0 || k < 1 || k > 256 || !(eps > 0.0)) return PPS_ERR_ARG;
    if (m == 0) return PPS_OK;
    if (!idx || !d2 || !rgba || !out || ((uintptr_t)rgba & 3) || ((uintptr_t)out & 3)) return PPS_ERR_ARG;
    if ((m + 255) / 256 > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    hipLaunchKernelGGL(blend_rgba_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, d2, m, k,
                       (const uint32_t*)rgba, n, eps, (uint32_t*)out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
