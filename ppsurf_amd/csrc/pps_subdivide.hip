// Longest-edge bisection for gfx950: every edge longer than a bound is split at its midpoint, in rounds of independent splits (DESIGN.md
// section 28).
//
// new capability: replaces nothing -- the reference has no such stage and every other mesh stage keeps, removes or re-arranges the
// connectivity it is given.  Driven by ppsurf_amd/subdivide.py (the edges and their owners by ppsurf_amd/topology.py); restated in numpy by
// tests/subdivide_spec.py, which the kernels match byte for byte.
//
// The rule, per round: vertices V f32 [nv,3] (finite), the working faces F int64 [nf,3] (a face that was invalid as given holds -1, -1, -1),
// max2 a double.
//   edges      the distinct undirected edges of the valid faces (pps_faces.h) in ascending key (min << 32) | max with their owners: the runs
//              of the edge sort.  The ends a < b of run e are the two halves of its key, its rank is e.  Any owner count >= 1 takes part.
//   candidate  P = double(V).  d = P_b - P_a, len2 = (dx dx + dy dy) + dz dz; M = f32((P_a + P_b) 0.5) per component.  A candidate iff
//              len2 > max2 and M differs from V[a] and from V[b] in some component (the floats compared, so -0 equals 0).  An edge between
//              neighbouring floats is never split, and no new vertex coincides with an end of its edge.
//   priority   one u64, the smallest first, the longest edge first: ((0x7FF00000 - (bits(len2) >> 32)) << 32) | fmix32(e).  The bits of
//              positive doubles are monotone and fmix32 (murmur3's finaliser) is a bijection: no two edges share one.  NONE = 2^64 - 1.
//   choice     every face looks at the priorities of its three edges and takes the slot k of the smallest (slot k is corner k -> corner k + 1
//              mod 3), none when all three are NONE, and casts one vote for that edge.
//   winners    a candidate wins iff its votes equal its owners: every face on it chose it.  Winners share no face (a face votes once), and
//              the smallest priority of all is the smallest in each of its faces, so a round with a candidate splits something.
//   apply      the winners in ascending key get the rows nv + i with position M.  A face whose chosen edge won is a hit; with m the new row,
//              row f becomes the old row with entry k + 1 replaced by m, and the old row with entry k replaced by m is appended at
//              nf + (the rank of f among the hits).  Both are wound like the parent.  Every other row is copied.
// fp64 throughout, every operation rounded on its own (-ffp-contract=off).  No floating-point atomics: the one atomic is an integer add of
// ones, which is exact in any order.  A pure function of (V, F, max2): no dependence on the launch shape or on timing.
//
// Shape: one thread per run or per face, 256 threads per workgroup, plain vector loads and stores, no LDS.  A face finds its edges through
// run_of int64 [3 nf], the run of every unsorted key position (the host scatters it through the sort's permutation); the kernels that work per
// face never read a vertex index as an address.  Every index -- the ends of a key, a run, a slot, a row of the prefix sums -- is range-checked
// before it becomes an address; what fails a check is no candidate, no hit, or a row copied as it is.
#include <math.h>

#include "pps_common.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

typedef unsigned long long u64;

constexpr u64 NONE = ~0ull;
constexpr uint32_t INF_HIGH = 0x7FF00000u;

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// the ends a < b of a key, both in [0, nv); false for the sentinel, a negative key and a key that names no such pair
__device__ __forceinline__ bool key_ends(int64_t key, int64_t nv, int64_t& a, int64_t& b) {
    a = key >> 32;
    b = key & 0xFFFFFFFFll;
    return key >= 0 && a < b && b < nv;
}

__device__ __forceinline__ float midpoint(float p, float q) { return (float)(((double)p + (double)q) * 0.5); }

__global__ __launch_bounds__(256) void edges_kernel(const int64_t* __restrict__ keys, int64_t ne, const float* __restrict__ verts, int64_t nv, double max2,
                                                    double* __restrict__ len2, u64* __restrict__ prio) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    int64_t a, b;
    if (!key_ends(keys[e], nv, a, b)) {
        len2[e] = 0.0;
        prio[e] = NONE;
        return;
    }
    const float ax = verts[3 * a], ay = verts[3 * a + 1], az = verts[3 * a + 2];
    const float bx = verts[3 * b], by = verts[3 * b + 1], bz = verts[3 * b + 2];
    const double dx = (double)bx - (double)ax, dy = (double)by - (double)ay, dz = (double)bz - (double)az;
    const double l2 = (dx * dx + dy * dy) + dz * dz;
    const float mx = midpoint(ax, bx), my = midpoint(ay, by), mz = midpoint(az, bz);
    const bool off_a = mx != ax || my != ay || mz != az, off_b = mx != bx || my != by || mz != bz;
    len2[e] = l2;
    if (!(l2 > max2) || !off_a || !off_b) {
        prio[e] = NONE;
        return;
    }
    const uint32_t high = INF_HIGH - (uint32_t)((u64)__double_as_longlong(l2) >> 32);
    prio[e] = ((u64)high << 32) | (u64)fmix32((uint32_t)e);
}

__global__ __launch_bounds__(256) void votes_kernel(const int64_t* __restrict__ run_of, int64_t nf, const u64* __restrict__ prio, int64_t ne,
                                                    int32_t* __restrict__ choice, int32_t* votes) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    u64 best = NONE;
    int k = -1;
    int64_t at = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t r = run_of[3 * f + j];
        const u64 p = (r >= 0 && r < ne) ? prio[r] : NONE;
        if (p < best) {
            best = p;
            k = j;
            at = r;
        }
    }
    choice[f] = k;
    if (k >= 0) atomicAdd(votes + at, 1);                                         // at lies in [0, ne): its priority was read
}

__global__ __launch_bounds__(256) void winners_kernel(const u64* __restrict__ prio, const int32_t* __restrict__ votes, const int64_t* __restrict__ owners,
                                                      int64_t ne, uint8_t* __restrict__ win) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    win[e] = (prio[e] != NONE && (int64_t)votes[e] == owners[e]) ? 1 : 0;
}

// the run that face f chose when that run won, else -1
__device__ __forceinline__ int64_t won_run(const int64_t* __restrict__ run_of, const int32_t* __restrict__ choice, const uint8_t* __restrict__ win,
                                           int64_t ne, int64_t f) {
    const int k = choice[f];
    if (k < 0 || k > 2) return -1;
    const int64_t r = run_of[3 * f + k];
    return (r >= 0 && r < ne && win[r] != 0) ? r : -1;
}

__global__ __launch_bounds__(256) void hits_kernel(const int64_t* __restrict__ run_of, const int32_t* __restrict__ choice, int64_t nf,
                                                   const uint8_t* __restrict__ win, int64_t ne, uint8_t* __restrict__ hit) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    hit[f] = won_run(run_of, choice, win, ne, f) >= 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void emit_vertices_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ keys,
                                                            const uint8_t* __restrict__ win, const int64_t* __restrict__ vslot, int64_t ne, int64_t nw,
                                                            float* __restrict__ new_verts, int64_t* __restrict__ ends) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne || win[e] == 0) return;
    const int64_t i = vslot[e];
    int64_t a, b;
    if (i < 0 || i >= nw || !key_ends(keys[e], nv, a, b)) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) new_verts[3 * i + j] = midpoint(verts[3 * a + j], verts[3 * b + j]);
    ends[2 * i] = a;
    ends[2 * i + 1] = b;
}

__global__ __launch_bounds__(256) void emit_faces_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, const int64_t* __restrict__ run_of,
                                                         const int32_t* __restrict__ choice, const uint8_t* __restrict__ hit,
                                                         const int64_t* __restrict__ fslot, int64_t nh, const uint8_t* __restrict__ win,
                                                         const int64_t* __restrict__ vslot, int64_t ne, int64_t nw, int64_t* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    int64_t row[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    const int64_t r = hit[f] != 0 ? won_run(run_of, choice, win, ne, f) : -1;
    const int64_t i = r >= 0 ? vslot[r] : -1, j = r >= 0 ? fslot[f] : -1;
    if (i >= 0 && i < nw && j >= 0 && j < nh) {
        const int k = choice[f];                                                  // 0..2: won_run looked
        const int64_t m = nv + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * (nf + j) + c] = c == k ? m : row[c];
        row[(k + 1) % 3] = m;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * f + c] = row[c];
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }
inline bool too_many_runs(int64_t n) { return n > (int64_t)UINT32_MAX; }
inline unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int ppsx_subdivide_edges(const int64_t* keys, int64_t ne, const float* verts, int64_t nv, double max2, double* len2, uint64_t* prio, void* stream) {
    if (ne < 0 || nv < 0 || too_many_runs(ne) || too_many(nv) || max2 != max2) return PPS_ERR_ARG;
    if (ne == 0) return PPS_OK;
    if (!keys || !len2 || !prio || (nv > 0 && !verts)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(edges_kernel, dim3(grid_of(ne, 256)), dim3(256), 0, (hipStream_t)stream, keys, ne, verts, nv, max2, len2, (u64*)prio);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_subdivide_votes(const int64_t* run_of, int64_t nf, const uint64_t* prio, int64_t ne, int32_t* choice, int32_t* votes, void* stream) {
    if (nf < 0 || ne < 0 || too_many(nf) || too_many_runs(ne)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!run_of || !choice || (ne > 0 && (!prio || !votes))) return PPS_ERR_ARG;
    hipLaunchKernelGGL(votes_kernel, dim3(grid_of(nf, 256)), dim3(256), 0, (hipStream_t)stream, run_of, nf, (const u64*)prio, ne, choice, votes);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_subdivide_winners(const uint64_t* prio, const int32_t* votes, const int64_t* owners, int64_t ne, uint8_t* win, void* stream) {
    if (ne < 0 || too_many_runs(ne)) return PPS_ERR_ARG;
    if (ne == 0) return PPS_OK;
    if (!prio || !votes || !owners || !win) return PPS_ERR_ARG;
    hipLaunchKernelGGL(winners_kernel, dim3(grid_of(ne, 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)prio, votes, owners, ne, win);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_subdivide_hits(const int64_t* run_of, const int32_t* choice, int64_t nf, const uint8_t* win, int64_t ne, uint8_t* hit, void* stream) {
    if (nf < 0 || ne < 0 || too_many(nf) || too_many_runs(ne)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!run_of || !choice || !hit || (ne > 0 && !win)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(hits_kernel, dim3(grid_of(nf, 256)), dim3(256), 0, (hipStream_t)stream, run_of, choice, nf, win, ne, hit);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_subdivide_emit(const float* verts, int64_t nv, const int64_t* keys, const uint8_t* win, const int64_t* vslot, int64_t ne, int64_t nw,
                        const int64_t* faces, int64_t nf, const int64_t* run_of, const int32_t* choice, const uint8_t* hit, const int64_t* fslot,
                        int64_t nh, float* new_verts, int64_t* ends, int64_t* out, void* stream) {
    if (nv < 0 || ne < 0 || nw < 0 || nf < 0 || nh < 0 || too_many(nv) || too_many_runs(ne) || too_many(nf) || nw > ne || nh > nf) return PPS_ERR_ARG;
    if (too_many(nv + nw) || too_many(nf + nh) || (out && out == faces)) return PPS_ERR_ARG;
    if (ne > 0 && (!keys || !win || !vslot || (nv > 0 && !verts) || (nw > 0 && (!new_verts || !ends)))) return PPS_ERR_ARG;
    if (nf > 0 && (!faces || !run_of || !choice || !hit || !fslot || !out)) return PPS_ERR_ARG;
    if (ne > 0 && nw > 0)
        hipLaunchKernelGGL(emit_vertices_kernel, dim3(grid_of(ne, 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, keys, win, vslot, ne, nw, new_verts,
                           ends);
    if (nf > 0)
        hipLaunchKernelGGL(emit_faces_kernel, dim3(grid_of(nf, 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, run_of, choice, hit, fslot, nh, win,
                           vslot, ne, nw, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
