// Orientation for gfx950: a coherent winding per face component, outward where the component is closed.
//
// new capability: replaces nothing -- the reference has no such stage and every other mesh stage takes the winding as it comes.  Driven by
// ppsurf_amd/orient.py (the pairs and their edge slots by ppsurf_amd/topology.py); restated in numpy by tests/orient_spec.py, which the
// kernels match byte for byte.
//
// The rule: vertices V f32 [nv,3] (finite), faces F int64 [nf,3], nv, nf <= 2^31 - 1, mode in {outward, inward, majority}.
//   valid face, adjacency, component, leader   as in pps_pieces.hip: face_valid of pps_faces.h; two valid faces are adjacent across an
//                 undirected edge that EXACTLY TWO valid faces hold; the leader is the smallest face index of the component.
//   pair sign     slot k of a face is the directed edge corner k -> corner k + 1 mod 3.  A pair (fa, fb) with the edge in the slots
//                 (ea, eb) has s = 1 when F[fa][ea] == F[fb][eb]: both run the edge the same way, one of them must turn; s = 0 when they
//                 run it in opposite directions (coherent).  The slots are sort positions % 3, never a comparison of corners: two copies of
//                 one free triangle are a pair three times over.
//   flip          in an orientable component flip[f] = the XOR of s along any path from the leader (flip[leader] = 0).  A component where
//                 some pair has flip[a] ^ flip[b] != s is NOT ORIENTABLE: it comes back byte for byte.
//   decision      per orientable component, T = its faces with flip 1, U = those with flip 0.  majority: turn the smaller, T on a tie.
//                 outward / inward, the component closed (2 pairs == 3 faces): outward turns T when V > 0 and U when V < 0, inward the
//                 opposite; V == 0 and every open component take the majority.  (host, on the tables of counts and volumes)
//   V             six times the signed volume with the flips applied, fp64, every operation rounded on its own (-ffp-contract=off), no
//                 floating-point atomics: R = the first corner of the leader as given, q_k = double(P_k) - double(R), the term of a face
//                 t = ((q0x (q1y q2z - q1z q2y)) + (q0y (q1z q2x - q1x q2z))) + (q0z (q1x q2y - q1y q2x)), negated when flip = 1.  The
//                 faces of a component in ascending index; position j lies in block j / 256; lane l = (j % 256) / 4 adds its four terms
//                 in order from +0.0 (absent: +0.0); then S[l] = S[l] + S[l + s] for s = 1, 2, 4, 8, 16, 32 and l a multiple of 2 s; the
//                 block sums of a component are added in ascending order from +0.0.
//   output        a turned face (a, b, c) becomes (a, c, b); every other row, the invalid ones included, is copied.
// A pure function of (V, F, mode): no dependence on the launch shape or on timing.
//
// Labelling with a parity (hook_kernel, compress_kernel) over the pairs fa, fb, s.  word[f] = (parent << 1) | flip of f relative to that
// parent, one int64 per face; it starts as f << 1 and is -1 for an invalid face, which is never touched.  The loop is the labelling
// layer's (labels.fixed_point) and the argument is that of pps_labels.h with the parent part of a word as the label; the walk, the hook
// and the compress are this file's own because the state is a different word.  What the parity adds:
//   hook      a pair (a, b, s) walks from a and from b to the ends (ra, qa), (rb, qb): a walk steps from x to its parent p while
//             0 <= p < x and XORs the flips it passes.  When ra != rb: atomicMin(&word[max(ra, rb)], (min(ra, rb) << 1) | (qa ^ qb ^ s))
//             and the flag goes up (whenever the ends differ, as in pps_pieces.hip).
//   compress  every face stores (the end of its walk << 1) | the parity of that walk in its own slot.
//   skipped   a pair entry outside [0, nf) or onto a face with a negative word.
//   I1  holds for the packed words too: a root's word is x << 1 and (min << 1) | 1 < max << 1, so a hook stores a parent below the slot.
//   I3  in an orientable component the flip of word[f] is flip[f] ^ flip[parent(f)].   It holds at the start (0 to itself).  A walk XORs
//                                             such relations, so its parity is flip[start] ^ flip[end]; the hook's value states
//                                             flip[max] ^ flip[min] = qa ^ qb ^ s because flip[a] ^ flip[b] = s; compress stores a walk's.
//   The parent parts order the packed words (the flip is the lowest bit), so they evolve exactly as the labels of pps_pieces.hip: an
//   atomicMin lowers the parent when the new one is smaller, and between two values with one parent it keeps the flip 0 -- by I3 both
//   flips are equal in an orientable component, and in a non-orientable one no flip is used.  The fixed point therefore has the leaders of
//   face_components, and the rounds are those of the labels without a parity: the parity adds no dependency.
//   Every word is read by ONE relaxed device-scope atomic load of 8 bytes, so parent and flip come from the same snapshot; a stale read
//   returns an earlier word, which by I1 - I3 states a true relation as well.  At the fixed point the compress before made every word
//   (root << 1) | parity of the walk to it, and by I3 that parity is flip[f] ^ flip[leader] = flip[f].
//   In a non-orientable component the flips depend on the path and so on timing; check_kernel only establishes that some pair fails.
//
// Shape: pair_sign, hook and check one thread per pair; compress and apply one thread per face; block_sums one wave per block of 256
// positions (four blocks per workgroup, four gathered faces per lane, the tree by shuffles, no LDS); comp_sums one thread per component.
// Every index is range-checked before it becomes an address.  The atomics are ordinary device-scope vector atomics.
#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

constexpr int SUM_BLOCK = 256;                              // positions per block of the volume sum: 64 lanes of four

__device__ __forceinline__ int64_t load_word(const int64_t* word, int64_t x) {
    return __hip_atomic_load(word + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct End {
    int64_t x;                                              // the end of the walk
    int64_t q;                                              // the XOR of the flips passed
};

// the end of the walk from x (0 <= x < nf, by the caller): it steps to the parent p of x while 0 <= p < x
__device__ __forceinline__ End walk_end(const int64_t* word, int64_t x) {
    int64_t q = 0;
    for (;;) {
        const int64_t w = load_word(word, x);
        const int64_t p = w >> 1;
        if (w < 0 || p >= x) return End{x, q};
        q ^= w & 1;
        x = p;
    }
}

// the pair i when both faces lie in [0, nf)
__device__ __forceinline__ bool pair_in_range(const int32_t* fa, const int32_t* fb, int64_t i, int64_t nf, int& a, int& b) {
    a = fa[i];
    b = fb[i];
    return a >= 0 && a < nf && b >= 0 && b < nf;
}

__global__ __launch_bounds__(256) void pair_sign_kernel(const int64_t* __restrict__ faces, int64_t nf, const int32_t* __restrict__ fa,
                                                        const int32_t* __restrict__ fb, const int32_t* __restrict__ ea,
                                                        const int32_t* __restrict__ eb, int64_t np, uint8_t* __restrict__ sign) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    int a, b;
    const int ka = ea[i], kb = eb[i];
    uint8_t s = 0;
    if (pair_in_range(fa, fb, i, nf, a, b) && ka >= 0 && ka < 3 && kb >= 0 && kb < 3) s = faces[3 * (int64_t)a + ka] == faces[3 * (int64_t)b + kb] ? 1 : 0;
    sign[i] = s;
}

__global__ __launch_bounds__(256) void hook_kernel(const int32_t* __restrict__ fa, const int32_t* __restrict__ fb, const uint8_t* __restrict__ sign,
                                                   int64_t np, int64_t* word, int64_t nf, int32_t* changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    int a, b;
    if (!pair_in_range(fa, fb, i, nf, a, b)) return;
    if (load_word(word, a) < 0 || load_word(word, b) < 0) return;              // onto an invalid face
    const End ra = walk_end(word, a), rb = walk_end(word, b);
    if (ra.x == rb.x) return;
    const int64_t q = ra.q ^ rb.q ^ (int64_t)(sign[i] & 1);
    const int64_t hi = ra.x > rb.x ? ra.x : rb.x, lo = ra.x > rb.x ? rb.x : ra.x;
    __hip_atomic_fetch_min(word + hi, (lo << 1) | q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *changed = 1;
}

__global__ __launch_bounds__(256) void compress_kernel(int64_t* word, int64_t nf) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    if (load_word(word, f) < 0) return;                     // an invalid face is never touched
    const End e = walk_end(word, f);
    word[f] = (e.x << 1) | e.q;
}

__global__ __launch_bounds__(256) void check_kernel(const int32_t* __restrict__ fa, const int32_t* __restrict__ fb, const uint8_t* __restrict__ sign,
                                                    int64_t np, const int64_t* word, int64_t nf, uint8_t* bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    int a, b;
    if (!pair_in_range(fa, fb, i, nf, a, b)) return;
    const int64_t wa = load_word(word, a), wb = load_word(word, b);
    if (wa < 0 || wb < 0) return;
    const int64_t leader = wa >> 1;
    if (leader >= nf) return;
    if (((wa ^ wb) & 1) != (int64_t)(sign[i] & 1)) bad[leader] = 1;
}

// the term of face f about R, +0.0 for a face that cannot be read through
__device__ __forceinline__ double volume_term(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                              const uint8_t* __restrict__ flip, int64_t f, double rx, double ry, double rz) {
    if (f < 0 || f >= nf) return 0.0;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!face_valid(a, b, c, nv)) return 0.0;
    const double q0x = (double)verts[3 * a] - rx, q0y = (double)verts[3 * a + 1] - ry, q0z = (double)verts[3 * a + 2] - rz;
    const double q1x = (double)verts[3 * b] - rx, q1y = (double)verts[3 * b + 1] - ry, q1z = (double)verts[3 * b + 2] - rz;
    const double q2x = (double)verts[3 * c] - rx, q2y = (double)verts[3 * c + 1] - ry, q2z = (double)verts[3 * c + 2] - rz;
    const double t = ((q0x * (q1y * q2z - q1z * q2y)) + (q0y * (q1z * q2x - q1x * q2z))) + (q0z * (q1x * q2y - q1y * q2x));
    return flip[f] == 1 ? -t : t;
}

__global__ __launch_bounds__(256) void block_sums_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                         const uint8_t* __restrict__ flip, const int32_t* __restrict__ list, int64_t nl,
                                                         const int64_t* __restrict__ first, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ lead, int64_t nb, double* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);         // one wave per block: the branch is uniform in the wave
    if (blk >= nb) return;
    const int64_t p0 = first[blk];
    const int n = count[blk];
    const int64_t lf = lead[blk];
    double s = 0.0;
    bool ok = p0 >= 0 && n >= 1 && n <= SUM_BLOCK && p0 <= nl - n && lf >= 0 && lf < nf;
    int64_t r = 0;
    if (ok) {
        r = faces[3 * lf];
        ok = face_valid(r, faces[3 * lf + 1], faces[3 * lf + 2], nv);
    }
    if (ok) {
        const double rx = (double)verts[3 * r], ry = (double)verts[3 * r + 1], rz = (double)verts[3 * r + 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * lane + j;
            s = s + (k < n ? volume_term(verts, nv, faces, nf, flip, list[p0 + k], rx, ry, rz) : 0.0);
        }
    }
#pragma unroll
    for (int stride = 1; stride <= 32; stride <<= 1) s = s + __shfl_down(s, stride);          // lane l, a multiple of 2 stride, adds lane l + stride
    if (lane == 0) sums[blk] = s;
}

__global__ __launch_bounds__(256) void comp_sums_kernel(const double* __restrict__ sums, int64_t nb, const int64_t* __restrict__ start, int64_t nc,
                                                        double* __restrict__ vol) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const int64_t b0 = start[c], b1 = start[c + 1];
    double v = 0.0;
    if (b0 >= 0 && b0 <= b1 && b1 <= nb)
        for (int64_t b = b0; b < b1; ++b) v = v + sums[b];
    vol[c] = v;
}

__global__ __launch_bounds__(256) void apply_kernel(const int64_t* __restrict__ faces, int64_t nf, const int32_t* __restrict__ cid,
                                                    const uint8_t* __restrict__ flip, const uint8_t* __restrict__ turn, int64_t nc,
                                                    int64_t* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const int comp = cid[f];
    bool turned = false;
    if (comp >= 0 && comp < nc) {
        const int t = turn[comp], q = flip[f];
        turned = (t == 1 && q == 1) || (t == 2 && q == 0);
    }
    out[3 * f] = a;
    out[3 * f + 1] = turned ? c : b;
    out[3 * f + 2] = turned ? b : c;
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }
inline unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int ppsx_orient_pair_sign(const int64_t* faces, int64_t nf, const int32_t* fa, const int32_t* fb, const int32_t* ea, const int32_t* eb,
                          int64_t np, uint8_t* sign, void* stream) {
    if (np < 0 || nf < 0 || too_many(np) || too_many(nf)) return PPS_ERR_ARG;
    if (np == 0) return PPS_OK;
    if (!fa || !fb || !ea || !eb || !sign || (nf > 0 && !faces)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(pair_sign_kernel, dim3(grid_of(np, 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, fa, fb, ea, eb, np, sign);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_orient_hook(const int32_t* fa, const int32_t* fb, const uint8_t* sign, int64_t np, int64_t* word, int64_t nf, int32_t* changed,
                     void* stream) {
    if (np < 0 || nf < 0 || too_many(np) || too_many(nf)) return PPS_ERR_ARG;
    if (np == 0 || nf == 0) return PPS_OK;
    if (!fa || !fb || !sign || !word || !changed) return PPS_ERR_ARG;
    hipLaunchKernelGGL(hook_kernel, dim3(grid_of(np, 256)), dim3(256), 0, (hipStream_t)stream, fa, fb, sign, np, word, nf, changed);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_orient_compress(int64_t* word, int64_t nf, void* stream) {
    if (nf < 0 || too_many(nf)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!word) return PPS_ERR_ARG;
    hipLaunchKernelGGL(compress_kernel, dim3(grid_of(nf, 256)), dim3(256), 0, (hipStream_t)stream, word, nf);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_orient_check(const int32_t* fa, const int32_t* fb, const uint8_t* sign, int64_t np, const int64_t* word, int64_t nf, uint8_t* bad,
                      void* stream) {
    if (np < 0 || nf < 0 || too_many(np) || too_many(nf)) return PPS_ERR_ARG;
    if (np == 0 || nf == 0) return PPS_OK;
    if (!fa || !fb || !sign || !word || !bad) return PPS_ERR_ARG;
    hipLaunchKernelGGL(check_kernel, dim3(grid_of(np, 256)), dim3(256), 0, (hipStream_t)stream, fa, fb, sign, np, word, nf, bad);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_orient_block_sums(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const uint8_t* flip, const int32_t* list,
                           int64_t nl, const int64_t* first, const int32_t* count, const int32_t* lead, int64_t nb, double* sums, void* stream) {
    if (nb < 0 || nl < 0 || nv < 0 || nf < 0 || too_many(nb) || too_many(nl) || too_many(nv) || too_many(nf)) return PPS_ERR_ARG;
    if (nb == 0) return PPS_OK;
    if (!first || !count || !lead || !sums || (nl > 0 && !list) || (nf > 0 && (!faces || !flip)) || (nv > 0 && !verts)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(block_sums_kernel, dim3(grid_of(nb, 4)), dim3(256), 0, (hipStream_t)stream, verts, nv, faces, nf, flip, list, nl, first,
                       count, lead, nb, sums);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_orient_comp_sums(const double* sums, int64_t nb, const int64_t* start, int64_t nc, double* vol, void* stream) {
    if (nc < 0 || nb < 0 || too_many(nc) || too_many(nb)) return PPS_ERR_ARG;
    if (nc == 0) return PPS_OK;
    if (!start || !vol || (nb > 0 && !sums)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(comp_sums_kernel, dim3(grid_of(nc, 256)), dim3(256), 0, (hipStream_t)stream, sums, nb, start, nc, vol);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_orient_apply(const int64_t* faces, int64_t nf, const int32_t* cid, const uint8_t* flip, const uint8_t* turn, int64_t nc, int64_t* out,
                      void* stream) {
    if (nf < 0 || nc < 0 || too_many(nf) || too_many(nc) || (faces && faces == out)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !cid || !flip || !out || (nc > 0 && !turn)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(apply_kernel, dim3(grid_of(nf, 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, cid, flip, turn, nc, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
