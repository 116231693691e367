// Isolated pieces for gfx950: the face components of a mesh, a table per component and the rules that drop components.
//
// new capability: replaces nothing -- the reference's only rule is remove_small_connected_components(num_faces = 6), which stays with
// pps_mesh_small_components (pps_mesh.hip, a bounded walk, k <= 32).  Driven by ppsurf_amd/pieces.py (the keys by ppsurf_amd/topology.py);
// restated in numpy by tests/pieces_spec.py, which the kernels match byte for byte.
//
// The rule: vertices V f32 [nv,3] (finite), faces F int64 [nf,3], nv, nf <= 2^31 - 1.
//   valid face    its three indices lie in [0, nv) and are pairwise distinct (face_valid of pps_faces.h).  An invalid face belongs to no
//                 component, is never read through, has the label -1 and is always dropped.
//   adjacency     two valid faces are adjacent when they share an undirected edge that EXACTLY TWO valid faces hold (the product's own rule:
//                 pps_mesh_small_components, oracle.mesh_oracle.components_union_find).  An edge with one owner joins nothing, an edge with
//                 three or more owners joins nothing, a duplicated face counts as two faces.
//   component     a class of the transitive closure of adjacency; its leader is its smallest face index; label[f] = the leader of f's
//                 component (int32).  Components are numbered 0 .. nc - 1 in ascending leader.
//   table         per component: faces, the count (int64); lo, hi f32 [3], the box of the corners of its faces, every coordinate loaded as
//                 x + 0.0f (-0.0 becomes +0.0, which fixes the bytes); diag2 fp64 = (dx dx + dy dy) + dz dz with dx = double(hi.x) -
//                 double(lo.x) and so on, every operation rounded on its own.  D2 is the same expression over the box of all components
//                 (0 with nc = 0).  No area, no floating-point sum: counts, minima and maxima are exact in any order of accumulation.
//   rules         each optional, a component is kept when it passes every rule given:
//                   min_faces = N       faces >= N
//                   min_diag_frac = F   diag2 >= (F F) D2: two fp64 products, no square root, no fused multiply-add (-ffp-contract=off)
//                   keep_largest = K    rank < K, the rank by faces descending, then leader ascending, over ALL components
//   output        the kept faces in their given order; the vertices no kept face references dropped, order kept, faces re-indexed (host).
// A pure function of (V, F, rules): no dependence on the launch shape or on timing.
//
// Labelling (hook_kernel here, the compress of pps_labels.hip; the argument is written out in pps_labels.h).  A node is a face, a link a
// pair of the list fa, fb int32 [np] (the edges with exactly two owners); label[f] starts as f, -1 for an invalid face.
//   hook      a pair (a, b) walks label from a and from b to the ends ra, rb; when ra != rb: atomicMin(&label[max(ra, rb)], min(ra, rb)) and
//             the flag goes up -- whenever the ends differ, not only when the label fell: a launch that leaves the flag down has issued no
//             atomic at all.
//   skipped   a pair entry outside [0, nf) or onto a face with a negative label.
//
// Statistics (stats_kernel): count, lo and hi by integer atomics -- exact in any order -- after combining on chip.  One destination per
// face would send 7 atomics per face of a one-component sphere to seven addresses.  Per wave: the lanes that share the component of the
// first live lane are reduced by shuffles (identities elsewhere) and leave; that first pass goes to LDS, where the workgroup's 16 waves
// are combined once more when they all name one component, so a workgroup inside one component issues seven atomics; up to PASSES more
// passes handle the other components of a mixed wave, one set of atomics per pass, and what is left after them adds lane by lane.  Float
// minima and maxima go through the order-preserving integer image of the f32 bits (b >= 0 ? b : b ^ 0x7FFFFFFF, its own inverse);
// init_kernel writes the images of +inf / -inf and zero counts before, decode_kernel turns the images back into floats after.
//
// Shape: edge_keys_kernel one thread per face, three 8-byte stores (as half_edges_kernel of pps_smooth.hip); hook_kernel one thread per pair;
// stats_kernel 1024 threads, one per face, 576 bytes of LDS (a component number and a box per wave); select_kernel one thread per component.
// Every index is range-checked before it becomes an address.  The atomics are ordinary device-scope vector atomics.
#include <math.h>

#include "pps_common.h"
#include "pps_faces.h"
#include "pps_labels.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

constexpr int STATS_BLOCK = 1024;
constexpr int STATS_WAVES = STATS_BLOCK / 64;
constexpr int PASSES = 7;                                   // wave passes after the first before the lanes left add one by one
constexpr int IMG_POS_INF = 0x7F800000;                     // the image of +inf
constexpr int IMG_NEG_INF = (int)0xFF800000u ^ 0x7FFFFFFF;  // the image of -inf

__device__ __forceinline__ int image_of(float x) {
    const int b = __float_as_int(x + 0.0f);                 // -0.0 -> +0.0
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}

__device__ __forceinline__ float float_of(int image) { return __int_as_float(image >= 0 ? image : image ^ 0x7FFFFFFF); }

__global__ __launch_bounds__(256) void edge_keys_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, int64_t* __restrict__ keys) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool valid = face_valid(a, b, c, nv);
    int64_t* k = keys + 3 * f;
    k[0] = valid ? ((a < b ? a : b) << 32) | (a < b ? b : a) : KEY_SENTINEL;
    k[1] = valid ? ((b < c ? b : c) << 32) | (b < c ? c : b) : KEY_SENTINEL;
    k[2] = valid ? ((c < a ? c : a) << 32) | (c < a ? a : c) : KEY_SENTINEL;
}

__global__ __launch_bounds__(256) void hook_kernel(const int32_t* __restrict__ fa, const int32_t* __restrict__ fb, int64_t np, int32_t* label,
                                                   int64_t nf, int32_t* changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const int a = fa[i], b = fb[i];
    if (a < 0 || a >= nf || b < 0 || b >= nf) return;
    if (load_label(label, a) < 0 || load_label(label, b) < 0) return;          // onto an invalid face
    const int ra = walk_end(label, a), rb = walk_end(label, b);
    if (ra == rb) return;
    atomicMin(label + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    *changed = 1;
}

__global__ __launch_bounds__(256) void stats_init_kernel(int64_t* __restrict__ count, int* __restrict__ lo, int* __restrict__ hi, int64_t nc) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    count[c] = 0;
    lo[3 * c] = lo[3 * c + 1] = lo[3 * c + 2] = IMG_POS_INF;
    hi[3 * c] = hi[3 * c + 1] = hi[3 * c + 2] = IMG_NEG_INF;
}

__global__ __launch_bounds__(256) void stats_decode_kernel(int* __restrict__ lo, int* __restrict__ hi, int64_t n3) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    lo[i] = __float_as_int(float_of(lo[i]));
    hi[i] = __float_as_int(float_of(hi[i]));
}

struct Box {
    int lo[3], hi[3];
    long long n;
};

__device__ __forceinline__ void add_box(int64_t* count, int* lo, int* hi, int c, const Box& b) {
    atomicAdd((unsigned long long*)(count + c), (unsigned long long)b.n);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(lo + 3 * (int64_t)c + k, b.lo[k]);
        atomicMax(hi + 3 * (int64_t)c + k, b.hi[k]);
    }
}

// the box of the lanes with `member` set, in every lane; the others count as identities
__device__ __forceinline__ Box wave_box(const Box& mine, bool member) {
    Box r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int l = member ? mine.lo[k] : INT32_MAX, h = member ? mine.hi[k] : INT32_MIN;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            l = min(l, __shfl_xor(l, s));
            h = max(h, __shfl_xor(h, s));
        }
        r.lo[k] = l;
        r.hi[k] = h;
    }
    long long n = member ? mine.n : 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) n += __shfl_xor(n, s);
    r.n = n;
    return r;
}

__global__ __launch_bounds__(STATS_BLOCK) void stats_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                            const int32_t* __restrict__ label, const int32_t* __restrict__ cid, int64_t nc,
                                                            int64_t* count, int* lo, int* hi) {
    __shared__ int s_cid[STATS_WAVES];
    __shared__ Box s_box[STATS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * STATS_BLOCK + threadIdx.x;
    int c = -1;
    Box mine;
    mine.n = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { mine.lo[k] = INT32_MAX; mine.hi[k] = INT32_MIN; }
    if (f < nf && label[f] >= 0) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], d = faces[3 * f + 2];
        const int cf = cid[f];
        if (face_valid(a, b, d, nv) && cf >= 0 && cf < nc) {
            c = cf;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int ia = image_of(verts[3 * a + k]), ib = image_of(verts[3 * b + k]), id = image_of(verts[3 * d + k]);
                mine.lo[k] = min(ia, min(ib, id));
                mine.hi[k] = max(ia, max(ib, id));
            }
        }
    }
    // the first pass: the component of the first live lane; it goes to LDS for the workgroup's combine
    unsigned long long live = __ballot(c >= 0);
    int lead = -1;
    Box first;
    first.n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { first.lo[k] = INT32_MAX; first.hi[k] = INT32_MIN; }
    if (live) {
        lead = __shfl(c, __ffsll((long long)live) - 1);
        const bool member = c == lead;
        first = wave_box(mine, member);
        if (member) c = -1;
    }
    if (lane == 0) {
        s_cid[wave] = lead;
        s_box[wave] = first;
    }
    // the other components of a mixed wave: one set of atomics per pass, then lane by lane
    for (int pass = 0; pass < PASSES; ++pass) {
        live = __ballot(c >= 0);
        if (!live) break;
        const int src = __ffsll((long long)live) - 1;
        const int other = __shfl(c, src);
        const bool member = c == other;
        const Box b = wave_box(mine, member);
        if (lane == src) add_box(count, lo, hi, other, b);
        if (member) c = -1;
    }
    if (c >= 0) add_box(count, lo, hi, c, mine);
    __syncthreads();
    if (wave != 0) return;
    // wave 0: lane w holds the first pass of wave w; one set of atomics when every wave that had a live lane names the same component
    const bool slot = lane < STATS_WAVES && s_cid[lane < STATS_WAVES ? lane : 0] >= 0;
    const int sc = slot ? s_cid[lane] : -1;
    Box sb = first;
    if (slot) sb = s_box[lane];
    const unsigned long long slots = __ballot(slot);
    if (!slots) return;
    const int src = __ffsll((long long)slots) - 1;
    const int common = __shfl(sc, src);
    const bool same = __ballot(slot && sc != common) == 0;
    if (same) {
        const Box all = wave_box(sb, slot);
        if (lane == src) add_box(count, lo, hi, common, all);
    } else if (slot) {
        add_box(count, lo, hi, sc, sb);
    }
}

__global__ __launch_bounds__(256) void select_kernel(const int64_t* __restrict__ count, const float* __restrict__ lo, const float* __restrict__ hi,
                                                     const int64_t* __restrict__ rank, int64_t nc, int has_min_faces, int64_t min_faces,
                                                     int has_min_diag_frac, double min_diag_frac, int has_keep_largest, int64_t keep_largest,
                                                     double box_diag2, uint8_t* __restrict__ keep) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    bool ok = true;
    if (has_min_faces) ok = ok && count[c] >= min_faces;
    if (has_min_diag_frac) {
        const double dx = (double)hi[3 * c] - (double)lo[3 * c], dy = (double)hi[3 * c + 1] - (double)lo[3 * c + 1],
                     dz = (double)hi[3 * c + 2] - (double)lo[3 * c + 2];
        const double diag2 = (dx * dx + dy * dy) + dz * dz;
        ok = ok && diag2 >= (min_diag_frac * min_diag_frac) * box_diag2;
    }
    if (has_keep_largest) ok = ok && rank[c] >= 0 && rank[c] < keep_largest;
    keep[c] = ok ? 1 : 0;
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }

}  // namespace

extern "C" {

int ppsx_pieces_edge_keys(const int64_t* faces, int64_t nf, int64_t nv, int64_t* keys, void* stream) {
    if (nf < 0 || nv < 0 || too_many(nv) || too_many(nf)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !keys) return PPS_ERR_ARG;
    hipLaunchKernelGGL(edge_keys_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, keys);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_pieces_hook(const int32_t* fa, const int32_t* fb, int64_t np, int32_t* label, int64_t nf, int32_t* changed, void* stream) {
    if (np < 0 || nf < 0 || too_many(nf) || too_many(np)) return PPS_ERR_ARG;
    if (np == 0 || nf == 0) return PPS_OK;
    if (!fa || !fb || !label || !changed) return PPS_ERR_ARG;
    hipLaunchKernelGGL(hook_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fa, fb, np, label, nf, changed);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_pieces_stats(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int32_t* label, const int32_t* cid, int64_t nc,
                      int64_t* count, float* lo, float* hi, void* stream) {
    if (nv < 0 || nf < 0 || nc < 0 || too_many(nv) || too_many(nf) || too_many(nc)) return PPS_ERR_ARG;
    if (nc == 0) return PPS_OK;
    if (!count || !lo || !hi || lo == hi || (nf > 0 && (!faces || !label || !cid)) || (nf > 0 && nv > 0 && !verts)) return PPS_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, count, (int*)lo, (int*)hi, nc);
    if (nf > 0 && nv > 0)
        hipLaunchKernelGGL(stats_kernel, dim3((unsigned)((nf + STATS_BLOCK - 1) / STATS_BLOCK)), dim3(STATS_BLOCK), 0, s, verts, nv, faces, nf, label,
                           cid, nc, count, (int*)lo, (int*)hi);
    hipLaunchKernelGGL(stats_decode_kernel, dim3((unsigned)((3 * nc + 255) / 256)), dim3(256), 0, s, (int*)lo, (int*)hi, 3 * nc);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_pieces_select(const int64_t* count, const float* lo, const float* hi, const int64_t* rank, int64_t nc, int has_min_faces,
                       int64_t min_faces, int has_min_diag_frac, double min_diag_frac, int has_keep_largest, int64_t keep_largest,
                       double box_diag2, uint8_t* keep, void* stream) {
    if (nc < 0 || too_many(nc) || (has_min_faces != 0 && has_min_faces != 1) || (has_min_diag_frac != 0 && has_min_diag_frac != 1) ||
        (has_keep_largest != 0 && has_keep_largest != 1) || !(has_min_faces || has_min_diag_frac || has_keep_largest))
        return PPS_ERR_ARG;
    if (has_min_faces && (min_faces < 1 || too_many(min_faces))) return PPS_ERR_ARG;
    if (has_min_diag_frac && !(min_diag_frac >= 0.0 && min_diag_frac <= 1.0)) return PPS_ERR_ARG;          // false for a NaN
    if (has_keep_largest && (keep_largest < 1 || too_many(keep_largest))) return PPS_ERR_ARG;
    if (!(box_diag2 >= 0.0 && box_diag2 < (double)INFINITY)) return PPS_ERR_ARG;
    if (nc == 0) return PPS_OK;
    if (!keep || (has_min_faces && !count) || (has_min_diag_frac && (!lo || !hi)) || (has_keep_largest && !rank)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, count, lo, hi, rank, nc, has_min_faces,
                       min_faces, has_min_diag_frac, min_diag_frac, has_keep_largest, keep_largest, box_diag2, keep);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
