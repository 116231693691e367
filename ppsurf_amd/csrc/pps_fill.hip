// Hole filling for gfx950: the rim half-edges of a mesh, the lengths of its border loops and the faces that close them.
//
// new capability: replaces nothing -- the reference has no mesh repair.  Driven by ppsurf_amd/fill.py and topology.rim_rows; restated in numpy
// by tests/fill_spec.py, which the kernels match bit for bit.
//
// Rule: vertices V f32 [nv,3], faces F int64 [nf,3], max_edges an integer in 3..4096.
//   valid face      its three indices lie in [0, nv) and are pairwise distinct (face_valid of pps_faces.h).  Invalid faces take no part and
//                   are never read through.  The multiplicity of an edge {i, j} is the number of valid faces that hold it (a duplicated
//                   face counts twice).
//   loose triangle  a valid face all three of whose edges have multiplicity 1.  Its edges are no rims: a free triangle is not closed by
//                   its own mirror image.
//   rim half-edge   a directed half-edge u->v (one of a->b, b->c, c->a) of a valid, non-loose face whose edge {u, v} has multiplicity 1.
//   simple vertex   exactly one rim half-edge leaves it and exactly one enters it; succ(u) is the destination of the one that leaves.
//                   Every other vertex has no succ (a vertex where two holes touch, a non-manifold fan, a vertex off the rims).
//   loop            vertices s_0 .. s_{L-1}, all simple, s_{j+1} = succ(s_j), succ(s_{L-1}) = s_0, s_0 the smallest index among them (the
//                   leader).  A chain that meets a vertex without succ is no loop.  L >= 3 follows from the multiplicity rule (a loop of
//                   two would be an edge of two faces).  A loop is filled when L <= max_edges.
//   output          loops in ascending leader.  Vertices: V, then one vertex per filled loop with L > 3 in that order.  Faces: F, then the
//                   new faces loop by loop.  L == 3: the one face (s_0, s_2, s_1).  L > 3: the L faces (s_{j+1}, s_j, c), j = 0..L-1, with
//                   s_L = s_0 and c the index of the loop's new vertex.  The new vertex, per component in fp64, every operation rounded on
//                   its own (-ffp-contract=off): acc = 0.0; acc = acc + double(V[s_j]) for j = 0..L-1 in that order; f32(acc / double(L)).
//                   A new face carries every rim edge in the opposite direction, so the winding stays consistent.
// The result is a pure function of (V, F, max_edges): it does not depend on the order of the faces, there are no float atomics (no atomics
// at all), and the summation order is the order of the loop from its leader.
//
// Between the kernels the caller (topology.rim_rows, fill.fill_holes) sorts the keys and drops the sentinels, counts the half-edges that
// leave and enter every vertex, writes succ (-1 for a vertex that is not simple), lists the vertices with a succ in ascending order as
// candidates, and after loops_kernel takes two exclusive running sums over the loops found: the slot of the new vertex and the first new face.
//
// Shape: rim_keys_kernel one thread per face, three binary searches in the ascending adjacency rows, three 8-byte stores.  loops_kernel
// one thread per candidate: it walks succ and gives up at the first vertex below its own, so on a typical labelling the work stays near the
// size of the rims; the worst case (a long rim whose indices ascend along it) is candidates x max_edges steps.  emit_kernel one lane per
// loop, because the fp64 sum is sequential by rule: one walk that checks the loop and sums, one that writes.  Plain vector loads and stores,
// no LDS.  These are latency-bound gathers.  Every index read from a table is range-checked before it becomes an address.
#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

constexpr int FILL_MAX_EDGES = 4096;

// the multiplicity of the edge u->v in the adjacency rows, 0 when the row is out of range or does not hold v
__device__ __forceinline__ int edge_mult(int64_t u, int64_t v, const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr,
                                         const int32_t* __restrict__ mult, int64_t ne) {
    int64_t lo = offsets[u], hi = offsets[u + 1];
    if (lo < 0 || lo > hi || hi > ne) return 0;             // a row outside [0, ne] is skipped, never read
    const int64_t end = hi;
    while (lo < hi) {                                       // the first entry >= v
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)nbr[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < end && (int64_t)nbr[lo] == v) ? mult[lo] : 0;
}

__global__ __launch_bounds__(256) void rim_keys_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv,
                                                       const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr,
                                                       const int32_t* __restrict__ mult, int64_t ne, int64_t* __restrict__ keys) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int64_t k0 = KEY_SENTINEL, k1 = KEY_SENTINEL, k2 = KEY_SENTINEL;
    if (face_valid(a, b, c, nv)) {
        const bool r0 = edge_mult(a, b, offsets, nbr, mult, ne) == 1;
        const bool r1 = edge_mult(b, c, offsets, nbr, mult, ne) == 1;
        const bool r2 = edge_mult(c, a, offsets, nbr, mult, ne) == 1;
        if (!(r0 && r1 && r2)) {                            // all three: a loose triangle, no rims
            if (r0) k0 = (a << 32) | b;
            if (r1) k1 = (b << 32) | c;
            if (r2) k2 = (c << 32) | a;
        }
    }
    keys[3 * f] = k0;
    keys[3 * f + 1] = k1;
    keys[3 * f + 2] = k2;
}

__global__ __launch_bounds__(256) void loops_kernel(const int64_t* __restrict__ cand, int64_t nc, const int32_t* __restrict__ succ, int64_t nv,
                                                    int max_edges, int32_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const int64_t v = cand[i];
    int32_t found = 0;
    if (v >= 0 && v < nv) {
        int64_t cur = v;
        for (int step = 1; step <= max_edges; ++step) {
            const int64_t nxt = succ[cur];
            if (nxt == v) {                                 // closed after `step` edges; fewer than three is no loop of a mesh
                found = step >= 3 ? step : 0;
                break;
            }
            if (nxt < v || nxt >= nv) break;                // no succ (-1), out of range, or a smaller vertex: v does not lead
            cur = nxt;
        }
    }
    len[i] = found;
}

__global__ __launch_bounds__(64) void emit_kernel(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ succ,
                                                  const int64_t* __restrict__ leader, const int32_t* __restrict__ len,
                                                  const int64_t* __restrict__ vslot, const int64_t* __restrict__ foff, int64_t nl,
                                                  float* __restrict__ new_verts, int64_t nnew, int64_t* __restrict__ new_faces, int64_t nfnew) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= nl) return;
    const int64_t s0 = leader[i], L = len[i], fo = foff[i];
    const bool fan = L > 3;
    const int64_t slot = fan ? vslot[i] : 0;
    if (s0 < 0 || s0 >= nv || L < 3 || L > FILL_MAX_EDGES) return;
    if (fo < 0 || fo > nfnew || (fan ? L : 1) > nfnew - fo) return;          // the rows of this loop lie in new_faces
    if (fan && (slot < 0 || slot >= nnew)) return;
    // first walk: the loop closes after exactly L edges, every vertex on the way is one; the sum runs in loop order
    double acc[3] = {0.0, 0.0, 0.0};
    int64_t cur = s0;
    for (int64_t j = 0; j < L; ++j) {
        acc[0] = acc[0] + (double)verts[3 * cur];
        acc[1] = acc[1] + (double)verts[3 * cur + 1];
        acc[2] = acc[2] + (double)verts[3 * cur + 2];
        const int64_t nxt = succ[cur];
        if (nxt < 0 || nxt >= nv || ((nxt == s0) != (j == L - 1))) return;   // broken, early or late: nothing is written
        cur = nxt;
    }
    if (!fan) {
        const int64_t s1 = succ[s0], s2 = succ[s1];                          // both checked by the walk above
        int64_t* o = new_faces + 3 * fo;
        o[0] = s0;
        o[1] = s2;
        o[2] = s1;
        return;
    }
    const double d = (double)L;
    new_verts[3 * slot] = (float)(acc[0] / d);
    new_verts[3 * slot + 1] = (float)(acc[1] / d);
    new_verts[3 * slot + 2] = (float)(acc[2] / d);
    const int64_t c = nv + slot;
    cur = s0;
    for (int64_t j = 0; j < L; ++j) {                                        // second walk over the checked loop: face j = (s_{j+1}, s_j, c)
        const int64_t nxt = succ[cur];
        int64_t* o = new_faces + 3 * (fo + j);
        o[0] = nxt;
        o[1] = cur;
        o[2] = c;
        cur = nxt;
    }
}

}  // namespace

extern "C" {

int ppsx_fill_rim_keys(const int64_t* faces, int64_t nf, int64_t nv, const int64_t* offsets, const int32_t* nbr, const int32_t* mult, int64_t ne,
                       int64_t* keys, void* stream) {
    if (nf < 0 || nv < 0 || ne < 0 || nf > (int64_t)INT32_MAX || nv > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !keys || (nv > 0 && !offsets) || (ne > 0 && (!nbr || !mult))) return PPS_ERR_ARG;
    const int64_t blocks = (nf + 255) / 256;
    hipLaunchKernelGGL(rim_keys_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, offsets, nbr, mult, ne, keys);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_fill_loops(const int64_t* cand, int64_t nc, const int32_t* succ, int64_t nv, int max_edges, int32_t* len, void* stream) {
    if (nc < 0 || nv < 0 || nc > (int64_t)INT32_MAX || nv > (int64_t)INT32_MAX || max_edges < 3 || max_edges > FILL_MAX_EDGES) return PPS_ERR_ARG;
    if (nc == 0) return PPS_OK;
    if (!cand || !len || (nv > 0 && !succ)) return PPS_ERR_ARG;
    const int64_t blocks = (nc + 255) / 256;
    hipLaunchKernelGGL(loops_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cand, nc, succ, nv, max_edges, len);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_fill_emit(const float* verts, int64_t nv, const int32_t* succ, const int64_t* leader, const int32_t* len, const int64_t* vslot,
                   const int64_t* foff, int64_t nl, float* new_verts, int64_t nnew, int64_t* new_faces, int64_t nfnew, void* stream) {
    if (nv < 0 || nl < 0 || nnew < 0 || nfnew < 0 || nv > (int64_t)INT32_MAX || nl > (int64_t)INT32_MAX || nnew > (int64_t)INT32_MAX ||
        nfnew > (int64_t)INT32_MAX)
        return PPS_ERR_ARG;
    if (nl == 0) return PPS_OK;
    if (!leader || !len || !vslot || !foff || (nv > 0 && (!verts || !succ)) || (nnew > 0 && !new_verts) || (nfnew > 0 && !new_faces))
        return PPS_ERR_ARG;
    const int64_t blocks = (nl + 63) / 64;
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, verts, nv, succ, leader, len, vslot, foff, nl,
                       new_verts, nnew, new_faces, nfnew);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
