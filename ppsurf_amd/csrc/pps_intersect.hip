// Self-intersections for gfx950: which pairs of faces of a mesh cross.
//
// new capability: replaces nothing -- the reference has no such check.  Driven by ppsurf_amd/intersect.py; restated in numpy by
// tests/intersect_spec.py (brute force over all pairs, no grid), which the kernels match bit for bit.
//
// Rule.  A face is LIVE when it is valid (face_valid of pps_faces.h) and its nine coordinates are finite; every other face is never flagged
// and never read through.  A live face has the closed box lo..hi of its three f32 corners.  A pair f != g is BOXED when both are live, the
// boxes overlap on all three axes (lo_f <= hi_g && lo_g <= hi_f, f32 compares) and the faces share at most one vertex INDEX.  A boxed pair
// CROSSES when one of its admitted edge-against-triangle tests is positive: all six with no shared index, with one shared index only the two
// edges opposite the shared vertex, each against the other triangle (the edge opposite corner k is (k + 1, k + 2) mod 3).  The test of the
// edge (p, q) against (a, b, c) as stored, widened to fp64, every operation rounded on its own (-ffp-contract=off), sub / dot / cross of
// pps_tri.h:
//   n = (b - a) x (c - a); sp = dot(n, p - a), sq = dot(n, q - a) strictly opposite in sign, both non-zero;
//   d = q - p; t0 = dot(d x (a - p), b - p), t1 = dot(d x (b - p), c - p), t2 = dot(d x (c - p), a - p) all >= 0 or all <= 0, not all zero.
// Seen from f or from g the same six tests are made with the same operands, so the verdict is symmetric and the flags do not depend on the
// order of the faces.  Coplanar overlaps, a vertex exactly in the other plane and zero-area faces are contacts, not crossings.
//
// Broad phase.  The caller puts the box lower corners (the anchors) of the SMALL live faces -- ext <= h, ext the largest fp64 extent of the
// box rounded up to f32 -- into the cell lists of pps_cells.h with cell edge h (ppsx_trim_cell_slots, a sort, row offsets) and lists the
// other live faces, the LARGE ones, of any extent (the host splits at an extent L <= h).  A wave owns one face f, small or large, and opens the cells of [rd32(lo_f - H), hi_f] per axis with
// H = h (1 + 2^-20) and the cell_of that placed the anchors: a small g whose box overlaps f's has lo_g <= hi_f and
// lo_g >= hi_g - (hi_g - lo_g) >= lo_f - h (1 + 2^-52) > lo_f - H in real numbers (section 29 spells the roundings out), subtract, multiply
// and floor are monotone, so its anchor lies in a cell of the range.  When the range holds more cells than there are anchors the lanes walk all
// anchors instead.  Every wave then walks the list of large faces, strided over its lanes.  Each partner g != f is met exactly once: an
// anchor lives in one cell, and the two lists are disjoint.
//
// Shape: one wave per face, four faces per 256-thread workgroup; lane l takes the cells l, l + 64, ... of the range.  The loop is
// wave-uniform -- every turn a lane opens its next cell or tests one candidate -- and the counts are ballots, so no atomics, no LDS.  The emit
// kernel makes the same walk and writes the pair (f, g), g > f, at offsets[f] + its ballot-prefix position, only while that position stays
// below count[f].  Every index read from faces, order, offsets, small and large is range-checked before it is used as an address.
#include <math.h>

#include "pps_cells.h"
#include "pps_faces.h"
#include "pps_tri.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

using cells::u64;
typedef cells::Grid<float> Grid;
typedef V3<double> P3;

constexpr int FACES_PER_BLOCK = 4;

struct Box {
    float hi[3];                                             // of the anchors (Grid carries lo)
};

struct Tri {
    P3 a, b, c;
};

__device__ __forceinline__ P3 point_of(const float* __restrict__ verts, int64_t i) {
    return {(double)verts[3 * i], (double)verts[3 * i + 1], (double)verts[3 * i + 2]};
}

// One thread per face: box, extent and the live flag; the rows of a face that is not live are zero.
__global__ __launch_bounds__(256) void boxes_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                    float* __restrict__ lo, float* __restrict__ hi, float* __restrict__ ext,
                                                    uint8_t* __restrict__ live) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    bool ok = face_valid(i0, i1, i2, nv);                                                  // a bad index is never read through
    float l[3] = {0.0f, 0.0f, 0.0f}, h[3] = {0.0f, 0.0f, 0.0f};
    double e = 0.0;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = verts[3 * i0 + k], y = verts[3 * i1 + k], z = verts[3 * i2 + k];
            ok = ok && isfinite(x) && isfinite(y) && isfinite(z);
            l[k] = fminf(x, fminf(y, z));
            h[k] = fmaxf(x, fmaxf(y, z));
            e = fmax(e, (double)h[k] - (double)l[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[3 * f + k] = ok ? l[k] : 0.0f;
        hi[3 * f + k] = ok ? h[k] : 0.0f;
    }
    ext[f] = ok ? __double2float_ru(e) : 0.0f;
    live[f] = ok ? 1 : 0;
}

// the edge (p, q) against the triangle t with the normal n of t and sp = dot(n, p - t.a), sq = dot(n, q - t.a)
__device__ __forceinline__ bool edge_hits(P3 p, P3 q, double sp, double sq, const Tri& t) {
    if (!((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0))) return false;
    const P3 d = sub(q, p), ap = sub(t.a, p), bp = sub(t.b, p), cp = sub(t.c, p);
    const double t0 = dot(cross(d, ap), bp), t1 = dot(cross(d, bp), cp), t2 = dot(cross(d, cp), ap);
    const bool inside = (t0 >= 0.0 && t1 >= 0.0 && t2 >= 0.0) || (t0 <= 0.0 && t1 <= 0.0 && t2 <= 0.0);
    return inside && !(t0 == 0.0 && t1 == 0.0 && t2 == 0.0);
}

// the edges of e admitted by `only` (-1: all three, k: the one opposite corner k) against the triangle t
__device__ __forceinline__ bool edges_hit(const Tri& e, const Tri& t, int only) {
    const P3 n = cross(sub(t.b, t.a), sub(t.c, t.a));
    const double s0 = dot(n, sub(e.a, t.a)), s1 = dot(n, sub(e.b, t.a)), s2 = dot(n, sub(e.c, t.a));
    bool hit = false;
    if (only < 0 || only == 0) hit = hit || edge_hits(e.b, e.c, s1, s2, t);
    if (only < 0 || only == 1) hit = hit || edge_hits(e.c, e.a, s2, s0, t);
    if (only < 0 || only == 2) hit = hit || edge_hits(e.a, e.b, s0, s1, t);
    return hit;
}

struct Face {
    int64_t i[3];
    float lo[3], hi[3];
    Tri t;
};

// The narrow phase of f against the candidate g: boxed and crosses.
__device__ __forceinline__ void test_pair(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                          const float* __restrict__ lo, const float* __restrict__ hi, const uint8_t* __restrict__ live,
                                          int64_t f, const Face& F, int64_t g, bool& boxed, bool& crosses) {
    boxed = crosses = false;
    if (g < 0 || g >= nf || g == f || live[g] == 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (!(F.lo[k] <= hi[3 * g + k] && lo[3 * g + k] <= F.hi[k])) return;
    const int64_t j0 = faces[3 * g], j1 = faces[3 * g + 1], j2 = faces[3 * g + 2];
    if (!face_valid(j0, j1, j2, nv)) return;                                                // live says so; never read through a bad index
    const int64_t j[3] = {j0, j1, j2};
    int shared = 0, kf = -1, kg = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (F.i[a] == j[b]) { ++shared; kf = a; kg = b; }
    if (shared > 1) return;
    boxed = true;
    const Tri G = {point_of(verts, j0), point_of(verts, j1), point_of(verts, j2)};
    crosses = edges_hit(F.t, G, kf) || edges_hit(G, F.t, kg);
}

template <bool EMIT>
__global__ __launch_bounds__(64 * FACES_PER_BLOCK) void walk_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces,
                                                                    int64_t nf, const float* __restrict__ lo, const float* __restrict__ hi,
                                                                    const uint8_t* __restrict__ live, const int64_t* __restrict__ small, int64_t ns,
                                                                    Grid grid, Box box, const u64* __restrict__ table, u64 mask,
                                                                    const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                                    const int64_t* __restrict__ large, int64_t nl, uint8_t* __restrict__ flag,
                                                                    int32_t* __restrict__ count, int32_t* __restrict__ nboxed,
                                                                    const int32_t* __restrict__ caps, const int64_t* __restrict__ pair_offsets,
                                                                    int64_t np, int64_t* __restrict__ pairs) {
    const int64_t f = (int64_t)blockIdx.x * FACES_PER_BLOCK + (threadIdx.x >> 6);          // wave-uniform
    if (f >= nf) return;
    const int lane = threadIdx.x & 63;
    Face F;
    F.i[0] = faces[3 * f]; F.i[1] = faces[3 * f + 1]; F.i[2] = faces[3 * f + 2];
    if (live[f] == 0 || !face_valid(F.i[0], F.i[1], F.i[2], nv)) {                          // wave-uniform: f is
        if (!EMIT && lane == 0) { flag[f] = 0; count[f] = 0; nboxed[f] = 0; }
        return;
    }
    F.t = {point_of(verts, F.i[0]), point_of(verts, F.i[1]), point_of(verts, F.i[2])};
    int c0[3] = {0, 0, 0}, cn[3] = {0, 0, 0};
    bool cells_open = ns > 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.lo[k] = lo[3 * f + k];
        F.hi[k] = hi[3 * f + k];
        if (ns > 0) {
            const float blo = __double2float_rd((double)F.lo[k] - (double)grid.h * (1.0 + 0x1p-20));
            cells_open = cells_open && blo <= box.hi[k] && F.hi[k] >= grid.lo[k];           // disjoint from the anchors' box: no small candidate
            c0[k] = cells::cell_of(blo, grid.lo[k], grid.inv_h, grid.g[k]);
            cn[k] = cells::cell_of(F.hi[k], grid.lo[k], grid.inv_h, grid.g[k]) - c0[k] + 1;
        }
    }
    int64_t cap = 0, at = 0;                                                                // emit: count[f] and where its pairs start
    if (EMIT) {
        cap = caps[f];
        at = pair_offsets[f];
        if (cap <= 0 || at < 0 || at > np - cap) return;                                    // wave-uniform; nothing of f fits
    }
    const u64 below = (1ull << lane) - 1ull;
    int64_t n_cross = 0, n_boxed = 0;                                                       // wave-uniform sums of ballots
    bool any = false;

    auto tally = [&](int64_t g, bool boxed, bool crosses) {                                 // every lane of the wave calls it
        const bool up = g > f;
        const u64 b_cross = __ballot(crosses && up);
        if (EMIT) {
            const int64_t pos = n_cross + __popcll(b_cross & below);
            if (crosses && up && pos < cap) {
                pairs[2 * (at + pos)] = f;
                pairs[2 * (at + pos) + 1] = g;
            }
        } else {
            n_boxed += __popcll(__ballot(boxed && up));
            any = any || crosses;
        }
        n_cross += __popcll(b_cross);
    };

    if (cells_open) {
        const int64_t ncells = (int64_t)cn[0] * cn[1] * cn[2];                              // each factor <= 2^20
        if (ncells > ns) {                                                                  // more cells than anchors: all anchors
            for (int64_t base = 0; base < ns; base += 64) {
                const int64_t i = base + lane;
                bool boxed = false, crosses = false;
                const int64_t g = i < ns ? small[i] : -1;
                if (i < ns) test_pair(verts, nv, faces, nf, lo, hi, live, f, F, g, boxed, crosses);
                tally(g, boxed, crosses);
            }
        } else {
            int64_t cell = lane, j = 0, jend = 0;
            while (true) {
                bool boxed = false, crosses = false;
                int64_t g = -1;
                if (j < jend) {                                                             // one anchor of the open cell
                    const int64_t i = order[j++];
                    if (i >= 0 && i < ns) {
                        g = small[i];
                        test_pair(verts, nv, faces, nf, lo, hi, live, f, F, g, boxed, crosses);
                    }
                } else if (cell < ncells) {                                                 // open the next cell: a read-only probe
                    const int cx = c0[0] + (int)(cell % cn[0]), cy = c0[1] + (int)((cell / cn[0]) % cn[1]);
                    const int cz = c0[2] + (int)(cell / ((int64_t)cn[0] * cn[1]));
                    cells::find_run(table, mask, cells::key_of(grid, cx, cy, cz), offsets, ns, j, jend);
                    cell += 64;
                }
                tally(g, boxed, crosses);
                if (!__any(j < jend || cell < ncells)) break;
            }
        }
    }
    for (int64_t base = 0; base < nl; base += 64) {                                         // the large faces: every wave walks them all
        const int64_t i = base + lane;
        bool boxed = false, crosses = false;
        const int64_t g = i < nl ? large[i] : -1;
        if (i < nl) test_pair(verts, nv, faces, nf, lo, hi, live, f, F, g, boxed, crosses);
        tally(g, boxed, crosses);
    }
    if (!EMIT) {
        any = __any(any);
        if (lane == 0) {
            flag[f] = any ? 1 : 0;
            count[f] = (int32_t)n_cross;
            nboxed[f] = (int32_t)n_boxed;
        }
    }
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }

// the shared argument rule of the two walks: PPS_OK = launch, -1 = no face and nothing to do, else the status to return
inline int walk_args(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* lo, const float* hi, const uint8_t* live,
                     const int64_t* small, int64_t ns, const float* glo, const float* ghi, float h, float inv_h, const uint64_t* table,
                     int64_t capacity, const int64_t* order, const int64_t* offsets, const int64_t* large, int64_t nl, Grid* grid, Box* box) {
    if (nf < 0 || nv < 0 || ns < 0 || nl < 0 || too_many(nf) || too_many(nv) || ns > nf || nl > nf - ns || !(h >= 0.0f)) return PPS_ERR_ARG;
    if (nf == 0) return -1;
    if (!faces || !lo || !hi || !live || (nv > 0 && !verts) || (nl > 0 && !large)) return PPS_ERR_ARG;
    *grid = Grid();
    *box = Box();
    if (ns > 0) {
        if (!small || !table || !order || !offsets || !cells::table_ok(ns, capacity) || !cells::make_grid(glo, ghi, h, inv_h, grid)) return PPS_ERR_ARG;
        for (int k = 0; k < 3; ++k) box->hi[k] = ghi[k];
    }
    if ((nf + FACES_PER_BLOCK - 1) / FACES_PER_BLOCK > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    return PPS_OK;
}

}  // namespace

extern "C" {

int ppsx_intersect_boxes(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, float* lo, float* hi, float* ext, uint8_t* live,
                         void* stream) {
    if (nf < 0 || nv < 0 || too_many(nf) || too_many(nv)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !lo || !hi || !ext || !live || (nv > 0 && !verts)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, faces, nf, lo, hi, ext, live);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_intersect_count(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* lo, const float* hi, const uint8_t* live,
                         const int64_t* small, int64_t ns, const float* glo, const float* ghi, float h, float inv_h, const uint64_t* table,
                         int64_t capacity, const int64_t* order, const int64_t* offsets, const int64_t* large, int64_t nl, uint8_t* flag,
                         int32_t* count, int32_t* boxed, void* stream) {
    Grid grid;
    Box box;
    const int rc = walk_args(verts, nv, faces, nf, lo, hi, live, small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl, &grid, &box);
    if (rc != PPS_OK) return rc < 0 ? PPS_OK : rc;
    if (!flag || !count || !boxed) return PPS_ERR_ARG;
    hipLaunchKernelGGL(walk_kernel<false>, dim3((unsigned)((nf + FACES_PER_BLOCK - 1) / FACES_PER_BLOCK)), dim3(64 * FACES_PER_BLOCK), 0,
                       (hipStream_t)stream, verts, nv, faces, nf, lo, hi, live, small, ns, grid, box, (const u64*)table, (u64)(capacity - 1), order,
                       offsets, large, nl, flag, count, boxed, (const int32_t*)nullptr, (const int64_t*)nullptr, (int64_t)0, (int64_t*)nullptr);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_intersect_emit(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* lo, const float* hi, const uint8_t* live,
                        const int64_t* small, int64_t ns, const float* glo, const float* ghi, float h, float inv_h, const uint64_t* table,
                        int64_t capacity, const int64_t* order, const int64_t* offsets, const int64_t* large, int64_t nl, const int32_t* count,
                        const int64_t* pair_offsets, int64_t np, int64_t* pairs, void* stream) {
    Grid grid;
    Box box;
    if (np < 0) return PPS_ERR_ARG;
    const int rc = walk_args(verts, nv, faces, nf, lo, hi, live, small, ns, glo, ghi, h, inv_h, table, capacity, order, offsets, large, nl, &grid, &box);
    if (rc != PPS_OK) return rc < 0 ? PPS_OK : rc;
    if (!count || !pair_offsets || (np > 0 && !pairs)) return PPS_ERR_ARG;
    if (np == 0) return PPS_OK;
    hipLaunchKernelGGL(walk_kernel<true>, dim3((unsigned)((nf + FACES_PER_BLOCK - 1) / FACES_PER_BLOCK)), dim3(64 * FACES_PER_BLOCK), 0,
                       (hipStream_t)stream, verts, nv, faces, nf, lo, hi, live, small, ns, grid, box, (const u64*)table, (u64)(capacity - 1), order,
                       offsets, large, nl, (uint8_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, count, pair_offsets, np, pairs);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
