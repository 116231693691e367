// Trim by support for gfx950: which faces of a reconstructed mesh have a point of the scan within a radius.
//
// new capability: replaces nothing -- the reference closes every surface and has no trim.  Driven by ppsurf_amd/trim.py; restated in numpy by
// tests/trim_spec.py (brute force over all pairs), which the kernel matches bit for bit.
//
// Rule: face f = (i0, i1, i2) is supported iff 0 <= i0, i1, i2 < nv (face_in_range of pps_faces.h), its nine corner coordinates are finite
//   and some cloud point p has
//   d2(p, triangle) <= r * r,  d2 from closest_on_triangle<double> of pps_tri.h on the f32 inputs widened to fp64, r * r one fp64 multiply.
// Existence does not depend on the order in which the points are visited, so support is a pure function of (points, verts, faces, r).
//
// Cell lists: the grid and table of pps_cells.h in fp32 over the cloud's box, cell edge h >= r.  slots_kernel inserts every point's cell key
// and writes the slot it landed in; the caller sorts the points by slot (order, offsets).  WHICH slot a cell gets depends on timing, the
// set of points per cell does not, and support depends on neither.
//
// Candidates of a face: its box in fp64 (exact: the corners are f32), widened by R = r * (1 + 2^-20) and rounded OUTWARD to f32.  A box
// disjoint from the cloud's box [lo, hi] has no candidate.  Otherwise the cell range is cell_of(box lo) .. cell_of(box hi) per axis with the
// cell_of that placed the points: subtract, multiply and floor are monotone, so every point inside the f32 box lies in a cell of the range;
// DESIGN.md 15 argues why a point outside the box cannot pass the test.  When the range holds more cells than the cloud has points the lanes
// walk all points instead: same result, work bounded by min(cells, n).
//
// Shape: one wave per face, four faces per 256-thread workgroup.  Lane l takes the cells l, l + 64, ... of the range (x fastest), probes the
// table read-only and walks the points of its cell through `order`.  The loop is wave-uniform -- every turn a lane either opens its next
// cell or tests one point -- and ends on the first hit of any lane (__any) or when no lane has work left.  Plain vector loads, one byte
// stored per face, no LDS, no atomics.  Every index read from faces, offsets and order is range-checked before it is used as an address.
#include <math.h>

#include "pps_cells.h"
#include "pps_faces.h"
#include "pps_tri.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

using cells::u64;
typedef cells::Grid<float> Grid;

constexpr int FACES_PER_BLOCK = 4;

struct Box {
    float hi[3];                                             // of the cloud (Grid carries lo)
};

// One thread per point: find or insert the point's cell, slot[i] = where it lives.
__global__ __launch_bounds__(256) void slots_kernel(const float* __restrict__ pts, int64_t n, Grid grid, u64* __restrict__ table, u64 mask,
                                                    int64_t* __restrict__ slot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int cx = cells::cell_of(pts[3 * i], grid.lo[0], grid.inv_h, grid.g[0]);
    const int cy = cells::cell_of(pts[3 * i + 1], grid.lo[1], grid.inv_h, grid.g[1]);
    const int cz = cells::cell_of(pts[3 * i + 2], grid.lo[2], grid.inv_h, grid.g[2]);
    bool fresh = false;
    slot[i] = (int64_t)cells::find_or_insert(table, mask, cells::key_of(grid, cx, cy, cz), fresh);
}

__device__ __forceinline__ bool within(const float* __restrict__ pts, int64_t i, V3<double> a, V3<double> b, V3<double> c, double r2) {
    const V3<double> p = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
    double s, t, d2;
    closest_on_triangle<double>(p, a, b, c, s, t, d2);
    return d2 <= r2;
}

__global__ __launch_bounds__(64 * FACES_PER_BLOCK) void face_support_kernel(const float* __restrict__ verts, int64_t nv,
                                                                            const int64_t* __restrict__ faces, int64_t nf,
                                                                            const float* __restrict__ pts, int64_t n, Grid grid, Box box,
                                                                            const u64* __restrict__ table, u64 mask,
                                                                            const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                                            double r, uint8_t* __restrict__ support) {
    const int64_t f = (int64_t)blockIdx.x * FACES_PER_BLOCK + (threadIdx.x >> 6);          // wave-uniform
    if (f >= nf) return;
    const int lane = threadIdx.x & 63;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    bool live = face_in_range(i0, i1, i2, nv);                                             // a bad index is never read through
    V3<double> a = {0.0, 0.0, 0.0}, b = a, c = a;
    int c0[3] = {0, 0, 0}, cn[3] = {0, 0, 0};
    if (live) {
        a = {(double)verts[3 * i0], (double)verts[3 * i0 + 1], (double)verts[3 * i0 + 2]};
        b = {(double)verts[3 * i1], (double)verts[3 * i1 + 1], (double)verts[3 * i1 + 2]};
        c = {(double)verts[3 * i2], (double)verts[3 * i2 + 1], (double)verts[3 * i2 + 2]};
        const double R = r * (1.0 + 0x1p-20);
        const double ca[3][3] = {{a.x, b.x, c.x}, {a.y, b.y, c.y}, {a.z, b.z, c.z}};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double mn = fmin(ca[k][0], fmin(ca[k][1], ca[k][2])), mx = fmax(ca[k][0], fmax(ca[k][1], ca[k][2]));
            live = live && isfinite(ca[k][0]) && isfinite(ca[k][1]) && isfinite(ca[k][2]);
            const float blo = __double2float_rd(mn - R), bhi = __double2float_ru(mx + R);
            live = live && blo <= box.hi[k] && bhi >= grid.lo[k];                           // disjoint from the cloud's box: no candidate
            c0[k] = cells::cell_of(blo, grid.lo[k], grid.inv_h, grid.g[k]);
            cn[k] = cells::cell_of(bhi, grid.lo[k], grid.inv_h, grid.g[k]) - c0[k] + 1;
        }
    }
    if (!live) {                                                                            // wave-uniform: f is
        if (lane == 0) support[f] = 0;
        return;
    }
    const double r2 = r * r;
    const int64_t ncells = (int64_t)cn[0] * cn[1] * cn[2];                                  // each factor <= 2^20
    bool hit = false;
    if (ncells > n) {                                                                       // more cells than points: all points
        for (int64_t i = lane; __any(i < n); i += 64) {
            if (i < n) hit = within(pts, i, a, b, c, r2);
            if (__any(hit)) break;
        }
    } else {
        int64_t cell = lane, j = 0, jend = 0;
        while (true) {
            if (j < jend) {                                                                 // one point of the open cell
                const int64_t i = order[j++];
                if (i >= 0 && i < n) hit = within(pts, i, a, b, c, r2);
            } else if (cell < ncells) {                                                     // open the next cell: a read-only probe
                const int cx = c0[0] + (int)(cell % cn[0]), cy = c0[1] + (int)((cell / cn[0]) % cn[1]);
                const int cz = c0[2] + (int)(cell / ((int64_t)cn[0] * cn[1]));
                cells::find_run(table, mask, cells::key_of(grid, cx, cy, cz), offsets, n, j, jend);
                cell += 64;
            }
            if (__any(hit) || !__any(j < jend || cell < ncells)) break;
        }
    }
    hit = __any(hit);
    if (lane == 0) support[f] = hit ? 1 : 0;
}

}  // namespace

extern "C" {

int ppsx_trim_cell_slots(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, uint64_t* table, int64_t capacity,
                         int64_t* slot, void* stream) {
    Grid grid;
    if (!pts || !table || !slot || !cells::table_ok(n, capacity) || !cells::make_grid(lo, hi, h, inv_h, &grid)) return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0xFF, (size_t)capacity * 8, st) != hipSuccess) return PPS_ERR_LAUNCH;
    hipLaunchKernelGGL(slots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, grid, (u64*)table, (u64)(capacity - 1), slot);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_trim_face_support(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* pts, int64_t n, const float* lo,
                           const float* hi, float h, float inv_h, const uint64_t* table, int64_t capacity, const int64_t* order,
                           const int64_t* offsets, double r, uint8_t* support, void* stream) {
    if (nf < 0 || nv < 0 || n < 0 || !(r > 0.0) || !(r <= 1.0e300) || !((double)h >= r)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (!support) return PPS_ERR_ARG;
        return hipMemsetAsync(support, 0, (size_t)nf, st) == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
    }
    Grid grid;
    if (!verts || !faces || !pts || !table || !order || !offsets || !support || !cells::table_ok(n, capacity) ||
        !cells::make_grid(lo, hi, h, inv_h, &grid))
        return PPS_ERR_ARG;
    const int64_t blocks = (nf + FACES_PER_BLOCK - 1) / FACES_PER_BLOCK;
    if (blocks > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    const Box box = {{hi[0], hi[1], hi[2]}};
    hipLaunchKernelGGL(face_support_kernel, dim3((unsigned)blocks), dim3(64 * FACES_PER_BLOCK), 0, st, verts, nv, faces, nf, pts, n, grid, box,
                       (const u64*)table, (u64)(capacity - 1), order, offsets, r, support);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
