// Weld for gfx950: the vertices of a mesh that coincide, or lie within a tolerance, become one row, and the faces this collapses leave
// (DESIGN.md section 24).
//
// new capability: replaces nothing -- the reference has no such stage, and pps_mesh_corner_weld stays what it is, the weld of Marching Cubes
// in its own grid index space.  Driven by ppsurf_amd/weld.py (the cell lists by trim.SupportGrid); restated in numpy by tests/weld_spec.py
// (brute force over all pairs, a union by smallest row), which the kernels match byte for byte.
//
// The rule: vertices V f32 [nv,3] (finite), faces F int64 [nf,3], eps >= 0 (fp64), nv, nf <= 2^31 - 1.
//   link       rows i != j are linked when ((dx dx + dy dy) + dz dz) <= eps2, d* = double(V_i*) - double(V_j*), eps2 = eps * eps (one fp64
//              multiply on the host), every operation rounded on its own (-ffp-contract=off).  Symmetric in i, j.  With eps = 0 it is
//              equality of the three coordinates, -0.0 equal to +0.0.
//   cluster    a connected component of the link graph (single linkage: a row of points each within eps of the next is ONE cluster); its
//              leader is its smallest row; label[v] = the leader of v's cluster (int32).
//   vertices   the leaders in ascending row; newrow[v] = the output row of v's leader (host: a cumsum and a gather).
//   faces      code 1: invalid as given (face_valid of pps_faces.h) or a newrow entry outside [0, nv); code 2: valid as given, two corners in
//              one cluster; code 0: kept, its corners renumbered, its winding as given.
// A pure function of (V, F, eps): no dependence on the cell grid, the table capacity, the launch shape or on timing.
//
// Labelling (hook_kernel here, the compress of pps_labels.hip; the argument is written out in pps_labels.h).  A node is a vertex, a link
// a pair of rows within eps, found on the fly: label[v] starts as v.
//   hook      vertex i visits every j < i it is linked to and joins their ends (join_ends of pps_labels.h): the flag goes up only when a
//             label fell, so a launch raises it exactly when it changed a label.  No pair list is kept: k copies of one point are
//             k k / 2 pairs.
//   skipped   a vertex with a negative label, as i and as j; an order entry outside [0, i).
//
// Candidates of vertex i (the point query of section 15's argument): per axis the interval p_i -+ R, R = eps (1 + 2^-20), computed in fp64
// and rounded OUTWARD to f32; the cell range is cell_of(lower) .. cell_of(upper) with the cell_of that placed the points, which is monotone,
// so every point inside the f32 interval on all three axes lies in a cell of the range.  A linked j lies inside: from d2 <= eps2 follows
// |d_a| <= eps (1 + 2^-50) per axis (the roundings of the difference, the squares, the sums and of eps2), and the rounding of p_i -+ R is at
// most 2^-53 (|p_i| + R), which the slack 2^-20 eps covers while eps >= 2^-32 |p_i|; below that eps is under half the spacing of the f32
// near p_i, so a linked j has d_a = 0 exactly, and p_i itself is never outside its own interval (fp64 subtraction of R >= 0 and the
// outward rounding are monotone).  When the range holds more cells than there are vertices, i walks the rows below it instead: same links.
// The cell edge only sets the work: no result depends on it.
//
// Shape: hook_kernel one thread per vertex, a serial walk over its cells (at most 27 to 64 with a cell edge >= eps) and their runs of
// `order`; faces_kernel one thread per face.  Plain vector loads and stores, integer atomics only, no LDS.  Every index read
// from order, offsets, label, faces or newrow is range-checked before it becomes an address.
#include <math.h>

#include "pps_cells.h"
#include "pps_faces.h"
#include "pps_labels.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

using cells::u64;
typedef cells::Grid<float> Grid;

struct Query {
    double x, y, z, eps2;
    int i;
};

// j < i (0 <= j, by the caller): when the two are linked, their ends are joined
__device__ __forceinline__ void visit(const float* __restrict__ pts, const Query& q, int j, int32_t* label, int32_t* changed) {
    const double dx = q.x - (double)pts[3 * (int64_t)j], dy = q.y - (double)pts[3 * (int64_t)j + 1], dz = q.z - (double)pts[3 * (int64_t)j + 2];
    if (!(((dx * dx + dy * dy) + dz * dz) <= q.eps2)) return;
    if (load_label(label, j) < 0) return;                                                   // a vertex that takes no part
    join_ends(label, q.i, j, changed);
}

__global__ __launch_bounds__(256) void hook_kernel(const float* __restrict__ pts, int64_t n, Grid grid, const u64* __restrict__ table, u64 mask,
                                                   const int64_t* __restrict__ order, const int64_t* __restrict__ offsets, double eps,
                                                   double eps2, int32_t* label, int32_t* changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || load_label(label, i) < 0) return;
    const Query q = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], eps2, (int)i};
    const double R = eps * (1.0 + 0x1p-20), p[3] = {q.x, q.y, q.z};
    int c0[3], c1[3];
    int64_t ncells = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = cells::cell_of(__double2float_rd(p[k] - R), grid.lo[k], grid.inv_h, grid.g[k]);
        c1[k] = cells::cell_of(__double2float_ru(p[k] + R), grid.lo[k], grid.inv_h, grid.g[k]);
        ncells *= (int64_t)(c1[k] - c0[k] + 1);                                             // each factor in 1 .. 2^20
    }
    if (ncells > n) {                                                                       // more cells than vertices: the rows below i
        for (int j = 0; j < (int)i; ++j) visit(pts, q, j, label, changed);
        return;
    }
    for (int cz = c0[2]; cz <= c1[2]; ++cz)
        for (int cy = c0[1]; cy <= c1[1]; ++cy)
            for (int cx = c0[0]; cx <= c1[0]; ++cx) {
                int64_t t = 0, tend = 0;
                cells::find_run(table, mask, cells::key_of(grid, cx, cy, cz), offsets, n, t, tend);
                for (; t < tend; ++t) {
                    const int64_t j = order[t];
                    if (j >= 0 && j < i) visit(pts, q, (int)j, label, changed);
                }
            }
}

__global__ __launch_bounds__(256) void faces_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, const int64_t* __restrict__ newrow,
                                                    int64_t* __restrict__ out, uint8_t* __restrict__ code) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    uint8_t what = 1;
    if (face_valid(a, b, c, nv)) {
        const int64_t na = newrow[a], nb = newrow[b], nc = newrow[c];
        if (face_in_range(na, nb, nc, nv)) {
            what = (na == nb || nb == nc || nc == na) ? 2 : 0;
            if (what == 0) { a = na; b = nb; c = nc; }
        }
    }
    out[3 * f] = a;
    out[3 * f + 1] = b;
    out[3 * f + 2] = c;
    code[f] = what;
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }

}  // namespace

extern "C" {

int ppsx_weld_hook(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, const uint64_t* table, int64_t capacity,
                   const int64_t* order, const int64_t* offsets, double eps, int32_t* label, int32_t* changed, void* stream) {
    if (n < 0 || too_many(n) || !(eps >= 0.0)) return PPS_ERR_ARG;                          // false for a NaN
    if (n == 0) return PPS_OK;
    Grid grid;
    if (!pts || !table || !order || !offsets || !label || !changed || !cells::table_ok(n, capacity) || !cells::make_grid(lo, hi, h, inv_h, &grid))
        return PPS_ERR_ARG;
    const double eps2 = eps * eps;
    hipLaunchKernelGGL(hook_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, n, grid, (const u64*)table,
                       (u64)(capacity - 1), order, offsets, eps, eps2, label, changed);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_weld_faces(const int64_t* faces, int64_t nf, int64_t nv, const int64_t* newrow, int64_t* out, uint8_t* code, void* stream) {
    if (nf < 0 || nv < 0 || too_many(nf) || too_many(nv)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !out || !code || out == faces || (nv > 0 && !newrow)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(faces_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, newrow, out, code);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
