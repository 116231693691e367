// Mesh simplification for gfx950: Lindstrom's quadric vertex clustering (SIGGRAPH 2000), DESIGN.md section 13.
//
// new capability: the reference writes its Marching Cubes mesh at the grid's own density and has no decimation.  Driven by
// ppsurf_amd/simplify.py; restated in numpy by tests/simplify_spec.py, which the kernels match bit for bit.  Everything is fp64, each operation
// rounded on its own (-ffp-contract=off), integer atomics only.
//
// The cell grid and table of pps_cells.h in fp64, one thread per vertex.
//   leader  of a cell: its lowest vertex index, one 64-bit atomicMin per vertex; a second kernel writes leader[v] for every vertex
//   count   faces whose three leaders differ pairwise, added once per wave
// Cluster ids (the rank of a cell's leader among all leaders) and the two CSRs (corner entries e = 3 f + k by cluster, vertices by cluster,
// both ascending inside a cluster: pps_csr_build) are made by the caller.
//
// Placement, one thread per cell, sequential in this order:
//   centre_a = lo_a + (double(c_a) + 0.5) * h            (c from the cell's first vertex)
//   xhat_a   = (sum over the cell's vertices v, ascending, of (p_v,a - centre_a)) / double(number of vertices)
//   for every corner entry (f, k) of the cell, ascending, unless a corner j < k of f lies in the same cell:
//       q_i = p_i - centre (i = 0, 1, 2 the corners of f), u = q_1 - q_0, w = q_2 - q_0
//       n = (u_y w_z - u_z w_y,  u_z w_x - u_x w_z,  u_x w_y - u_y w_x)               un-normalised: Lindstrom's area^2 weight
//       m = (n_x q_0x + n_y q_0y) + n_z q_0z                                           (= -d of the plane n.x + d = 0)
//       A00 += n_x n_x, A01 += n_x n_y, A02 += n_x n_z, A11 += n_y n_y, A12 += n_y n_z, A22 += n_z n_z;   b_a += m * n_a
//   lambda = 1e-3 * ((A00 + A11) + A22);  M = A + lambda I;  r_a = b_a + lambda * xhat_a
//   cofactors  c00 = M11 M22 - M12 M12,  c01 = M02 M12 - M01 M22,  c02 = M01 M12 - M02 M11,
//              c11 = M00 M22 - M02 M02,  c12 = M01 M02 - M00 M12,  c22 = M00 M11 - M01 M01
//   det = (M00 c00 + M01 c01) + M02 c02
//   x_0 = ((c00 r_0 + c01 r_1) + c02 r_2) / det,  x_1 = ((c01 r_0 + c11 r_1) + c12 r_2) / det,  x_2 = ((c02 r_0 + c12 r_1) + c22 r_2) / det
//   x = xhat (a fallback, counted) when the trace is 0, a component of x is not finite, or |x_a| > wall for some axis (the optimum left the
//   cell: Lindstrom's rule), wall = half + half * 2^-30 with half = h * 0.5.  The 2^-30 is the thickness of a wall in fp64: a coordinate relative
//   to a cell centre carries a few roundings of 2^-52 of its magnitude, up to 2^20 cell edges, so a surface that lies ON a wall (an axis-aligned
//   face through lo or hi) is on it only to that precision.  placement 'mean' takes xhat always and counts nothing.
//   position_a = centre_a + x_a
#include "pps_cells.h"
#include "../../include/ppsurf_amd.h"

namespace {

using cells::cell_of;
using cells::u64;
typedef cells::Grid<double> GridD;

// One thread per vertex: find or insert the vertex's cell, compete for its leader, remember the slot in leader[v].
__global__ __launch_bounds__(256) void simp_insert_kernel(const double* __restrict__ verts, int64_t nv, GridD grid, u64* __restrict__ table,
                                                          u64* __restrict__ best, u64 mask, int64_t* __restrict__ leader, u64* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool fresh = false;
    if (i < nv) {
        const int cx = cell_of(verts[3 * i], grid.lo[0], grid.inv_h, grid.g[0]);
        const int cy = cell_of(verts[3 * i + 1], grid.lo[1], grid.inv_h, grid.g[1]);
        const int cz = cell_of(verts[3 * i + 2], grid.lo[2], grid.inv_h, grid.g[2]);
        const u64 slot = cells::find_or_insert(table, mask, cells::key_of(grid, cx, cy, cz), fresh);
        atomicMin(best + slot, (u64)i);
        leader[i] = (int64_t)slot;
    }
    cells::wave_count(count, fresh);
}

__global__ __launch_bounds__(256) void simp_leader_kernel(const u64* __restrict__ best, int64_t nv, int64_t* __restrict__ leader) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv) leader[i] = (int64_t)best[leader[i]];
}

__global__ __launch_bounds__(256) void simp_count_kernel(const int64_t* __restrict__ faces, int64_t nf, const int64_t* __restrict__ leader,
                                                         int64_t nv, u64* __restrict__ count) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool alive = false;
    if (f < nf) {
        const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if ((u64)i0 < (u64)nv && (u64)i1 < (u64)nv && (u64)i2 < (u64)nv) {
            const int64_t a = leader[i0], b = leader[i1], c = leader[i2];
            alive = a != b && b != c && a != c;
        }
    }
    cells::wave_count(count, alive);
}

__global__ __launch_bounds__(128) void simp_place_kernel(const double* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces,
                                                         const int64_t* __restrict__ cid, int64_t ncell, const int64_t* __restrict__ corner_order,
                                                         const int64_t* __restrict__ corner_off, const int64_t* __restrict__ vert_order,
                                                         const int64_t* __restrict__ vert_off, GridD grid, int mean_only, double* __restrict__ A,
                                                         double* __restrict__ bvec, double* __restrict__ xhat, double* __restrict__ pos,
                                                         uint8_t* __restrict__ fallback) {
    const int64_t c = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (c >= ncell) return;
    const int64_t v0 = vert_off[c], v1 = vert_off[c + 1];
    double ctr[3] = {0.0, 0.0, 0.0};
    double xh[3] = {0.0, 0.0, 0.0};
    if (v1 > v0) {                                                 // every cluster holds its leader; guard against a foreign CSR
        const int64_t first = vert_order[v0];
        for (int a = 0; a < 3; ++a)
            ctr[a] = grid.lo[a] + ((double)cell_of(verts[3 * first + a], grid.lo[a], grid.inv_h, grid.g[a]) + 0.5) * grid.h;
        for (int64_t p = v0; p < v1; ++p) {
            const int64_t v = vert_order[p];
            for (int a = 0; a < 3; ++a) xh[a] += verts[3 * v + a] - ctr[a];
        }
        const double m = (double)(v1 - v0);
        for (int a = 0; a < 3; ++a) xh[a] = xh[a] / m;
    }
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int64_t p = corner_off[c]; p < corner_off[c + 1]; ++p) {
        const int64_t e = corner_order[p];
        const int64_t f = e / 3;
        const int k = (int)(e - 3 * f);
        const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (k >= 1 && cid[i0] == c) continue;
        if (k == 2 && cid[i1] == c) continue;
        const double q0x = verts[3 * i0] - ctr[0], q0y = verts[3 * i0 + 1] - ctr[1], q0z = verts[3 * i0 + 2] - ctr[2];
        const double q1x = verts[3 * i1] - ctr[0], q1y = verts[3 * i1 + 1] - ctr[1], q1z = verts[3 * i1 + 2] - ctr[2];
        const double q2x = verts[3 * i2] - ctr[0], q2y = verts[3 * i2 + 1] - ctr[1], q2z = verts[3 * i2 + 2] - ctr[2];
        const double ux = q1x - q0x, uy = q1y - q0y, uz = q1z - q0z;
        const double wx = q2x - q0x, wy = q2y - q0y, wz = q2z - q0z;
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double m = (nx * q0x + ny * q0y) + nz * q0z;
        a00 += nx * nx; a01 += nx * ny; a02 += nx * nz; a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
        b0 += m * nx; b1 += m * ny; b2 += m * nz;
    }
    A[6 * c] = a00; A[6 * c + 1] = a01; A[6 * c + 2] = a02; A[6 * c + 3] = a11; A[6 * c + 4] = a12; A[6 * c + 5] = a22;
    bvec[3 * c] = b0; bvec[3 * c + 1] = b1; bvec[3 * c + 2] = b2;
    double x[3] = {xh[0], xh[1], xh[2]};
    uint8_t fell = 0;
    if (!mean_only) {
        const double trace = (a00 + a11) + a22;
        const double lambda = 1e-3 * trace;
        const double m00 = a00 + lambda, m11 = a11 + lambda, m22 = a22 + lambda, m01 = a01, m02 = a02, m12 = a12;
        const double r0 = b0 + lambda * xh[0], r1 = b1 + lambda * xh[1], r2 = b2 + lambda * xh[2];
        const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
        const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const double det = (m00 * c00 + m01 * c01) + m02 * c02;
        const double s0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        const double s1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        const double s2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        const double half = grid.h * 0.5;
        const double wall = half + half * 0x1p-30;
        // written so that a NaN fails the test: finite and inside the cell
        const bool ok = trace != 0.0 && fabs(s0) <= wall && fabs(s1) <= wall && fabs(s2) <= wall;
        if (ok) { x[0] = s0; x[1] = s1; x[2] = s2; } else fell = 1;
    }
    for (int a = 0; a < 3; ++a) {
        xhat[3 * c + a] = xh[a];
        pos[3 * c + a] = ctr[a] + x[a];
    }
    fallback[c] = fell;
}

}  // namespace

extern "C" {

int pps_simplify_leaders(const double* verts, int64_t nv, const double* lo, const double* hi, double h, double inv_h, uint64_t* table,
                         uint64_t* best, int64_t capacity, int64_t* leader, uint64_t* count, void* stream) {
    GridD grid;
    if (!verts || !table || !best || !leader || !count || !cells::table_ok(nv, capacity) || !cells::make_grid(lo, hi, h, inv_h, &grid))
        return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0xFF, (size_t)capacity * 8, st) != hipSuccess || hipMemsetAsync(best, 0xFF, (size_t)capacity * 8, st) != hipSuccess ||
        hipMemsetAsync(count, 0, 8, st) != hipSuccess)
        return PPS_ERR_LAUNCH;
    const unsigned blocks = (unsigned)((nv + 255) / 256);
    hipLaunchKernelGGL(simp_insert_kernel, dim3(blocks), dim3(256), 0, st, verts, nv, grid, (u64*)table, (u64*)best, (u64)(capacity - 1), leader,
                       (u64*)count);
    hipLaunchKernelGGL(simp_leader_kernel, dim3(blocks), dim3(256), 0, st, (const u64*)best, nv, leader);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_simplify_count(const int64_t* faces, int64_t nf, const int64_t* leader, int64_t nv, uint64_t* count, void* stream) {
    if (nf < 0 || nv < 1 || !leader || !count || (nf > 0 && !faces)) return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, 8, st) != hipSuccess) return PPS_ERR_LAUNCH;
    if (nf == 0) return PPS_OK;
    hipLaunchKernelGGL(simp_count_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, faces, nf, leader, nv, (u64*)count);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_simplify_place(const double* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* cid, int64_t ncell,
                       const int64_t* corner_order, const int64_t* corner_off, const int64_t* vert_order, const int64_t* vert_off, const double* lo,
                       const double* hi, double h, double inv_h, int mean_only, double* A, double* b, double* xhat, double* pos, uint8_t* fallback,
                       void* stream) {
    GridD grid;
    if (!verts || nv < 1 || nf < 0 || (nf > 0 && (!faces || !corner_order)) || !cid || ncell < 1 || ncell > nv || !corner_off || !vert_order ||
        !vert_off || !A || !b || !xhat || !pos || !fallback || !cells::make_grid(lo, hi, h, inv_h, &grid))
        return PPS_ERR_ARG;
    hipLaunchKernelGGL(simp_place_kernel, dim3((unsigned)((ncell + 127) / 128)), dim3(128), 0, (hipStream_t)stream, verts, nv, faces, cid, ncell,
                       corner_order, corner_off, vert_order, vert_off, grid, mean_only, A, b, xhat, pos, fallback);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
