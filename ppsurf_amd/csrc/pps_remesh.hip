// Isotropic remeshing for gfx950: the candidates of the short-edge collapse and the tangential relaxation.
//
// new capability: replaces nothing -- the reference has no remeshing, and decimate, flip, subdivide and smooth stay as they are.  Driven by
// ppsurf_amd/remesh.py (the rows by ppsurf_amd/topology.py, the rest of a collapse round by the entries of pps_decimate.hip); restated in
// numpy by tests/remesh_spec.py, which the kernels match byte for byte.  Everything is fp64, every operation rounded on its own
// (-ffp-contract=off); no square root, no atomic, no LDS, no sum whose order is not stated.
//
// Short edges, one thread per adjacency entry (a, b) = (src[e], nbr[e]) of the rows of section 22:
//   candidate       a < b, both ends regular, the link rule of section 22 (exactly two common neighbours c < d, not the tetrahedron), short,
//                   folds no face and stretches no edge.
//   short           len2 = (dx dx + dy dy) + dz dz < min2, d = P_b - P_a; len2 == 0 qualifies.
//   placement       mid = (P_a + P_b) * 0.5 and nothing else: no quadric, no fallback.  In the frame of section 22 that is x = (0, 0, 0).
//   fold rule       section 22's at x = 0: the faces of a ascending, then the faces of b that do not hold a; one that holds one end only, with
//                   that corner at mid, gives n' and the entry is no candidate unless (n_x n'_x + n_y n'_y) + n_z n'_z > 0 for each.  A face
//                   without area at an end has n = 0 and therefore blocks the collapse; the two faces on the edge itself are not asked.
//   length guard    every w of the rows of a and b other than a and b: q = P_w - mid, (q_x q_x + q_y q_y) + q_z q_z <= max2, or the entry is
//                   no candidate (Botsch and Kobbelt: a collapse must not make an edge that the next split would cut again).  max2 = +inf
//                   switches the guard off.
//   priority        (the bits of len2, h(key), key), section 22's layout, the shortest first; NONE three times for every other entry.  The
//                   vertex minimum, the ring minimum, the winners, the move (with x = 0) and the rename are section 22's entries unchanged,
//                   and so is the argument that the winners of a round are independent: the two guards read {a, b}, N(a) and N(b) only.
//
// Relaxation, one thread per vertex, a Jacobi pass from x to y with a state per vertex:
//   state 0         v is not regular (a border, a non-manifold fan, no face): copied bit for bit.
//   move            s = the sum of P_w over the adjacency row, ascending, from +0.0; c = s / count; d = c - P_v.
//                   N = the sum over the incidence row, ascending, from +0.0 of n = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x),
//                   u = P_i1 - P_i0, w = P_i2 - P_i0; nn = (N_x N_x + N_y N_y) + N_z N_z, nd = (N_x d_x + N_y d_y) + N_z d_z, r = nd / nn,
//                   t_k = d_k - N_k * r, P'_k = P_v,k + lam * t_k: the Laplacian step without its part along the area-weighted normal.
//   state 2         nn is 0 or not finite, or a t_k is not finite: copied.
//   state 3         on a second walk of the incidence row some face, its corners at v replaced by P' and the others where they were before
//                   the pass, has n' with not (n_x n'_x + n_y n'_y) + n_z n'_z > 0: copied.  The neighbours move in the same pass, so this
//                   guard is a filter, not a proof that no face folds.
//   state 1         moved: y_v = P'.
// Every index is range-checked before it becomes an address; a row whose offsets are not 0 <= o0 <= o1 <= count is taken as empty, and an
// entry out of range is neither read through nor counted.
#include <math.h>

#include "pps_collapse.h"
#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

using namespace pps_collapse;

__global__ __launch_bounds__(256) void short_edges_kernel(const double* __restrict__ pos, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                          const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr,
                                                          const int32_t* __restrict__ src, int64_t ne, const int64_t* __restrict__ inc_offsets,
                                                          const int32_t* __restrict__ inc, int64_t ni, const uint8_t* __restrict__ regular,
                                                          double min2, double max2, uint64_t* __restrict__ prio) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    Prio mine{NONE, NONE, NONE};
    const int64_t a = src[e], b = nbr[e];
    bool live = a >= 0 && a < b && b < nv && regular[a] != 0 && regular[b] != 0;
    int64_t c = -1, d = -1;
    if (live) {                                                      // the link rule: the common neighbours by a merge
        const Common both = common_neighbours(offsets, nbr, ne, a, b);
        c = both.c;
        d = both.d;
        live = both.count == 2;
    }
    if (live) {
        const double dx = pos[3 * b] - pos[3 * a], dy = pos[3 * b + 1] - pos[3 * a + 1], dz = pos[3 * b + 2] - pos[3 * a + 2];
        const double len2 = (dx * dx + dy * dy) + dz * dz;
        live = len2 < min2;
        if (live) {
            double mid[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) mid[k] = (pos[3 * a + k] + pos[3 * b + k]) * 0.5;
            bool tet_a = false, tet_b = false, folds = false, longer = false;
            for (int part = 0; part < 2; ++part) {
                const int64_t end_v = part == 0 ? a : b;
                int64_t p, end;
                open_row(inc_offsets, end_v, ni, p, end);
                for (; p < end; ++p) {
                    const int64_t t = inc[p];
                    if (t < 0 || t >= nf) continue;
                    const int64_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
                    if (!face_valid(i0, i1, i2, nv)) continue;
                    if ((i0 == c || i1 == c || i2 == c) && (i0 == d || i1 == d || i2 == d)) {
                        if (part == 0) tet_a = true; else tet_b = true;
                    }
                    if (part == 1 && (i0 == a || i1 == a || i2 == a)) continue;
                    const bool e0 = i0 == a || i0 == b, e1 = i1 == a || i1 == b, e2 = i2 == a || i2 == b;
                    if ((int)e0 + (int)e1 + (int)e2 != 1) continue;
                    Plane f;
                    plane_of(pos, i0, i1, i2, mid, f);
                    if (!(turn_at_mid(f, e0, e1, e2) > 0.0)) folds = true;
                }
                open_row(offsets, end_v, ne, p, end);
                for (; p < end; ++p) {                               // the length guard over the row of this end
                    const int64_t w = nbr[p];
                    if (w < 0 || w >= nv || w == a || w == b) continue;
                    const double qx = pos[3 * w] - mid[0], qy = pos[3 * w + 1] - mid[1], qz = pos[3 * w + 2] - mid[2];
                    if (!((qx * qx + qy * qy) + qz * qz <= max2)) longer = true;
                }
            }
            live = !(tet_a && tet_b) && !folds && !longer;
            if (live) mine = prio_of(len2, a, b);
        }
    }
    store_prio(prio, e, mine);
}

__global__ __launch_bounds__(256) void relax_pass_kernel(const double* __restrict__ x, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                         const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr, int64_t ne,
                                                         const int64_t* __restrict__ inc_offsets, const int32_t* __restrict__ inc, int64_t ni,
                                                         const uint8_t* __restrict__ regular, double lam, double* __restrict__ y,
                                                         uint8_t* __restrict__ state) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const double pv[3] = {x[3 * v], x[3 * v + 1], x[3 * v + 2]};
    double out[3] = {pv[0], pv[1], pv[2]};
    uint8_t st = 0;
    if (regular[v] != 0) {
        double s[3] = {0.0, 0.0, 0.0}, nsum[3] = {0.0, 0.0, 0.0};
        int64_t count = 0, p, end;
        open_row(offsets, v, ne, p, end);
        for (; p < end; ++p) {
            const int64_t w = nbr[p];
            if (w < 0 || w >= nv) continue;
            s[0] = s[0] + x[3 * w];
            s[1] = s[1] + x[3 * w + 1];
            s[2] = s[2] + x[3 * w + 2];
            ++count;
        }
        int64_t fp, fend;
        open_row(inc_offsets, v, ni, fp, fend);
        for (p = fp; p < fend; ++p) {
            const int64_t t = inc[p];
            if (t < 0 || t >= nf) continue;
            const int64_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
            if (!face_valid(i0, i1, i2, nv)) continue;
            const double ux = x[3 * i1] - x[3 * i0], uy = x[3 * i1 + 1] - x[3 * i0 + 1], uz = x[3 * i1 + 2] - x[3 * i0 + 2];
            const double wx = x[3 * i2] - x[3 * i0], wy = x[3 * i2 + 1] - x[3 * i0 + 1], wz = x[3 * i2 + 2] - x[3 * i0 + 2];
            nsum[0] = nsum[0] + (uy * wz - uz * wy);
            nsum[1] = nsum[1] + (uz * wx - ux * wz);
            nsum[2] = nsum[2] + (ux * wy - uy * wx);
        }
        const double cnt = (double)count;
        const double d0 = s[0] / cnt - pv[0], d1 = s[1] / cnt - pv[1], d2 = s[2] / cnt - pv[2];
        const double nn = (nsum[0] * nsum[0] + nsum[1] * nsum[1]) + nsum[2] * nsum[2];
        const double nd = (nsum[0] * d0 + nsum[1] * d1) + nsum[2] * d2;
        const double r = nd / nn;
        const double t0 = d0 - nsum[0] * r, t1 = d1 - nsum[1] * r, t2 = d2 - nsum[2] * r;
        if (nn == 0.0 || !is_finite(nn) || !is_finite(t0) || !is_finite(t1) || !is_finite(t2)) {
            st = 2;
        } else {
            const double q[3] = {pv[0] + lam * t0, pv[1] + lam * t1, pv[2] + lam * t2};
            bool folds = false;
            for (p = fp; p < fend; ++p) {
                const int64_t t = inc[p];
                if (t < 0 || t >= nf) continue;
                const int64_t idx[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
                if (!face_valid(idx[0], idx[1], idx[2], nv)) continue;
                double g[3][3], h[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        g[c][k] = x[3 * idx[c] + k];
                        h[c][k] = idx[c] == v ? q[k] : g[c][k];
                    }
                }
                const double ux = g[1][0] - g[0][0], uy = g[1][1] - g[0][1], uz = g[1][2] - g[0][2];
                const double wx = g[2][0] - g[0][0], wy = g[2][1] - g[0][1], wz = g[2][2] - g[0][2];
                const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                const double ax = h[1][0] - h[0][0], ay = h[1][1] - h[0][1], az = h[1][2] - h[0][2];
                const double bx = h[2][0] - h[0][0], by = h[2][1] - h[0][1], bz = h[2][2] - h[0][2];
                const double mx = ay * bz - az * by, my = az * bx - ax * bz, mz = ax * by - ay * bx;
                if (!((nx * mx + ny * my) + nz * mz > 0.0)) folds = true;
            }
            st = folds ? 3 : 1;
            if (!folds) {
                out[0] = q[0];
                out[1] = q[1];
                out[2] = q[2];
            }
        }
    }
    y[3 * v] = out[0];
    y[3 * v + 1] = out[1];
    y[3 * v + 2] = out[2];
    state[v] = st;
}

inline bool bad_count(int64_t n) { return n < 0 || n > (int64_t)INT32_MAX; }

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

inline int launched() { return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH; }

}  // namespace

extern "C" {

int ppsx_remesh_short_edges(const double* pos, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* nbr,
                            const int32_t* src, int64_t ne, const int64_t* inc_offsets, const int32_t* inc, int64_t ni, const uint8_t* regular,
                            double min2, double max2, uint64_t* prio, void* stream) {
    if (bad_count(nv) || bad_count(nf) || bad_count(ne) || ni < 0 || !(min2 >= 0.0) || !(max2 >= 0.0)) return PPS_ERR_ARG;
    if (ne == 0) return PPS_OK;
    if (!nbr || !src || !prio || (nv > 0 && (!pos || !offsets || !inc_offsets || !regular)) || (nf > 0 && !faces) || (ni > 0 && !inc))
        return PPS_ERR_ARG;
    hipLaunchKernelGGL(short_edges_kernel, dim3(blocks_of(ne)), dim3(256), 0, (hipStream_t)stream, pos, nv, faces, nf, offsets, nbr, src, ne,
                       inc_offsets, inc, ni, regular, min2, max2, prio);
    return launched();
}

int ppsx_remesh_relax_pass(const double* x, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* nbr, int64_t ne,
                           const int64_t* inc_offsets, const int32_t* inc, int64_t ni, const uint8_t* regular, double lam, double* y,
                           uint8_t* state, void* stream) {
    if (bad_count(nv) || bad_count(nf) || ne < 0 || ni < 0 || !(lam > 0.0 && lam <= 1.0)) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    if (!x || !offsets || !inc_offsets || !regular || !y || !state || x == y || (nf > 0 && !faces) || (ne > 0 && !nbr) || (ni > 0 && !inc))
        return PPS_ERR_ARG;
    hipLaunchKernelGGL(relax_pass_kernel, dim3(blocks_of(nv)), dim3(256), 0, (hipStream_t)stream, x, nv, faces, nf, offsets, nbr, ne, inc_offsets,
                       inc, ni, regular, lam, y, state);
    return launched();
}

}  // extern "C"
