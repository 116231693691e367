// Edge-collapse decimation for gfx950: quadric error metric, rounds of independent collapses.
//
// new capability: replaces nothing -- the reference has no decimation, and the vertex clustering of pps_simplify.hip stays as it is.  Driven
// by ppsurf_amd/decimate.py (the rows by ppsurf_amd/topology.py); restated in numpy by tests/decimate_spec.py, which the kernels match byte
// for byte.  Everything is fp64, every operation rounded on its own (-ffp-contract=off); no square root, no atomic, no sum whose order is
// not stated.
//
// A round works on the positions P f64 [nv,3], the current faces F int64 [nf,3] (all valid), their adjacency rows (offsets, nbr ascending,
// mult; src[e] the row of entry e) and their incidence rows (inc_offsets, inc ascending).
//   regular vertex  it has a face, every entry of its adjacency row has mult == 2, and its faces are as many as its neighbours.  Borders,
//                   non-manifold fans and everything that touches them have an end that is not regular: they are never moved.
//   candidate       an adjacency entry (a, b), a < b, both ends regular, that passes the link rule, has a finite cost and folds no face.
//   link rule       the rows of a and b share exactly two vertices c < d (one merge of the two ascending rows), and not (a face of a holds c
//                   and d, and a face of b holds c and d): the tetrahedron.
//   face list       the faces of a ascending, then the faces of b that do not hold a, ascending.  Walked twice from the rows in memory;
//                   nothing is gathered into a local buffer, so a vertex with 300 faces costs time and no registers.
//   placement       mid = (P_a + P_b) * 0.5.  Per face (i0, i1, i2) of the list: q_k = P_ik - mid, u = q_1 - q_0, w = q_2 - q_0,
//                   n = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x), m = (n_x q_0x + n_y q_0y) + n_z q_0z,
//                   A00 += n_x n_x, A01 += n_x n_y, A02 += n_x n_z, A11 += n_y n_y, A12 += n_y n_z, A22 += n_z n_z, b_k += m n_k.
//                   lambda = 1e-3 * ((A00 + A11) + A22), M = A + lambda I, r = b: the pull is towards x = 0, the midpoint.
//                   cofactors  c00 = M11 M22 - M12 M12,  c01 = M02 M12 - M01 M22,  c02 = M01 M12 - M02 M11,
//                              c11 = M00 M22 - M02 M02,  c12 = M01 M02 - M00 M12,  c22 = M00 M11 - M01 M01
//                   det = (M00 c00 + M01 c01) + M02 c02,  x_0 = ((c00 r_0 + c01 r_1) + c02 r_2) / det and so on (pps_simplify.hip).
//                   x = (0, 0, 0), a fallback, when the trace is 0, a component of x is not finite or (x_0^2 + x_1^2) + x_2^2 > |P_b - P_a|^2.
//   cost            second walk: t = ((n_x x_0 + n_y x_1) + n_z x_2) - m, cost = cost + t * t from +0.0: never negative.
//   fold rule       a face of the list that holds one end only, with that corner's q replaced by x, gives n'; the edge is no candidate
//                   unless (n_x n'_x + n_y n'_y) + n_z n'_z > 0 for each.
//   priority        (the bits of the cost, h(key), key) as three u64 compared lexicographically, key = (a << 32) | b, h the splitmix64
//                   finaliser of key + 0x9E3779B97F4A7C15.  Every other entry gets NONE = 2^64 - 1 three times.
//   winners         m1[u] = the minimum priority over the entries of row u (the entry (u, v) with u > v is read at its mirror (v, u), found
//                   by a binary search in row v); best[w] = the minimum of m1 over w and its row; an entry wins when best[a] == best[b] ==
//                   its priority != NONE.  Two winners never share or neighbour an end: if e = (a, b) and e' = (a', b') win and an end v of
//                   e is an end or a neighbour of an end v' of e', then m1[v] <= prio(e) and best[v'] <= m1[v] give prio(e') <= prio(e),
//                   and the other way round, so e = e' (priorities are distinct: they hold the key).  A collapse reads the positions and
//                   rows of {a, b}, N(a), N(b) only and moves a, b only, so the winners of a round are independent.
//   apply           P_a = mid + x, rename[b] = a (one thread per winner); every face renamed, keep = its three indices still differ (one
//                   thread per face).  The caller compacts the kept faces in their order.
// Every index is range-checked before it becomes an address; a row whose offsets are not 0 <= o0 <= o1 <= count is taken as empty.
#include <math.h>

#include "pps_collapse.h"
#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

using namespace pps_collapse;          // Prio and its order, mix, open_row, the link-rule merge, plane_of

__global__ __launch_bounds__(256) void regular_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ mult, int64_t ne,
                                                      const int64_t* __restrict__ inc_offsets, int64_t ni, int64_t nv, uint8_t* __restrict__ regular) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int64_t p, end, fp, fend;
    open_row(offsets, v, ne, p, end);
    open_row(inc_offsets, v, ni, fp, fend);
    bool ok = fend - fp >= 1 && fend - fp == end - p;
    for (; ok && p < end; ++p) ok = mult[p] == 2;
    regular[v] = ok ? 1 : 0;
}

// One thread per adjacency entry: rules (1) to (6).
__global__ __launch_bounds__(256) void edges_kernel(const double* __restrict__ pos, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                    const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr,
                                                    const int32_t* __restrict__ src, int64_t ne, const int64_t* __restrict__ inc_offsets,
                                                    const int32_t* __restrict__ inc, int64_t ni, const uint8_t* __restrict__ regular,
                                                    uint64_t* __restrict__ prio, double* __restrict__ xout, uint8_t* __restrict__ fell) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    Prio mine{NONE, NONE, NONE};
    double x[3] = {0.0, 0.0, 0.0};
    bool fallback = false;
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
        double mid[3], d2 = 0.0;
        {
            const double dx = pos[3 * b] - pos[3 * a], dy = pos[3 * b + 1] - pos[3 * a + 1], dz = pos[3 * b + 2] - pos[3 * a + 2];
            d2 = (dx * dx + dy * dy) + dz * dz;
#pragma unroll
            for (int k = 0; k < 3; ++k) mid[k] = (pos[3 * a + k] + pos[3 * b + k]) * 0.5;
        }
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, cost = 0.0;
        bool tet_a = false, tet_b = false, folds = false;
        for (int pass = 0; pass < 2; ++pass) {
            for (int part = 0; part < 2; ++part) {
                int64_t p, end;
                open_row(inc_offsets, part == 0 ? a : b, ni, p, end);
                for (; p < end; ++p) {
                    const int64_t t = inc[p];
                    if (t < 0 || t >= nf) continue;
                    const int64_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
                    if (!face_valid(i0, i1, i2, nv)) continue;
                    if (pass == 0 && (i0 == c || i1 == c || i2 == c) && (i0 == d || i1 == d || i2 == d)) {
                        if (part == 0) tet_a = true; else tet_b = true;
                    }
                    if (part == 1 && (i0 == a || i1 == a || i2 == a)) continue;
                    Plane f;
                    plane_of(pos, i0, i1, i2, mid, f);
                    if (pass == 0) {
                        a00 += f.n[0] * f.n[0]; a01 += f.n[0] * f.n[1]; a02 += f.n[0] * f.n[2];
                        a11 += f.n[1] * f.n[1]; a12 += f.n[1] * f.n[2]; a22 += f.n[2] * f.n[2];
                        b0 += f.m * f.n[0]; b1 += f.m * f.n[1]; b2 += f.m * f.n[2];
                        continue;
                    }
                    const double t1 = ((f.n[0] * x[0] + f.n[1] * x[1]) + f.n[2] * x[2]) - f.m;
                    cost += t1 * t1;
                    const bool e0 = i0 == a || i0 == b, e1 = i1 == a || i1 == b, e2 = i2 == a || i2 == b;
                    if ((int)e0 + (int)e1 + (int)e2 != 1) continue;
                    double g[3][3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        g[0][k] = e0 ? x[k] : f.q[0][k];
                        g[1][k] = e1 ? x[k] : f.q[1][k];
                        g[2][k] = e2 ? x[k] : f.q[2][k];
                    }
                    const double ux = g[1][0] - g[0][0], uy = g[1][1] - g[0][1], uz = g[1][2] - g[0][2];
                    const double wx = g[2][0] - g[0][0], wy = g[2][1] - g[0][1], wz = g[2][2] - g[0][2];
                    const double hx = uy * wz - uz * wy, hy = uz * wx - ux * wz, hz = ux * wy - uy * wx;
                    if (!((f.n[0] * hx + f.n[1] * hy) + f.n[2] * hz > 0.0)) folds = true;
                }
            }
            if (pass == 0) {
                const double trace = (a00 + a11) + a22;
                const double lambda = 1e-3 * trace;
                const double m00 = a00 + lambda, m11 = a11 + lambda, m22 = a22 + lambda, m01 = a01, m02 = a02, m12 = a12;
                const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
                const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
                const double det = (m00 * c00 + m01 * c01) + m02 * c02;
                const double s0 = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
                const double s1 = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
                const double s2 = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
                const bool ok = trace != 0.0 && is_finite(s0) && is_finite(s1) && is_finite(s2) && !((s0 * s0 + s1 * s1) + s2 * s2 > d2);
                if (ok) { x[0] = s0; x[1] = s1; x[2] = s2; }
                fallback = !ok;
            }
        }
        live = !(tet_a && tet_b) && is_finite(cost) && !folds;
        if (live) mine = prio_of(cost, a, b);
    }
    store_prio(prio, e, mine);
#pragma unroll
    for (int k = 0; k < 3; ++k) xout[3 * e + k] = live ? x[k] : 0.0;
    fell[e] = live && fallback ? 1 : 0;
}

// the entry of row v that names u, or -1: a binary search in the ascending row
__device__ __forceinline__ int64_t entry_of(const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr, int64_t ne, int64_t v, int64_t u) {
    int64_t lo, hi;
    open_row(offsets, v, ne, lo, hi);
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int32_t w = nbr[mid];
        if (w == u) return mid;
        if (w < u) lo = mid + 1; else hi = mid;
    }
    return -1;
}

__global__ __launch_bounds__(256) void vertex_min_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr, int64_t ne, int64_t nv,
                                                         const uint64_t* __restrict__ prio, uint64_t* __restrict__ m1) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= nv) return;
    Prio best{NONE, NONE, NONE};
    int64_t p, end;
    open_row(offsets, u, ne, p, end);
    for (; p < end; ++p) {
        const int64_t v = nbr[p];
        if (v < 0 || v >= nv || v == u) continue;
        const int64_t at = u < v ? p : entry_of(offsets, nbr, ne, v, u);
        if (at < 0) continue;
        const Prio q = load_prio(prio, at);
        if (less(q, best)) best = q;
    }
    store_prio(m1, u, best);
}

__global__ __launch_bounds__(256) void ring_min_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr, int64_t ne, int64_t nv,
                                                       const uint64_t* __restrict__ m1, uint64_t* __restrict__ best) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nv) return;
    Prio low = load_prio(m1, w);
    int64_t p, end;
    open_row(offsets, w, ne, p, end);
    for (; p < end; ++p) {
        const int64_t v = nbr[p];
        if (v < 0 || v >= nv) continue;
        const Prio q = load_prio(m1, v);
        if (less(q, low)) low = q;
    }
    store_prio(best, w, low);
}

__global__ __launch_bounds__(256) void winners_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ nbr, int64_t ne, int64_t nv,
                                                      const uint64_t* __restrict__ prio, const uint64_t* __restrict__ best, uint8_t* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const int64_t a = src[e], b = nbr[e];
    bool wins = false;
    if (a >= 0 && a < b && b < nv) {
        const Prio p = load_prio(prio, e);
        wins = !same(p, Prio{NONE, NONE, NONE}) && same(load_prio(best, a), p) && same(load_prio(best, b), p);
    }
    flag[e] = wins ? 1 : 0;
}

__global__ __launch_bounds__(256) void move_kernel(const int64_t* __restrict__ win, int64_t nw, const int32_t* __restrict__ src,
                                                   const int32_t* __restrict__ nbr, int64_t ne, const double* __restrict__ x, double* pos, int64_t nv,
                                                   int32_t* __restrict__ rename) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw) return;
    const int64_t e = win[i];
    if (e < 0 || e >= ne) return;
    const int64_t a = src[e], b = nbr[e];
    if (a < 0 || a >= b || b >= nv) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) pos[3 * a + k] = (pos[3 * a + k] + pos[3 * b + k]) * 0.5 + x[3 * e + k];
    rename[b] = (int32_t)a;
}

__global__ __launch_bounds__(256) void rename_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, const int32_t* __restrict__ rename,
                                                     int64_t* __restrict__ out, uint8_t* __restrict__ keep) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    bool ok = face_in_range(a, b, c, nv);
    if (ok) {
        a = rename[a];
        b = rename[b];
        c = rename[c];
        ok = face_valid(a, b, c, nv);
    }
    out[3 * f] = a;
    out[3 * f + 1] = b;
    out[3 * f + 2] = c;
    keep[f] = ok ? 1 : 0;
}

inline bool bad_count(int64_t n) { return n < 0 || n > (int64_t)INT32_MAX; }

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

inline int launched() { return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH; }

}  // namespace

extern "C" {

int ppsx_decimate_regular(const int64_t* offsets, const int32_t* mult, int64_t ne, const int64_t* inc_offsets, int64_t ni, int64_t nv,
                          uint8_t* regular, void* stream) {
    if (bad_count(nv) || ne < 0 || ni < 0) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    if (!offsets || !inc_offsets || !regular || (ne > 0 && !mult)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(regular_kernel, dim3(blocks_of(nv)), dim3(256), 0, (hipStream_t)stream, offsets, mult, ne, inc_offsets, ni, nv, regular);
    return launched();
}

int ppsx_decimate_edges(const double* pos, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* nbr,
                        const int32_t* src, int64_t ne, const int64_t* inc_offsets, const int32_t* inc, int64_t ni, const uint8_t* regular,
                        uint64_t* prio, double* x, uint8_t* fell, void* stream) {
    if (bad_count(nv) || bad_count(nf) || ne < 0 || ni < 0) return PPS_ERR_ARG;
    if (ne == 0) return PPS_OK;
    if (!nbr || !src || !prio || !x || !fell || (nv > 0 && (!pos || !offsets || !inc_offsets || !regular)) || (nf > 0 && !faces) || (ni > 0 && !inc))
        return PPS_ERR_ARG;
    hipLaunchKernelGGL(edges_kernel, dim3(blocks_of(ne)), dim3(256), 0, (hipStream_t)stream, pos, nv, faces, nf, offsets, nbr, src, ne, inc_offsets,
                       inc, ni, regular, prio, x, fell);
    return launched();
}

int ppsx_decimate_vertex_min(const int64_t* offsets, const int32_t* nbr, int64_t ne, int64_t nv, const uint64_t* prio, uint64_t* m1, void* stream) {
    if (bad_count(nv) || ne < 0) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    if (!offsets || !m1 || (ne > 0 && (!nbr || !prio))) return PPS_ERR_ARG;
    hipLaunchKernelGGL(vertex_min_kernel, dim3(blocks_of(nv)), dim3(256), 0, (hipStream_t)stream, offsets, nbr, ne, nv, prio, m1);
    return launched();
}

int ppsx_decimate_ring_min(const int64_t* offsets, const int32_t* nbr, int64_t ne, int64_t nv, const uint64_t* m1, uint64_t* best, void* stream) {
    if (bad_count(nv) || ne < 0) return PPS_ERR_ARG;
    if (nv == 0) return PPS_OK;
    if (!offsets || !m1 || !best || m1 == best || (ne > 0 && !nbr)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(ring_min_kernel, dim3(blocks_of(nv)), dim3(256), 0, (hipStream_t)stream, offsets, nbr, ne, nv, m1, best);
    return launched();
}

int ppsx_decimate_winners(const int32_t* src, const int32_t* nbr, int64_t ne, int64_t nv, const uint64_t* prio, const uint64_t* best, uint8_t* flag,
                          void* stream) {
    if (bad_count(nv) || ne < 0) return PPS_ERR_ARG;
    if (ne == 0) return PPS_OK;
    if (!src || !nbr || !prio || !flag || (nv > 0 && !best)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(winners_kernel, dim3(blocks_of(ne)), dim3(256), 0, (hipStream_t)stream, src, nbr, ne, nv, prio, best, flag);
    return launched();
}

int ppsx_decimate_move(const int64_t* win, int64_t nw, const int32_t* src, const int32_t* nbr, int64_t ne, const double* x, double* pos, int64_t nv,
                       int32_t* rename, void* stream) {
    if (bad_count(nv) || bad_count(nw) || ne < 0) return PPS_ERR_ARG;
    if (nw == 0) return PPS_OK;
    if (!win || (ne > 0 && (!src || !nbr || !x)) || (nv > 0 && (!pos || !rename))) return PPS_ERR_ARG;
    if (ne == 0 || nv == 0) return PPS_OK;
    hipLaunchKernelGGL(move_kernel, dim3(blocks_of(nw)), dim3(256), 0, (hipStream_t)stream, win, nw, src, nbr, ne, x, pos, nv, rename);
    return launched();
}

int ppsx_decimate_rename(const int64_t* faces, int64_t nf, int64_t nv, const int32_t* rename, int64_t* out, uint8_t* keep, void* stream) {
    if (bad_count(nv) || bad_count(nf)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !out || !keep || (nv > 0 && !rename)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(rename_kernel, dim3(blocks_of(nf)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, rename, out, keep);
    return launched();
}

}  // extern "C"
