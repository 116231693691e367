// What the candidate kernels of the two edge-collapse stages share (pps_decimate.hip; pps_remesh.hip, section 30): the
// priority triple and its order, the splitmix64 finaliser, the checked row bounds, the link-rule merge and the plane of a face about a
// midpoint.  Everything is fp64, every operation rounded on its own.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace pps_collapse {

typedef unsigned long long u64;
constexpr u64 NONE = ~0ull;

struct Prio {
    u64 cost, hash, key;
};

__device__ __forceinline__ bool less(const Prio& p, const Prio& q) {
    if (p.cost != q.cost) return p.cost < q.cost;
    if (p.hash != q.hash) return p.hash < q.hash;
    return p.key < q.key;
}

__device__ __forceinline__ bool same(const Prio& p, const Prio& q) { return p.cost == q.cost && p.hash == q.hash && p.key == q.key; }

__device__ __forceinline__ Prio load_prio(const uint64_t* __restrict__ t, int64_t i) { return Prio{t[3 * i], t[3 * i + 1], t[3 * i + 2]}; }

__device__ __forceinline__ void store_prio(uint64_t* __restrict__ t, int64_t i, const Prio& p) {
    t[3 * i] = p.cost;
    t[3 * i + 1] = p.hash;
    t[3 * i + 2] = p.key;
}

__device__ __forceinline__ u64 mix(u64 key) {
    u64 z = key + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The priority of the entry (a, b), a < b, with the fp64 `cost` in its first word.
__device__ __forceinline__ Prio prio_of(double cost, int64_t a, int64_t b) {
    const u64 key = ((u64)a << 32) | (u64)b;
    return Prio{(u64)__double_as_longlong(cost), mix(key), key};
}

__device__ __forceinline__ void open_row(const int64_t* __restrict__ offsets, int64_t v, int64_t count, int64_t& p, int64_t& end) {
    const int64_t o0 = offsets[v], o1 = offsets[v + 1];
    const bool ok = o0 >= 0 && o0 <= o1 && o1 <= count;
    p = ok ? o0 : 0;
    end = ok ? o1 : 0;
}

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < (double)INFINITY; }          // false for a NaN

// The link rule's merge: how many entries the ascending rows of a and b share, and the first two of them (-1 where there is none).
struct Common {
    int count;
    int64_t c, d;
};

__device__ __forceinline__ Common common_neighbours(const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr, int64_t ne, int64_t a,
                                                    int64_t b) {
    int64_t pa, ea, pb, eb;
    open_row(offsets, a, ne, pa, ea);
    open_row(offsets, b, ne, pb, eb);
    Common out{0, -1, -1};
    while (pa < ea && pb < eb) {
        const int32_t va = nbr[pa], vb = nbr[pb];
        if (va == vb) {
            if (out.count == 0) out.c = va;
            if (out.count == 1) out.d = va;
            ++out.count;
        }
        pa += va <= vb;
        pb += vb <= va;
    }
    return out;
}

// The corners of a face relative to mid, its normal and its plane offset.
struct Plane {
    double q[3][3], n[3], m;
};

__device__ __forceinline__ void plane_of(const double* __restrict__ pos, int64_t i0, int64_t i1, int64_t i2, const double mid[3], Plane& f) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f.q[0][k] = pos[3 * i0 + k] - mid[k];
        f.q[1][k] = pos[3 * i1 + k] - mid[k];
        f.q[2][k] = pos[3 * i2 + k] - mid[k];
    }
    const double ux = f.q[1][0] - f.q[0][0], uy = f.q[1][1] - f.q[0][1], uz = f.q[1][2] - f.q[0][2];
    const double wx = f.q[2][0] - f.q[0][0], wy = f.q[2][1] - f.q[0][1], wz = f.q[2][2] - f.q[0][2];
    f.n[0] = uy * wz - uz * wy;
    f.n[1] = uz * wx - ux * wz;
    f.n[2] = ux * wy - uy * wx;
    f.m = (f.n[0] * f.q[0][0] + f.n[1] * f.q[0][1]) + f.n[2] * f.q[0][2];
}

// (n . n') of the face f with the corners flagged e0, e1, e2 moved onto mid, the origin of f.q: positive when the face keeps its side.
__device__ __forceinline__ double turn_at_mid(const Plane& f, bool e0, bool e1, bool e2) {
    const double g0x = e0 ? 0.0 : f.q[0][0], g0y = e0 ? 0.0 : f.q[0][1], g0z = e0 ? 0.0 : f.q[0][2];
    const double g1x = e1 ? 0.0 : f.q[1][0], g1y = e1 ? 0.0 : f.q[1][1], g1z = e1 ? 0.0 : f.q[1][2];
    const double g2x = e2 ? 0.0 : f.q[2][0], g2y = e2 ? 0.0 : f.q[2][1], g2z = e2 ? 0.0 : f.q[2][2];
    const double ux = g1x - g0x, uy = g1y - g0y, uz = g1z - g0z;
    const double wx = g2x - g0x, wy = g2y - g0y, wz = g2z - g0z;
    const double hx = uy * wz - uz * wy, hy = uz * wx - ux * wz, hz = ux * wy - uy * wx;
    return (f.n[0] * hx + f.n[1] * hy) + f.n[2] * hz;
}

}  // namespace pps_collapse
