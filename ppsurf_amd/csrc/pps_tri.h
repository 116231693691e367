// Point-triangle closest point, shared by the qualitative comparison (pps_vis.hip, T = float and double) and the trim by support
// (pps_trim.hip, T = double); DESIGN.md sections 10 and 15.  Restated in numpy (float64) by tests/trim_spec.py.
//
// Voronoi-region classification (Ericson, Real-Time Collision Detection, 5.1.5).  A face with |e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2 (zero or
// next to zero area) is its longest edge.  Every operation is in T and rounded on its own (-ffp-contract=off).
#pragma once
#include "pps_common.h"

namespace {

template <typename T> struct V3 { T x, y, z; };
template <typename T> __host__ __device__ __forceinline__ V3<T> sub(V3<T> a, V3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T> __host__ __device__ __forceinline__ T dot(V3<T> a, V3<T> b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
template <typename T> __host__ __device__ __forceinline__ V3<T> cross(V3<T> a, V3<T> b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename T> __device__ __forceinline__ T clamp01(T v) { return v < T(0) ? T(0) : (v > T(1) ? T(1) : v); }

// Closest point of p on triangle (a, b, c) as a + s ab + t ac; d2 = its squared distance (the interior region as the plane distance).
template <typename T>
__device__ __forceinline__ void closest_on_triangle(V3<T> p, V3<T> a, V3<T> b, V3<T> c, T& s, T& t, T& d2) {
    const V3<T> ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
    const V3<T> n = cross(ab, ac);
    const T nn = dot(n, n), lab = dot(ab, ab), lac = dot(ac, ac);
    if (!(nn > T(1e-12) * (lab * lac))) {                     // degenerate: the longest edge (face-uniform branch)
        const T lbc = dot(bc, bc);
        V3<T> o = a, e = ab;
        T le = lab;
        int which = 0;
        if (lac > le) { e = ac; le = lac; which = 1; }
        if (lbc > le) { o = b; e = bc; le = lbc; which = 2; }
        const T u = le > T(0) ? clamp01(dot(sub(p, o), e) / le) : T(0);
        s = which == 0 ? u : (which == 1 ? T(0) : T(1) - u);
        t = which == 0 ? T(0) : u;
        const V3<T> q = {o.x + u * e.x, o.y + u * e.y, o.z + u * e.z};
        const V3<T> dq = sub(p, q);
        d2 = dot(dq, dq);
        return;
    }
    const V3<T> ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
    const T d1 = dot(ab, ap), d2_ = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
    const T vc = d1 * d4 - d3 * d2_, vb = d5 * d2_ - d1 * d6, va = d3 * d6 - d5 * d4;
    bool interior = false;
    if (d1 <= T(0) && d2_ <= T(0)) { s = T(0); t = T(0); }                                    // vertex a
    else if (d3 >= T(0) && d4 <= d3) { s = T(1); t = T(0); }                                  // vertex b
    else if (vc <= T(0) && d1 >= T(0) && d3 <= T(0)) { s = clamp01(d1 / (d1 - d3)); t = T(0); }   // edge ab
    else if (d6 >= T(0) && d5 <= d6) { s = T(0); t = T(1); }                                  // vertex c
    else if (vb <= T(0) && d2_ >= T(0) && d6 <= T(0)) { s = T(0); t = clamp01(d2_ / (d2_ - d6)); }  // edge ac
    else if (va <= T(0) && (d4 - d3) >= T(0) && (d5 - d6) >= T(0)) {                           // edge bc
        const T w = clamp01((d4 - d3) / ((d4 - d3) + (d5 - d6)));
        s = T(1) - w; t = w;
    } else {                                                                                  // interior
        const T den = va + vb + vc;
        s = den > T(0) ? clamp01(vb / den) : T(0);
        t = den > T(0) ? clamp01(vc / den) : T(0);
        if (s + t > T(1)) { const T k = T(1) / (s + t); s *= k; t *= k; }
        interior = true;
    }
    if (interior) {
        const T h = dot(ap, n);
        d2 = h * h / nn;
    } else {
        const V3<T> q = {(a.x + s * ab.x) + t * ac.x, (a.y + s * ab.y) + t * ac.y, (a.z + s * ab.z) + t * ac.z};
        const V3<T> dq = sub(p, q);
        d2 = dot(dq, dq);
    }
}

}  // namespace
