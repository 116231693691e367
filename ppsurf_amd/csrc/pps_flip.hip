// Delaunay edge flips for gfx950: sliver triangles are repaired by turning the diagonal of a quad, in rounds of independent flips (DESIGN.md
// section 27).
//
// new capability: replaces nothing -- the reference has no such stage and every other mesh stage keeps or removes the connectivity it is
// given.  Driven by ppsurf_amd/flip.py (the edges, their owners and slots by ppsurf_amd/topology.py); restated in numpy by tests/flip_spec.py,
// which the kernels match byte for byte.
//
// The rule, per round: vertices V f32 [nv,3] (finite), the working faces F int64 [nf,3], nv, nf <= 2^31 - 1, cos2, min_gain doubles.
//   edges      the distinct undirected edges of the valid faces (pps_faces.h) in ascending key (min << 32) | max with their owners.  Only an
//              edge with EXACTLY TWO owners can flip; its rank r is its position among those edges in ascending key.  Borders and
//              many-owner edges are never touched, and no flip changes the owner count of any other edge.
//   quad       f < g the two owners (the sort decides which one the pair list names first; the kernel puts them in order), k and l the slot
//              of the edge in each (slot k is corner k -> corner k + 1 mod 3): a = F[f][k], b = F[f][k + 1], c = F[f][k + 2].  The pair takes
//              part only when F[g][l] == b and F[g][l + 1] == a -- the two faces run the edge in opposite ways -- and then d = F[g][l + 2].
//   topology   c != d, and {c, d} is no edge of F: a binary search of its key in the ascending distinct keys.
//   geometry   P = double(V).  n1 = (P_b - P_a) x (P_c - P_a), n2 = (P_a - P_b) x (P_d - P_b): the normals of the two faces;
//              m1 = (P_d - P_a) x (P_c - P_a), m2 = (P_c - P_b) x (P_d - P_b): those of the two new faces; N = n1 + n2.
//              fold guard    m1.N > 0 and m2.N > 0.
//              crease guard  t = n1.n2, A = n1.n1, B = n2.n2: t >= 0 and t t >= cos2 (A B).  A face without area passes (0 >= 0).
//   criterion  p = (P_a - P_c).(P_b - P_c), q = (P_a - P_d).(P_b - P_d), s = p / sqrt(A) + q / sqrt(B), the sum of the cotangents of the
//              angles opposite the edge.  A candidate iff s < -min_gain (false for a NaN: inf - inf and 0 / 0 are no candidates).
//   priority   one u64, the smallest first: ((0x7F800000 - bits(f32(-s))) << 32) | fmix32(r).  -s is positive, the bits of positive floats
//              are monotone, and fmix32 (murmur3's finaliser) is a bijection: no two edges share a priority.  NONE = 2^64 - 1.
//   winners    vmin[v] = the minimum priority over the candidates whose quad {a, b, c, d} holds v.  An edge wins iff vmin equals its
//              priority at all four of its vertices.  Two winners share no quad vertex (they would share the priority vmin[v]), hence no
//              face, and the edges they create are different and have both ends outside the other's quad.
//   apply      F[f] = (a, d, c), F[g] = (b, c, d): the windings stay coherent, each face keeps its end of the old edge first.
// fp64 throughout, every operation rounded on its own (-ffp-contract=off); a cross is written out component by component, a dot is
// (x x' + y y') + z z'; sqrt and the division are IEEE.  No floating-point atomics: the one atomic is a 64-bit integer minimum of unique
// values, which is exact in any order.  A pure function of (V, F, cos2, min_gain): no dependence on the launch shape or on timing.
//
// Shape: one thread per pair in all three kernels, 256 threads per workgroup, plain vector loads and stores, no LDS.  The minimum per vertex
// is an atomicMin and no gather over incidence rows: the rows would cost a second sort per round, the candidates are a small part of the
// pairs after the first round, and four atomics per candidate onto distinct addresses do not queue.  Every index -- the faces, the slots,
// the four vertices, the quad entries on the way back in -- is range-checked before it becomes an address; the rank is the thread's own
// pair index, below np <= 2^31 - 1.  A pair that fails a check is no candidate.
#include <math.h>

#include "pps_common.h"
#include "pps_faces.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

typedef unsigned long long u64;

constexpr u64 NONE = ~0ull;
constexpr uint32_t INF_BITS = 0x7F800000u;

struct D3 {
    double x, y, z;
};

__device__ __forceinline__ D3 point(const float* __restrict__ verts, int64_t v) {
    return D3{(double)verts[3 * v], (double)verts[3 * v + 1], (double)verts[3 * v + 2]};
}
__device__ __forceinline__ D3 sub(D3 p, D3 q) { return D3{p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ D3 add(D3 p, D3 q) { return D3{p.x + q.x, p.y + q.y, p.z + q.z}; }
__device__ __forceinline__ D3 cross(D3 u, D3 w) { return D3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x}; }
__device__ __forceinline__ double dot(D3 p, D3 q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; }

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// whether `key` is one of keys[0 .. ne), ascending
__device__ __forceinline__ bool has_key(const int64_t* __restrict__ keys, int64_t ne, int64_t key) {
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < ne && keys[lo] == key;
}

// the priority of pair i, NONE when it is no candidate; q = (a, b, c, d) when it is one
__device__ __forceinline__ u64 pair_priority(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                             const int32_t* __restrict__ fa, const int32_t* __restrict__ fb, const int32_t* __restrict__ ea,
                                             const int32_t* __restrict__ eb, int64_t i, const int64_t* __restrict__ keys, int64_t ne, double cos2,
                                             double min_gain, int64_t q[4]) {
    int64_t f = fa[i], g = fb[i];
    int k = ea[i], l = eb[i];
    if (f < 0 || f >= nf || g < 0 || g >= nf || f == g || k < 0 || k > 2 || l < 0 || l > 2) return NONE;
    if (f > g) {
        const int64_t t = f; f = g; g = t;
        const int u = k; k = l; l = u;
    }
    const int64_t a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3], c = faces[3 * f + (k + 2) % 3];
    const int64_t gb = faces[3 * g + l], ga = faces[3 * g + (l + 1) % 3], d = faces[3 * g + (l + 2) % 3];
    if (!face_valid(a, b, c, nv) || !face_valid(gb, ga, d, nv)) return NONE;
    if (gb != b || ga != a || c == d) return NONE;
    if (has_key(keys, ne, ((c < d ? c : d) << 32) | (c < d ? d : c))) return NONE;
    const D3 Pa = point(verts, a), Pb = point(verts, b), Pc = point(verts, c), Pd = point(verts, d);
    const D3 n1 = cross(sub(Pb, Pa), sub(Pc, Pa)), n2 = cross(sub(Pa, Pb), sub(Pd, Pb));
    const D3 m1 = cross(sub(Pd, Pa), sub(Pc, Pa)), m2 = cross(sub(Pc, Pb), sub(Pd, Pb));
    const D3 N = add(n1, n2);
    if (!(dot(m1, N) > 0.0) || !(dot(m2, N) > 0.0)) return NONE;
    const double t = dot(n1, n2), A = dot(n1, n1), B = dot(n2, n2);
    if (!(t >= 0.0) || !(t * t >= cos2 * (A * B))) return NONE;
    const double p = dot(sub(Pa, Pc), sub(Pb, Pc)), r = dot(sub(Pa, Pd), sub(Pb, Pd));
    const double s = p / sqrt(A) + r / sqrt(B);
    if (!(s < -min_gain)) return NONE;
    q[0] = a; q[1] = b; q[2] = c; q[3] = d;
    const uint32_t high = INF_BITS - __float_as_uint((float)(-s));
    return ((u64)high << 32) | (u64)fmix32((uint32_t)i);
}

__global__ __launch_bounds__(256) void candidates_kernel(const float* __restrict__ verts, int64_t nv, const int64_t* __restrict__ faces, int64_t nf,
                                                         const int32_t* __restrict__ fa, const int32_t* __restrict__ fb,
                                                         const int32_t* __restrict__ ea, const int32_t* __restrict__ eb, int64_t np,
                                                         const int64_t* __restrict__ keys, int64_t ne, double cos2, double min_gain,
                                                         u64* __restrict__ prio, int32_t* __restrict__ quad, u64* vmin) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    int64_t q[4] = {0, 0, 0, 0};
    const u64 mine = pair_priority(verts, nv, faces, nf, fa, fb, ea, eb, i, keys, ne, cos2, min_gain, q);
    prio[i] = mine;
#pragma unroll
    for (int j = 0; j < 4; ++j) quad[4 * i + j] = (int32_t)q[j];
    if (mine == NONE) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicMin(vmin + q[j], mine);                  // q[j] lies in [0, nv): both faces are valid
}

__global__ __launch_bounds__(256) void winners_kernel(const u64* __restrict__ prio, const int32_t* __restrict__ quad, int64_t np,
                                                      const u64* __restrict__ vmin, int64_t nv, uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const u64 mine = prio[i];
    bool win = mine != NONE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t v = quad[4 * i + j];
        win = win && v >= 0 && v < nv && vmin[v] == mine;
    }
    flag[i] = win ? 1 : 0;
}

__global__ __launch_bounds__(256) void apply_kernel(const int32_t* __restrict__ fa, const int32_t* __restrict__ fb, const int32_t* __restrict__ quad,
                                                    const uint8_t* __restrict__ flag, int64_t np, int64_t nv, int64_t* faces, int64_t nf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np || flag[i] == 0) return;
    int64_t f = fa[i], g = fb[i];
    if (f < 0 || f >= nf || g < 0 || g >= nf || f == g) return;
    if (f > g) {
        const int64_t t = f; f = g; g = t;
    }
    const int64_t a = quad[4 * i], b = quad[4 * i + 1], c = quad[4 * i + 2], d = quad[4 * i + 3];
    if (!face_in_range(a, b, c, nv) || d < 0 || d >= nv) return;
    faces[3 * f] = a;
    faces[3 * f + 1] = d;
    faces[3 * f + 2] = c;
    faces[3 * g] = b;
    faces[3 * g + 1] = c;
    faces[3 * g + 2] = d;
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }
inline unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int ppsx_flip_candidates(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int32_t* fa, const int32_t* fb, const int32_t* ea,
                         const int32_t* eb, int64_t np, const int64_t* keys, int64_t ne, double cos2, double min_gain, uint64_t* prio, int32_t* quad,
                         uint64_t* vmin, void* stream) {
    if (np < 0 || nv < 0 || nf < 0 || ne < 0 || too_many(np) || too_many(nv) || too_many(nf) || ne > 3 * (int64_t)INT32_MAX) return PPS_ERR_ARG;
    if (np == 0) return PPS_OK;
    if (!fa || !fb || !ea || !eb || !prio || !quad || (nv > 0 && (!verts || !vmin)) || (nf > 0 && !faces) || (ne > 0 && !keys)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(candidates_kernel, dim3(grid_of(np, 256)), dim3(256), 0, (hipStream_t)stream, verts, nv, faces, nf, fa, fb, ea, eb, np, keys, ne,
                       cos2, min_gain, (u64*)prio, quad, (u64*)vmin);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_flip_winners(const uint64_t* prio, const int32_t* quad, int64_t np, const uint64_t* vmin, int64_t nv, uint8_t* flag, void* stream) {
    if (np < 0 || nv < 0 || too_many(np) || too_many(nv)) return PPS_ERR_ARG;
    if (np == 0) return PPS_OK;
    if (!prio || !quad || !flag || (nv > 0 && !vmin)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(winners_kernel, dim3(grid_of(np, 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)prio, quad, np, (const u64*)vmin, nv, flag);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_flip_apply(const int32_t* fa, const int32_t* fb, const int32_t* quad, const uint8_t* flag, int64_t np, int64_t nv, int64_t* faces, int64_t nf,
                    void* stream) {
    if (np < 0 || nv < 0 || nf < 0 || too_many(np) || too_many(nv) || too_many(nf)) return PPS_ERR_ARG;
    if (np == 0 || nf == 0) return PPS_OK;
    if (!fa || !fb || !quad || !flag || !faces) return PPS_ERR_ARG;
    hipLaunchKernelGGL(apply_kernel, dim3(grid_of(np, 256)), dim3(256), 0, (hipStream_t)stream, fa, fb, quad, flag, np, nv, faces, nf);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
