// The cell grid and its table, shared by the voxel stage of raw scans (pps_cloud.hip, T = float), the vertex clustering of meshes
// (pps_simplify.hip, T = double) and the cell lists of the trim and the weld (pps_trim.hip, pps_weld.hip, T = float; find_run);
// DESIGN.md section 12.  Restated in numpy by tests/grid_spec.py.
//
// Grid over the box lo..hi with step h (h and inv_h = 1 / h come from the host), every operation in T and rounded on its own
// (-ffp-contract=off):
//   dims    G_a = int(floor((hi_a - lo_a) * inv_h)) + 1; more than 2^20 cells along an axis is an error, not a truncation
//   cell    c_a = min(int(floor((p_a - lo_a) * inv_h)), G_a - 1): a point on a wall belongs to the cell above it, the points at hi_a may get
//           a layer of their own
//   key     (c_z * G_y + c_y) * G_x + c_x  in 64 bits
// The occupied cells live in an open-addressing table of 64-bit keys: capacity a power of two > n (by default >= 2 n), EMPTY = all ones,
// slot = finaliser(key) & mask, insertion by atomicCAS, linear probing.  WHICH slot a key lands in depends on timing; the set of keys, and
// any integer minimum a caller keeps per slot, do not.  Newly occupied cells are counted once per wave (ballot + popcount), not once per lane.
#pragma once
#include "pps_common.h"

namespace cells {

typedef unsigned long long u64;

constexpr u64 EMPTY = ~0ull;
constexpr int MAX_AXIS = 1 << 20;

template <typename T>
struct Grid {
    T lo[3];
    int g[3];
    T h, inv_h;
};

__host__ __device__ inline float floor_of(float t) { return floorf(t); }
__host__ __device__ inline double floor_of(double t) { return floor(t); }
constexpr float limit_of(float) { return 3.0e38f; }          // the largest extent, step and 1 / step that a grid takes
constexpr double limit_of(double) { return 1.0e300; }

template <typename T>
__device__ __forceinline__ int cell_of(T p, T lo, T inv_h, int g) {
    const T t = floor_of((p - lo) * inv_h);
    // the same value as min(int(t), g - 1) for every finite p >= lo; a NaN or a point below lo (excluded by the callers) goes to cell 0
    return t >= (T)(g - 1) ? g - 1 : (t > (T)0 ? (int)t : 0);
}

template <typename T>
__device__ __forceinline__ u64 key_of(const Grid<T>& grid, int cx, int cy, int cz) {
    return ((u64)cz * (u64)grid.g[1] + (u64)cy) * (u64)grid.g[0] + (u64)cx;
}

// Not mix64 of pps_rng.h: a hash finaliser without the additive constant (0 maps to 0), and no result depends on it.
__device__ __forceinline__ u64 mix64(u64 x) {                // splitmix64 finaliser: spreads the keys of neighbouring cells over the table
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The slot of `key`, inserted if absent; fresh = this thread occupied the slot.  capacity > n >= number of distinct keys: an empty slot
// always exists, the probe ends.
__device__ __forceinline__ u64 find_or_insert(u64* __restrict__ table, u64 mask, u64 key, bool& fresh) {
    u64 slot = mix64(key) & mask;
    while (true) {
        const u64 seen = atomicCAS(table + slot, EMPTY, key);
        if (seen == EMPTY) { fresh = true; break; }
        if (seen == key) break;
        slot = (slot + 1) & mask;
    }
    return slot;
}

// Read-only: the run [j, jend) of the caller's `order` that lists the points of the cell `key`, from offsets int64 [capacity + 1] over a
// table of n points.  The probe ends at the key or at an empty slot, after at most capacity tries; j and jend are left as they are when
// the cell is not in the table or its offsets are not 0 <= o0 <= o1 <= n.
__device__ __forceinline__ void find_run(const u64* __restrict__ table, u64 mask, u64 key, const int64_t* __restrict__ offsets, int64_t n,
                                         int64_t& j, int64_t& jend) {
    u64 s = mix64(key) & mask;
    for (u64 tries = 0; tries <= mask; ++tries) {
        const u64 seen = table[s];
        if (seen == key) {
            const int64_t o0 = offsets[s], o1 = offsets[s + 1];
            if (o0 >= 0 && o0 <= o1 && o1 <= n) { j = o0; jend = o1; }
            return;
        }
        if (seen == EMPTY) return;
        s = (s + 1) & mask;
    }
}

// count += number of lanes of this wave with `flag`; every lane of the wave must call it
__device__ __forceinline__ void wave_count(u64* __restrict__ count, bool flag) {
    const u64 ballot = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && ballot != 0) atomicAdd(count, (u64)__popcll(ballot));
}

// host side of the grid rule; false when an argument is out of range (nothing may be launched then)
template <typename T>
inline bool make_grid(const T* lo, const T* hi, T h, T inv_h, Grid<T>* grid) {
    const T big = limit_of(T());
    if (!lo || !hi || !(h > (T)0) || !(inv_h > (T)0) || !(h <= big) || !(inv_h <= big)) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(hi[a] >= lo[a]) || !(hi[a] - lo[a] <= big)) return false;
        const T t = floor_of((hi[a] - lo[a]) * inv_h);
        if (!(t < (T)MAX_AXIS)) return false;
        grid->lo[a] = lo[a];
        grid->g[a] = (int)t + 1;
    }
    grid->h = h;
    grid->inv_h = inv_h;
    return true;
}

inline bool table_ok(int64_t n, int64_t capacity) {
    return n >= 1 && n <= INT32_MAX && capacity > n && capacity <= ((int64_t)1 << 34) && (capacity & (capacity - 1)) == 0;
}

// the default capacity: the power of two >= 2 n (load <= 0.5), at least 64; -1 for n < 1
inline int64_t table_capacity(int64_t n) {
    if (n < 1) return -1;
    int64_t c = 64;
    while (c < 2 * n) c <<= 1;
    return c;
}

}  // namespace cells
