// The sliced face sweep: the brute-force query of m items (points, rays) against a triangle soup corners f32 [nf,9] (pps_eval_face_stats),
// shared by the winding number (pps_eval.hip), the closest point (pps_vis.hip) and the first hit (pps_scan.hip).
//
// Pass 1, sweep_kernel<Op>: workgroup (item block, face slice) visits the faces of its slice in face order for SWEEP_TILE items, SWEEP_IPL per
// lane in registers.  The face index is wave-uniform, so the nine corner floats of a face are scalar loads shared by the wave.  Every
// (slice, item) writes one partial at index slice * m + item; no atomics.  Pass 2, a small kernel of each caller's own, combines the
// partials of an item in slice order.
//
// An operation Op is a struct of device pointers with
//     struct Item;                                                   per-item register state
//     Item load(int64_t i) const;                                    the state of item i before the first face
//     void face(const float* c, int32_t f, Item (&it)[SWEEP_IPL]) const;   face f (corners c[0..8]) for the lane's whole tile
//     void store(const Item& it, int64_t k) const;                   the partial of one item at index k = slice * m + item
// face() gets the tile, not one item, so that an operation can hoist work that depends on the face alone.  f is the face id as the
// partials store it (int32_t: with an int64_t id the closest-point sweep allocated its registers measurably worse).
#pragma once
#include "pps_common.h"

constexpr int SWEEP_BLOCK = 256;
constexpr int SWEEP_IPL = 4;                                  // items per lane, held in registers
constexpr int SWEEP_TILE = SWEEP_BLOCK * SWEEP_IPL;           // items per workgroup
constexpr int64_t SWEEP_TARGET_BLOCKS = 16384;                // ~10 rounds of 256 CUs x 6 resident workgroups: a short tail
constexpr int64_t SWEEP_MIN_SLICE = 64;                       // faces per slice, at least

// Number of face slices for m items and nf faces (-1 for an empty problem): enough workgroups to fill the device, no empty slice.
// At most SWEEP_TARGET_BLOCKS, so it always fits gridDim.y.
inline int64_t sweep_slices(int64_t m, int64_t nf) {
    if (m < 1 || nf < 1) return -1;
    const int64_t blocks = (m + SWEEP_TILE - 1) / SWEEP_TILE;
    int64_t s = (SWEEP_TARGET_BLOCKS + blocks - 1) / blocks;
    const int64_t smax = (nf + SWEEP_MIN_SLICE - 1) / SWEEP_MIN_SLICE;
    s = s < smax ? s : smax;
    const int64_t per = (nf + s - 1) / s;                     // no empty slice
    return (nf + per - 1) / per;
}

template <typename Op>
__global__ __launch_bounds__(SWEEP_BLOCK) void sweep_kernel(const float* __restrict__ corners, int64_t nf, int64_t m, int64_t per_slice, Op op) {
    const int64_t i0 = (int64_t)blockIdx.x * SWEEP_TILE + threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.y * per_slice;
    const int64_t f1 = f0 + per_slice < nf ? f0 + per_slice : nf;
    typename Op::Item it[SWEEP_IPL];
#pragma unroll
    for (int j = 0; j < SWEEP_IPL; ++j) {
        const int64_t i = i0 + (int64_t)j * SWEEP_BLOCK;
        it[j] = op.load(i < m ? i : m - 1);                   // the tail repeats the last item and stores nothing
    }
    for (int64_t f = f0; f < f1; ++f) op.face(corners + 9 * f, (int32_t)f, it);
#pragma unroll
    for (int j = 0; j < SWEEP_IPL; ++j) {
        const int64_t i = i0 + (int64_t)j * SWEEP_BLOCK;
        if (i < m) op.store(it[j], (int64_t)blockIdx.y * m + i);
    }
}

// Launches pass 1 with `slices` face slices, 1 <= slices <= min(nf, 65535); any such count is valid.  Returns the number of slices that
// hold a face (the rows of the partials that are written, what pass 2 reads), or 0 when the launch shape is out of range.
template <typename Op>
inline int64_t sweep_launch(const float* corners, int64_t nf, int64_t m, int64_t slices, Op op, hipStream_t st) {
    const int64_t blocks = (m + SWEEP_TILE - 1) / SWEEP_TILE;
    if (slices < 1 || slices > 65535 || slices > nf || blocks > INT32_MAX) return 0;
    const int64_t per = (nf + slices - 1) / slices;
    const int64_t used = (nf + per - 1) / per;
    hipLaunchKernelGGL(sweep_kernel<Op>, dim3((unsigned)blocks, (unsigned)used), dim3(SWEEP_BLOCK), 0, st, corners, nf, m, per, op);
    return used;
}
