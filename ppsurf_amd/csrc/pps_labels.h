// The walk over int32 labels that the hooking and compressing stages share: the face components (pps_pieces.hip), the
// vertex clusters of the weld (pps_weld.hip, section 24) and the corner fans (pps_manifold.hip, section 25).  pps_orient.hip walks 64-bit
// words that carry a parity and keeps its own.
//
// label[x] <= x for every slot that takes part and labels only fall, so a walk descends and ends.  Every label is read by ONE relaxed
// device-scope atomic load: the range check and the use see the same value, and the value is the one the slot has or an earlier one -- the
// L2s of the XCDs are not coherent for plain loads, and no kernel relies on seeing another workgroup's write inside its launch (the
// argument is written out at the top of pps_pieces.hip).
#pragma once
#include <stdint.h>

__device__ __forceinline__ int load_label(const int32_t* label, int64_t x) {
    return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the end of the walk from x (0 <= x < n, by the caller): it steps to label[x] while 0 <= label[x] < x
__device__ __forceinline__ int walk_end(const int32_t* label, int x) {
    for (;;) {
        const int p = load_label(label, x);
        if (p < 0 || p >= x) return x;
        x = p;
    }
}
