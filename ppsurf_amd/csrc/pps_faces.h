// The face predicates of the mesh stages (pps_smooth.hip, pps_normals.hip, pps_trim.hip, pps_vis.hip) and the key that an invalid face gets.
//
// in range      the three indices lie in [0, nv): the face may be read through.
// valid face    in range and pairwise distinct: the face takes part in adjacency, incidence and normals.
// Restated in numpy by tests/topology_spec.py (`valid_faces`); the host side of the keys is ppsurf_amd/topology.py.
#pragma once
#include <stdint.h>

constexpr int64_t KEY_SENTINEL = INT64_MAX;                 // the keys of an invalid face: they sort last

__device__ __forceinline__ bool face_in_range(int64_t a, int64_t b, int64_t c, int64_t nv) {
    return a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv;
}

__device__ __forceinline__ bool face_valid(int64_t a, int64_t b, int64_t c, int64_t nv) {
    return face_in_range(a, b, c, nv) && a != b && b != c && c != a;
}
