// Counter-based generator of the surface sampler (pps_eval.hip), the scanner noise and the query points (pps_scan.hip); restated in numpy by
// tests/eval_spec.py and tests/scan_spec.py (keep them in step):
//     mix(x)    = splitmix64 finaliser of x + 0x9E3779B97F4A7C15:
//                   z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//                   return z ^ (z >> 31)                                                       (all uint64, wrapping)
//     key       = mix(mix(seed) ^ stream_id)
//     bits(c)   = mix(key ^ c)                                 counter c = (item index << 2) | draw, draw in {0, 1, 2}
//     unit53    = (bits >> 11) * 2^-53                         fp64 in [0, 1);  unit53_pos = ((bits >> 11) + 1) * 2^-53 in (0, 1]
//     unit24    = (bits >> 40) * 2^-24                         fp32 in [0, 1), exact
// A draw depends on (seed, stream_id, c) only.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint64_t rng_key(uint64_t seed, uint64_t stream_id) { return mix64(mix64(seed) ^ stream_id); }
__device__ __forceinline__ uint64_t rng_bits(uint64_t key, uint64_t ctr) { return mix64(key ^ ctr); }
__device__ __forceinline__ double unit53(uint64_t bits) { return (double)(bits >> 11) * 0x1.0p-53; }
__device__ __forceinline__ double unit53_pos(uint64_t bits) { return (double)((bits >> 11) + 1) * 0x1.0p-53; }
__device__ __forceinline__ float unit24(uint64_t bits) { return (float)(uint32_t)(bits >> 40) * 0x1.0p-24f; }
