/*
 * ppsurf_amd -- extension entries of the C ABI: everything added after ABI version 2.
 *
 * include/ppsurf_amd.h is frozen at ABI version 2 (pps_abi_version() stays 2, its `pps_` entries stay as they are).  New entry points are
 * declared here, carry the prefix `ppsx_` and live in the same shared library.  The conventions are those of the main header: every data
 * pointer is a DEVICE pointer owned by the caller, row-major; `stream` is a hipStream_t (NULL = default stream) and launches are
 * asynchronous; the return value is 0 ok, 1 bad argument, 2 launch failure; nothing is allocated inside.  ppsurf_amd/_lib.py parses this
 * file into EXT_SIGNATURES and `call` dispatches a `ppsx_` name like a `pps_` one.
 */
#ifndef PPSURF_AMD_EXT_H
#define PPSURF_AMD_EXT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- colour transfer from a scan to a mesh (csrc/pps_transfer.hip) --------------------------------------------------------------------------
 * new capability: replaces nothing -- the reference writes uncoloured meshes (source/poco_model.py:269 `mesh.export`).  Driven by
 * ppsurf_amd/transfer.py; the rule is written out at the top of csrc/pps_transfer.hip and in DESIGN.md section 14.
 *   ppsx_blend_rgba_u8  out u8 [m,4]: the inverse-squared-distance blend of the colours rgba u8 [n,4] of the k neighbours idx int64 [m,k] with
 *                       squared distances d2 f32 [m,k] (ops.KnnBlocks.query(..., return_d2=True)).  Per row, in fp64, j = 0..k-1 in column order,
 *                       every operation rounded on its own (no fused multiply-add): a neighbour counts when 0 <= idx[i,j] < n;
 *                       w = 1 / (double(d2[i,j]) + eps); S += w; T[c] += w * double(rgba[idx[i,j], c]).  S == 0 (no valid neighbour):
 *                       out[i,:] = 0; otherwise out[i,c] = u8(min(255, max(0, floor(T[c] / S + 0.5)))).  A pure function of its inputs: one
 *                       thread per row, no atomics.  rgba and out must be 4-byte aligned (each row moves as one dword).
 *                       m < 0, n < 0, k outside 1..256, eps not > 0, or, with m > 0, a NULL pointer or a misaligned rgba / out:
 *                       PPS_ERR_ARG, nothing is launched or written.  m == 0: 0, nothing is launched.  Indices outside [0, n) are skipped,
 *                       never read through. */
int ppsx_blend_rgba_u8(const int64_t* idx, const float* d2, int64_t m, int k, const uint8_t* rgba, int64_t n, double eps, uint8_t* out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPSURF_AMD_EXT_H */
