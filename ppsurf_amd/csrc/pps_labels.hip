// The compress step of the labelling layer for gfx950: one kernel and one entry for every stage that keeps int32 labels (the face
// components, the vertex clusters of the weld, the corner fans).  The argument is written out in pps_labels.h; the host loop that launches
// this between two hooks is ppsurf_amd/labels.py.
//
// new capability: replaces nothing in the reference.  Shape: one thread per node, a plain store into the thread's own slot, no atomics
// beyond the relaxed loads of the walk, no LDS.
#include "pps_common.h"
#include "pps_labels.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

__global__ __launch_bounds__(256) void compress_kernel(int32_t* label, int64_t n) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    if (load_label(label, x) < 0) return;                   // a node that takes no part is never touched
    label[x] = walk_end(label, (int)x);
}

}  // namespace

extern "C" {

int ppsx_labels_compress(int32_t* label, int64_t n, void* stream) {
    if (n < 0 || n > (int64_t)INT32_MAX) return PPS_ERR_ARG;
    if (n == 0) return PPS_OK;
    if (!label) return PPS_ERR_ARG;
    hipLaunchKernelGGL(compress_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, label, n);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
