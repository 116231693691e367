// Preparation of raw scans for gfx950: voxel-grid subsampling and statistical outlier removal.
//
// new capability: the reference asks its users to sub-sample large clouds themselves (source/occupancy_data_module.py:183-184) and has no
// outlier filter.  Driven by ppsurf_amd/cloud.py; restated in numpy by tests/cloud_spec.py, which the kernels match bit for bit.
//
// Voxel stage: the cell grid and table of pps_cells.h in fp32.  Thread t of the launch handles point t, so a wave reads 64 consecutive
// 12-byte rows.
//   winner  of a cell: its point nearest to the centre lo_a + (float(c_a) + 0.5f) * h, d2 = (dx*dx + dy*dy) + dz*dz, ties to the lowest index.
//           d2 >= 0, so its bits order like its value: one 64-bit atomicMin of (d2 bits << 32 | index) per point (the rasteriser's pattern,
//           pps_vis.hip raster_faces_kernel).  The winner of every key and the ascending list of winners do not depend on timing.
//           Integer atomics only.
//
// Outlier filter (the statistical filter of PCL / Open3D on the (k+1)-NN distances of ops.KnnBlocks):
//   m_i = (sum_{j=1..k} sqrt(double(d2[i, j]))) / k, in column order; column 0 is the point itself (or a duplicate of it)
//   mu = S1 / n, sigma = sqrt(S2 / n), S1 = sum m_i, S2 = sum (m_i - mu)^2: one workgroup, per-thread strided sums and a fixed LDS tree
//   (the shape of pps_eval.hip reduce_kernel), threshold = mu + ratio * sigma; a point is kept when m_i <= threshold.
#include "pps_cells.h"
#include "../../include/ppsurf_amd.h"

namespace {

using cells::u64;
typedef cells::Grid<float> Grid;

constexpr int CLOUD_RED = 512;

// One thread per point: find or insert the point's cell.  SELECT also competes for the cell with (d2 bits << 32 | index).
template <bool SELECT>
__global__ __launch_bounds__(256) void voxel_insert_kernel(const float* __restrict__ pts, int64_t n, Grid grid, u64* __restrict__ table,
                                                           u64* __restrict__ best, u64 mask, u64* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const int cx = cells::cell_of(x, grid.lo[0], grid.inv_h, grid.g[0]);
        const int cy = cells::cell_of(y, grid.lo[1], grid.inv_h, grid.g[1]);
        const int cz = cells::cell_of(z, grid.lo[2], grid.inv_h, grid.g[2]);
        const u64 slot = cells::find_or_insert(table, mask, cells::key_of(grid, cx, cy, cz), fresh);
        if (SELECT) {
            const float dx = x - (grid.lo[0] + ((float)cx + 0.5f) * grid.h);
            const float dy = y - (grid.lo[1] + ((float)cy + 0.5f) * grid.h);
            const float dz = z - (grid.lo[2] + ((float)cz + 0.5f) * grid.h);
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            atomicMin(best + slot, ((u64)__float_as_uint(d2) << 32) | (u64)(uint32_t)i);
        }
    }
    cells::wave_count(count, fresh);
}

// keep[winner of every occupied slot] = 1
__global__ __launch_bounds__(256) void voxel_mark_kernel(const u64* __restrict__ table, const u64* __restrict__ best, int64_t capacity, int64_t n,
                                                         uint8_t* __restrict__ keep) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= capacity || table[s] == cells::EMPTY) return;
    const int64_t i = (int64_t)(best[s] & 0xFFFFFFFFull);
    if (i < n) keep[i] = 1;
}

__global__ __launch_bounds__(256) void mean_dist_kernel(const float* __restrict__ d2, int64_t n, int k, double* __restrict__ m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* row = d2 + i * (int64_t)(k + 1);
    double s = 0.0;
    for (int j = 1; j <= k; ++j) s += sqrt((double)row[j]);
    m[i] = s / (double)k;
}

__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int h = CLOUD_RED / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// out[0] = mu, out[1] = sigma (population), out[2] = mu + ratio * sigma.  One workgroup, fixed order: bitwise reproducible.
__global__ __launch_bounds__(CLOUD_RED) void mean_std_kernel(const double* __restrict__ m, int64_t n, double ratio, double* __restrict__ out) {
    __shared__ double red[CLOUD_RED];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int64_t i = tid; i < n; i += CLOUD_RED) v += m[i];
    const double mu = block_sum(v, red, tid) / (double)n;
    v = 0.0;
    for (int64_t i = tid; i < n; i += CLOUD_RED) {
        const double d = m[i] - mu;
        v += d * d;
    }
    const double sigma = sqrt(block_sum(v, red, tid) / (double)n);
    if (tid == 0) {
        out[0] = mu;
        out[1] = sigma;
        out[2] = mu + ratio * sigma;
    }
}

__global__ __launch_bounds__(256) void outlier_keep_kernel(const double* __restrict__ m, int64_t n, const double* __restrict__ stats,
                                                           uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = m[i] <= stats[2] ? 1 : 0;
}

}  // namespace

extern "C" {

int64_t pps_cloud_table_capacity(int64_t n) {
    return cells::table_capacity(n);
}

int pps_cloud_voxel_count(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, uint64_t* table, int64_t capacity,
                          uint64_t* count, void* stream) {
    Grid grid;
    if (!pts || !table || !count || !cells::table_ok(n, capacity) || !cells::make_grid(lo, hi, h, inv_h, &grid)) return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0xFF, (size_t)capacity * 8, st) != hipSuccess || hipMemsetAsync(count, 0, 8, st) != hipSuccess) return PPS_ERR_LAUNCH;
    hipLaunchKernelGGL(voxel_insert_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, grid, (u64*)table, (u64*)nullptr,
                       (u64)(capacity - 1), (u64*)count);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_cloud_voxel_select(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, uint64_t* table, uint64_t* best,
                           int64_t capacity, uint64_t* count, uint8_t* keep, void* stream) {
    Grid grid;
    if (!pts || !table || !best || !count || !keep || !cells::table_ok(n, capacity) || !cells::make_grid(lo, hi, h, inv_h, &grid))
        return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0xFF, (size_t)capacity * 8, st) != hipSuccess || hipMemsetAsync(best, 0xFF, (size_t)capacity * 8, st) != hipSuccess ||
        hipMemsetAsync(count, 0, 8, st) != hipSuccess || hipMemsetAsync(keep, 0, (size_t)n, st) != hipSuccess)
        return PPS_ERR_LAUNCH;
    hipLaunchKernelGGL(voxel_insert_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, grid, (u64*)table, (u64*)best,
                       (u64)(capacity - 1), (u64*)count);
    hipLaunchKernelGGL(voxel_mark_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, st, (const u64*)table, (const u64*)best, capacity, n,
                       keep);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_cloud_mean_knn_dist(const float* d2, int64_t n, int k, double* m, void* stream) {
    if (n < 0 || k < 1) return PPS_ERR_ARG;
    if (n == 0) return PPS_OK;
    if (!d2 || !m) return PPS_ERR_ARG;
    hipLaunchKernelGGL(mean_dist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d2, n, k, m);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_cloud_outlier_stats(const double* m, int64_t n, double ratio, double* out, void* stream) {
    if (n < 1 || !m || !out || !(ratio == ratio)) return PPS_ERR_ARG;
    hipLaunchKernelGGL(mean_std_kernel, dim3(1), dim3(CLOUD_RED), 0, (hipStream_t)stream, m, n, ratio, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_cloud_outlier_keep(const double* m, int64_t n, const double* stats, uint8_t* keep, void* stream) {
    if (n < 0) return PPS_ERR_ARG;
    if (n == 0) return PPS_OK;
    if (!m || !stats || !keep) return PPS_ERR_ARG;
    hipLaunchKernelGGL(outlier_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, n, stats, keep);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
