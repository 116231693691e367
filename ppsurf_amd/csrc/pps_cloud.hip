// Preparation of raw scans for gfx950: voxel-grid subsampling and statistical outlier removal.
//
// new capability: the reference asks its users to sub-sample large clouds themselves (source/occupancy_data_module.py:183-184) and has no
// outlier filter.  Driven by ppsurf_amd/cloud.py; restated in numpy by tests/cloud_spec.py, which the kernels match bit for bit.
//
// Voxel grid (all in fp32, each operation rounded on its own, -ffp-contract=off):
//   cell    c_a = min(int(floorf((p_a - lo_a) * inv_h)), G_a - 1),  G_a = int(floorf((hi_a - lo_a) * inv_h)) + 1  (G_a <= 2^20)
//   key     (c_z * G_y + c_y) * G_x + c_x  in 64 bits
//   winner  of a cell: its point nearest to the centre lo_a + (float(c_a) + 0.5f) * h, d2 = (dx*dx + dy*dy) + dz*dz, ties to the lowest index.
//           d2 >= 0, so its bits order like its value: one 64-bit atomicMin of (d2 bits << 32 | index) per point (the rasteriser's pattern,
//           pps_vis.hip raster_faces_kernel).
// The cells live in an open-addressing table of 64-bit keys (capacity a power of two > n, insertion by atomicCAS, linear probing).  WHICH slot
// a key lands in depends on timing; the set of keys, the winner of every key and the ascending list of winners do not.  Integer atomics only.
// Thread t of the grid handles point t, so a wave reads 64 consecutive 12-byte rows, and the number of newly occupied cells is added to the
// counter once per wave (ballot + popcount), not once per lane.
//
// Outlier filter (the statistical filter of PCL / Open3D on the (k+1)-NN distances of ops.KnnBlocks):
//   m_i = (sum_{j=1..k} sqrt(double(d2[i, j]))) / k, in column order; column 0 is the point itself (or a duplicate of it)
//   mu = S1 / n, sigma = sqrt(S2 / n), S1 = sum m_i, S2 = sum (m_i - mu)^2: one workgroup, per-thread strided sums and a fixed LDS tree
//   (the shape of pps_eval.hip reduce_kernel), threshold = mu + ratio * sigma; a point is kept when m_i <= threshold.
#include "pps_common.h"
#include "../../include/ppsurf_amd.h"

namespace {

typedef unsigned long long u64;

constexpr u64 CLOUD_EMPTY = ~0ull;
constexpr int CLOUD_MAX_AXIS = 1 << 20;
constexpr int CLOUD_RED = 512;

struct Grid {
    float lo[3];
    int g[3];
    float h, inv_h;
};

// Not mix64 of pps_rng.h: a hash finaliser without the additive constant (0 maps to 0), and the voxel results do not depend on it.
__device__ __forceinline__ u64 cloud_mix64(u64 x) {          // splitmix64 finaliser: spreads the keys of neighbouring cells over the table
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ int cell_of(float p, float lo, float inv_h, int g) {
    const float t = floorf((p - lo) * inv_h);
    // the same value as min(int(t), g - 1) for every finite p >= lo; a NaN or a point below lo (excluded by the caller) goes to cell 0
    return t >= (float)(g - 1) ? g - 1 : (t > 0.f ? (int)t : 0);
}

// One thread per point: find or insert the point's cell.  SELECT also competes for the cell with (d2 bits << 32 | index).
template <bool SELECT>
__global__ __launch_bounds__(256) void voxel_insert_kernel(const float* __restrict__ pts, int64_t n, Grid grid, u64* __restrict__ table,
                                                           u64* __restrict__ best, u64 mask, u64* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const int cx = cell_of(x, grid.lo[0], grid.inv_h, grid.g[0]);
        const int cy = cell_of(y, grid.lo[1], grid.inv_h, grid.g[1]);
        const int cz = cell_of(z, grid.lo[2], grid.inv_h, grid.g[2]);
        const u64 key = ((u64)cz * (u64)grid.g[1] + (u64)cy) * (u64)grid.g[0] + (u64)cx;
        u64 slot = cloud_mix64(key) & mask;
        // capacity > n >= number of distinct keys: an empty slot always exists, the probe ends
        while (true) {
            const u64 seen = atomicCAS(table + slot, CLOUD_EMPTY, key);
            if (seen == CLOUD_EMPTY) { fresh = true; break; }
            if (seen == key) break;
            slot = (slot + 1) & mask;
        }
        if (SELECT) {
            const float dx = x - (grid.lo[0] + ((float)cx + 0.5f) * grid.h);
            const float dy = y - (grid.lo[1] + ((float)cy + 0.5f) * grid.h);
            const float dz = z - (grid.lo[2] + ((float)cz + 0.5f) * grid.h);
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            atomicMin(best + slot, ((u64)__float_as_uint(d2) << 32) | (u64)(uint32_t)i);
        }
    }
    const u64 ballot = __ballot(fresh);
    if ((threadIdx.x & 63) == 0 && ballot != 0) atomicAdd(count, (u64)__popcll(ballot));
}

// keep[winner of every occupied slot] = 1
__global__ __launch_bounds__(256) void voxel_mark_kernel(const u64* __restrict__ table, const u64* __restrict__ best, int64_t capacity, int64_t n,
                                                         uint8_t* __restrict__ keep) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= capacity || table[s] == CLOUD_EMPTY) return;
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

// host side of the grid rule; false when an argument is out of range (nothing may be launched then)
bool make_grid(const float* lo, const float* hi, float h, float inv_h, Grid* grid) {
    if (!lo || !hi || !(h > 0.f) || !(inv_h > 0.f) || !(h <= 3.0e38f) || !(inv_h <= 3.0e38f)) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(hi[a] >= lo[a]) || !(hi[a] - lo[a] <= 3.0e38f)) return false;
        const float t = floorf((hi[a] - lo[a]) * inv_h);
        if (!(t < (float)CLOUD_MAX_AXIS)) return false;            // more than 2^20 cells along an axis: an error, not a truncation
        grid->lo[a] = lo[a];
        grid->g[a] = (int)t + 1;
    }
    grid->h = h;
    grid->inv_h = inv_h;
    return true;
}

bool table_ok(int64_t n, int64_t capacity) {
    return n >= 1 && n <= INT32_MAX && capacity > n && capacity <= ((int64_t)1 << 34) && (capacity & (capacity - 1)) == 0;
}

}  // namespace

extern "C" {

int64_t pps_cloud_table_capacity(int64_t n) {
    if (n < 1) return -1;
    int64_t c = 64;
    while (c < 2 * n) c <<= 1;
    return c;
}

int pps_cloud_voxel_count(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, uint64_t* table, int64_t capacity,
                          uint64_t* count, void* stream) {
    Grid grid;
    if (!pts || !table || !count || !table_ok(n, capacity) || !make_grid(lo, hi, h, inv_h, &grid)) return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0xFF, (size_t)capacity * 8, st) != hipSuccess || hipMemsetAsync(count, 0, 8, st) != hipSuccess) return PPS_ERR_LAUNCH;
    hipLaunchKernelGGL(voxel_insert_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, grid, (u64*)table, (u64*)nullptr,
                       (u64)(capacity - 1), (u64*)count);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_cloud_voxel_select(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, uint64_t* table, uint64_t* best,
                           int64_t capacity, uint64_t* count, uint8_t* keep, void* stream) {
    Grid grid;
    if (!pts || !table || !best || !count || !keep || !table_ok(n, capacity) || !make_grid(lo, hi, h, inv_h, &grid)) return PPS_ERR_ARG;
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
