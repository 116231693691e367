// Qualitative comparison of reconstructions (source/make_comparison.py): the exact closest point of query points on a triangle mesh, which
// colours a reconstruction by its distance to the ground truth, and a deterministic z-buffer rasteriser for meshes and point clouds.
//
// Closest point -- replaces source/base/proximity.py:20-36 (trimesh.proximity.closest_point in batches of 1000 on the CPU), called from
// source/base/visualization.py:91-93.  Point-triangle closest point by Voronoi-region classification (Ericson, Real-Time Collision
// Detection, 5.1.5; in pps_tri.h).  A face with |e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2 (zero or next to zero area) is its longest edge.  Pass 1 picks, per
// query and face slice, the smallest squared distance, ties to the lowest face: in fp32 (the interior region measured as the plane
// distance (ap.n)^2 / n.n), or in fp64 for a thin face (height below 0.1 x its longest edge), whose fp32 region tests are unreliable.
// Pass 2 takes the minimum over the slices in slice order (ties to the lower face again) and recomputes distance and closest point of
// the winning face in fp64.  The result depends on (corners, query) only, not on the slice count.  Pass 1 is an operation of the sliced
// face sweep of pps_sweep.h; corners is the face table of pps_eval_face_stats.
//
// Rasteriser -- replaces the pyrender / pyglet renders of source/base/visualization.py:25-63, 122-134.  Camera (host array of 16 floats):
// M = cam[0..8] (world -> view rotation, row-major), eye = cam[9..11], f = cam[12] (focal length in pixels); cam[13..15] unused.  Per
// vertex, fp32 without contraction, in this order:
//     d = v - eye;  xc = (M00 dx + M01 dy) + M02 dz  (yc, zc alike);  depth = -zc
//     sx = 0.5 W + (f xc) / depth;  sy = 0.5 H - (f yc) / depth                       (pixel (x, y) has its centre at (x + 0.5, y + 0.5))
// A triangle with a vertex of depth < near (0.01), or of zero screen area, is dropped; no back-face culling.  Coverage in fp64 on the
// fp32 screen coordinates, oriented so that the screen area is positive:
//     edge(a, b, p) = (bx - ax)(py - ay) - (by - ay)(px - ax);  E0 = edge(P1, P2, p), E1 = edge(P2, P0, p), E2 = edge(P0, P1, p)
//     covered iff every Ei > 0, or Ei == 0 on an owned edge a -> b: (by - ay) < 0, or (by - ay) == 0 and (bx - ax) > 0 (top-left rule)
//     view depth = 1 / sum_i (Ei / area) / depth_i                                     (fp64, then fp32)
// key = (float bits of the view depth << 32) | id, a 64-bit atomicMin into keys [H,W] (initialised to all ones): bitwise reproducible.
// The pixels of every triangle's bounding box are spread over the threads by an inclusive prefix of the box sizes and a binary search
// in it, so one screen-filling triangle does not serialise onto one thread.  Points are discs of radius r px: pixel centre within r of
// (sx, sy) (fp64), depth of the point.  Shading: colour (vertex colours interpolated with the perspective-correct barycentrics, or a
// uniform colour) times 0.3 + 0.7 |n . v|, n the unit face normal, v the unit vector from the surface point to the eye; points are
// unshaded; background white; channel = min(255, (int)(c + 0.5)).
#include <math.h>

#include "pps_common.h"
#include "pps_faces.h"
#include "pps_sweep.h"
#include "pps_tri.h"
#include "../../include/ppsurf_amd.h"

namespace {

constexpr float NEAR = 0.01f;
constexpr float SLIVER = 0.01f;                               // |e1 x e2|^2 < SLIVER lmax^4 (height < 0.1 x longest edge): pass 1 in fp64

// Pass 1 (pps_sweep.h): the smallest squared distance of every query over the faces of its slice.  Strict < keeps the lowest face of equal
// distance; face -1 means no finite distance in the slice.  The face is classified once for the lane's whole tile.  The running minimum
// is two selects, not a branch: the branch costs three more VGPRs.
struct ClosestOp {
    const float* __restrict__ query;
    float* __restrict__ part_d2;
    int32_t* __restrict__ part_face;
    struct Item {
        V3<float> p;
        float best;
        int32_t bf;
    };
    __device__ __forceinline__ Item load(int64_t q) const { return {{query[3 * q], query[3 * q + 1], query[3 * q + 2]}, INFINITY, -1}; }
    __device__ __forceinline__ void face(const float* __restrict__ c, int32_t f, Item (&it)[SWEEP_IPL]) const {
        const V3<float> a = {c[0], c[1], c[2]}, b = {c[3], c[4], c[5]}, cc = {c[6], c[7], c[8]};
        const V3<float> ab = sub(b, a), ac = sub(cc, a), bc = sub(cc, b), n = cross(ab, ac);
        const float lmax = fmaxf(dot(ab, ab), fmaxf(dot(ac, ac), dot(bc, bc)));
        if (dot(n, n) < SLIVER * (lmax * lmax)) {             // thin face (face-uniform branch): fp32 misclassifies the regions
            const V3<double> a64 = {a.x, a.y, a.z}, b64 = {b.x, b.y, b.z}, c64 = {cc.x, cc.y, cc.z};
#pragma unroll
            for (int j = 0; j < SWEEP_IPL; ++j) {
                double s, t, d2;
                closest_on_triangle<double>(V3<double>{it[j].p.x, it[j].p.y, it[j].p.z}, a64, b64, c64, s, t, d2);
                const float d2f = (float)d2;
                const bool lt = d2f < it[j].best;
                it[j].best = lt ? d2f : it[j].best;
                it[j].bf = lt ? f : it[j].bf;
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < SWEEP_IPL; ++j) {
            float s, t, d2;
            closest_on_triangle<float>(it[j].p, a, b, cc, s, t, d2);
            const bool lt = d2 < it[j].best;
            it[j].best = lt ? d2 : it[j].best;
            it[j].bf = lt ? f : it[j].bf;
        }
    }
    __device__ __forceinline__ void store(const Item& it, int64_t k) const {
        part_d2[k] = it.best;
        part_face[k] = it.bf;
    }
};

// Pass 2: minimum over the slices in slice order (strict <: ties to the lower slice, i.e. the lower face), then distance and closest
// point of the winning face in fp64.  A query whose every distance is NaN gets face 0.
__global__ __launch_bounds__(256) void closest_final_kernel(const float* __restrict__ corners, const float* __restrict__ query, int64_t m,
                                                            int64_t slices, const float* __restrict__ part_d2, const int32_t* __restrict__ part_face,
                                                            float* __restrict__ out_d, int32_t* __restrict__ out_face, float* __restrict__ out_pt) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    float best = INFINITY;
    int32_t f = -1;
    for (int64_t k = 0; k < slices; ++k) {
        const float d2 = part_d2[k * m + q];
        const int32_t fk = part_face[k * m + q];             // -1: no finite distance in slice k
        if (fk >= 0 && (f < 0 || d2 < best)) {
            best = d2;
            f = fk;
        }
    }
    f = f < 0 ? 0 : f;
    const float* c = corners + 9 * (int64_t)f;
    const V3<double> p = {(double)query[3 * q], (double)query[3 * q + 1], (double)query[3 * q + 2]};
    const V3<double> a = {(double)c[0], (double)c[1], (double)c[2]}, b = {(double)c[3], (double)c[4], (double)c[5]};
    const V3<double> cc = {(double)c[6], (double)c[7], (double)c[8]};
    double s, t, d2;
    closest_on_triangle<double>(p, a, b, cc, s, t, d2);
    const V3<double> ab = sub(b, a), ac = sub(cc, a);
    const V3<double> x = {(a.x + s * ab.x) + t * ac.x, (a.y + s * ab.y) + t * ac.y, (a.z + s * ab.z) + t * ac.z};
    const V3<double> dx = sub(p, x);
    out_d[q] = (float)sqrt(dot(dx, dx));
    out_face[q] = f;
    out_pt[3 * q] = (float)x.x;
    out_pt[3 * q + 1] = (float)x.y;
    out_pt[3 * q + 2] = (float)x.z;
}

// ---- rasteriser -----------------------------------------------------------------------------------------------------------------------------------
struct Cam {
    float m[9], eye[3], f, hw, hh;
};

__host__ __device__ __forceinline__ void project(const Cam& c, float vx, float vy, float vz, float& sx, float& sy, float& depth) {
    const float dx = vx - c.eye[0], dy = vy - c.eye[1], dz = vz - c.eye[2];
    const float xc = (c.m[0] * dx + c.m[1] * dy) + c.m[2] * dz;
    const float yc = (c.m[3] * dx + c.m[4] * dy) + c.m[5] * dz;
    const float zc = (c.m[6] * dx + c.m[7] * dy) + c.m[8] * dz;
    depth = -zc;
    sx = c.hw + (c.f * xc) / depth;
    sy = c.hh - (c.f * yc) / depth;
}

__device__ __forceinline__ double edge_fn(double ax, double ay, double bx, double by, double px, double py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

__device__ __forceinline__ bool owned(double ax, double ay, double bx, double by) {
    const double dy = by - ay;
    return dy < 0.0 || (dy == 0.0 && bx - ax > 0.0);
}

__global__ __launch_bounds__(256) void project_kernel(const float* __restrict__ verts, int64_t nv, Cam cam, float* __restrict__ proj) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    float sx, sy, z;
    project(cam, verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], sx, sy, z);
    proj[3 * i] = sx;
    proj[3 * i + 1] = sy;
    proj[3 * i + 2] = z;
}

// Per face: oriented screen corners and depths {x0 y0 x1 y1} {x2 y2 z0 z1} {z2 bx by bw} (bx, by, bw as int bits) and the pixel count of
// the clamped bounding box of the covered pixel centres (0 for a dropped face) into cnt.
__global__ __launch_bounds__(256) void face_setup_kernel(const int32_t* __restrict__ faces, int64_t nf, int64_t nv, const float* __restrict__ proj,
                                                         int width, int height, float4* __restrict__ rec, int64_t* __restrict__ cnt) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    int64_t count = 0;
    float4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0}, r2 = {0, 0, 0, 0};
    if (face_in_range(i0, i1, i2, nv)) {
        float x0 = proj[3 * (int64_t)i0], y0 = proj[3 * (int64_t)i0 + 1], z0 = proj[3 * (int64_t)i0 + 2];
        float x1 = proj[3 * (int64_t)i1], y1 = proj[3 * (int64_t)i1 + 1], z1 = proj[3 * (int64_t)i1 + 2];
        float x2 = proj[3 * (int64_t)i2], y2 = proj[3 * (int64_t)i2 + 1], z2 = proj[3 * (int64_t)i2 + 2];
        const double area = edge_fn(x0, y0, x1, y1, x2, y2);
        if (z0 >= NEAR && z1 >= NEAR && z2 >= NEAR && area != 0.0 && area == area) {
            if (area < 0.0) {                                 // orient: swap corners 1 and 2
                float t;
                t = x1; x1 = x2; x2 = t;
                t = y1; y1 = y2; y2 = t;
                t = z1; z1 = z2; z2 = t;
            }
            const float mnx = fminf(x0, fminf(x1, x2)), mxx = fmaxf(x0, fmaxf(x1, x2));
            const float mny = fminf(y0, fminf(y1, y2)), mxy = fmaxf(y0, fmaxf(y1, y2));
            // pixel x is inside when mnx <= x + 0.5 <= mxx; clamp in float before the integer conversion
            const float bx0 = fmaxf(ceilf(mnx - 0.5f), 0.f), bx1 = fminf(floorf(mxx - 0.5f), (float)(width - 1));
            const float by0 = fmaxf(ceilf(mny - 0.5f), 0.f), by1 = fminf(floorf(mxy - 0.5f), (float)(height - 1));
            if (bx0 <= bx1 && by0 <= by1) {
                const int ix0 = (int)bx0, iy0 = (int)by0, bw = (int)bx1 - ix0 + 1, bh = (int)by1 - iy0 + 1;
                count = (int64_t)bw * bh;
                r0 = {x0, y0, x1, y1};
                r1 = {x2, y2, z0, z1};
                r2 = {z2, __int_as_float(ix0), __int_as_float(iy0), __int_as_float(bw)};
            }
        }
    }
    rec[3 * f] = r0;
    rec[3 * f + 1] = r1;
    rec[3 * f + 2] = r2;
    cnt[f] = count;
}

constexpr int SCAN_BLOCK = 1024;

// In-place inclusive prefix of cnt [n] by one workgroup: thread t owns a contiguous chunk, chunk sums are scanned in LDS.
__global__ __launch_bounds__(SCAN_BLOCK) void scan_kernel(int64_t* __restrict__ cnt, int64_t n) {
    __shared__ int64_t sums[SCAN_BLOCK];
    const int tid = threadIdx.x;
    const int64_t chunk = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int64_t b = tid * chunk, e = b + chunk < n ? b + chunk : n;
    int64_t s = 0;
    for (int64_t i = b; i < e; ++i) s += cnt[i];
    sums[tid] = s;
    __syncthreads();
    for (int off = 1; off < SCAN_BLOCK; off <<= 1) {          // Hillis-Steele inclusive scan of the chunk sums
        const int64_t v = tid >= off ? sums[tid - off] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int64_t run = tid > 0 ? sums[tid - 1] : 0;
    for (int64_t i = b; i < e; ++i) {
        run += cnt[i];
        cnt[i] = run;
    }
}

// Grid-stride over the pixel work items [0, prefix[nf-1]): item i belongs to the face of the first prefix entry > i.
__global__ __launch_bounds__(256) void raster_faces_kernel(const float4* __restrict__ rec, const int64_t* __restrict__ prefix, int64_t nf,
                                                           int width, unsigned long long* __restrict__ keys) {
    const int64_t total = prefix[nf - 1];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        int64_t lo = 0, hi = nf - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (prefix[mid] > i) hi = mid; else lo = mid + 1;
        }
        const int local = (int)(i - (lo > 0 ? prefix[lo - 1] : 0));
        const float4 r0 = rec[3 * lo], r1 = rec[3 * lo + 1], r2 = rec[3 * lo + 2];
        const int bw = __float_as_int(r2.w);
        const int px = __float_as_int(r2.y) + local % bw, py = __float_as_int(r2.z) + local / bw;
        const double cx = px + 0.5, cy = py + 0.5;
        const double x0 = r0.x, y0 = r0.y, x1 = r0.z, y1 = r0.w, x2 = r1.x, y2 = r1.y;
        const double e0 = edge_fn(x1, y1, x2, y2, cx, cy);
        const double e1 = edge_fn(x2, y2, x0, y0, cx, cy);
        const double e2 = edge_fn(x0, y0, x1, y1, cx, cy);
        const bool in0 = e0 > 0.0 || (e0 == 0.0 && owned(x1, y1, x2, y2));
        const bool in1 = e1 > 0.0 || (e1 == 0.0 && owned(x2, y2, x0, y0));
        const bool in2 = e2 > 0.0 || (e2 == 0.0 && owned(x0, y0, x1, y1));
        if (in0 && in1 && in2) {
            const double area = edge_fn(x0, y0, x1, y1, x2, y2);
            const double iz = ((e0 / area) / (double)r1.z + (e1 / area) / (double)r1.w) + (e2 / area) / (double)r2.x;
            const float depth = (float)(1.0 / iz);
            const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)lo;
            atomicMin(keys + (int64_t)py * width + px, key);
        }
    }
}

__global__ __launch_bounds__(256) void raster_points_kernel(const float* __restrict__ pts, int64_t n, Cam cam, int width, int height, float radius,
                                                            unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sx, sy, z;
    project(cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], sx, sy, z);
    if (!(z >= NEAR) || !(fabsf(sx) < 1e7f) || !(fabsf(sy) < 1e7f)) return;
    const float bx0 = fmaxf(ceilf(sx - radius - 0.5f), 0.f), bx1 = fminf(floorf(sx + radius - 0.5f), (float)(width - 1));
    const float by0 = fmaxf(ceilf(sy - radius - 0.5f), 0.f), by1 = fminf(floorf(sy + radius - 0.5f), (float)(height - 1));
    const double r2 = (double)radius * (double)radius;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)i;
    for (int py = (int)by0; py <= (int)by1; ++py) {
        for (int px = (int)bx0; px <= (int)bx1; ++px) {
            const double dx = (px + 0.5) - (double)sx, dy = (py + 0.5) - (double)sy;
            if (dx * dx + dy * dy <= r2) atomicMin(keys + (int64_t)py * width + px, key);
        }
    }
}

__device__ __forceinline__ uint8_t to_u8(float c) {
    const float v = c + 0.5f;
    return (uint8_t)(v >= 255.f ? 255 : (v <= 0.f ? 0 : (int)v));
}

__global__ __launch_bounds__(256) void shade_kernel(const unsigned long long* __restrict__ keys, int width, int height, const float* __restrict__ verts,
                                                    const int32_t* __restrict__ faces, const uint8_t* __restrict__ colors, uint32_t rgb, Cam cam,
                                                    uint8_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)width * height) return;
    const unsigned long long key = keys[p];
    float cr = 255.f, cg = 255.f, cb = 255.f;
    if (key != ~0ull) {
        const int64_t id = (int64_t)(uint32_t)(key & 0xffffffffull);
        cr = (float)((rgb >> 16) & 255u);
        cg = (float)((rgb >> 8) & 255u);
        cb = (float)(rgb & 255u);
        if (!faces) {
            if (colors) {
                cr = colors[3 * id];
                cg = colors[3 * id + 1];
                cb = colors[3 * id + 2];
            }
        } else {
            const int64_t vi[3] = {faces[3 * id], faces[3 * id + 1], faces[3 * id + 2]};
            V3<float> w[3];
            double sx[3], sy[3], z[3];
            for (int k = 0; k < 3; ++k) {
                w[k] = {verts[3 * vi[k]], verts[3 * vi[k] + 1], verts[3 * vi[k] + 2]};
                float fx, fy, fz;
                project(cam, w[k].x, w[k].y, w[k].z, fx, fy, fz);
                sx[k] = fx; sy[k] = fy; z[k] = fz;
            }
            const double px = (double)(p % width) + 0.5, py = (double)(p / width) + 0.5;
            const double area = edge_fn(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
            double b[3] = {edge_fn(sx[1], sy[1], sx[2], sy[2], px, py) / area, edge_fn(sx[2], sy[2], sx[0], sy[0], px, py) / area,
                           edge_fn(sx[0], sy[0], sx[1], sy[1], px, py) / area};
            const double iz = (b[0] / z[0] + b[1] / z[1]) + b[2] / z[2];
            double lam[3];
            for (int k = 0; k < 3; ++k) lam[k] = (b[k] / z[k]) / iz;  // perspective-correct barycentrics
            if (colors) {
                double acc[3] = {0, 0, 0};
                for (int k = 0; k < 3; ++k)
                    for (int ch = 0; ch < 3; ++ch) acc[ch] += lam[k] * (double)colors[3 * vi[k] + ch];
                cr = (float)acc[0];
                cg = (float)acc[1];
                cb = (float)acc[2];
            }
            const V3<double> a = {w[0].x, w[0].y, w[0].z}, bb = {w[1].x, w[1].y, w[1].z}, c = {w[2].x, w[2].y, w[2].z};
            V3<double> n = cross(sub(bb, a), sub(c, a));
            const V3<double> x = {lam[0] * a.x + lam[1] * bb.x + lam[2] * c.x, lam[0] * a.y + lam[1] * bb.y + lam[2] * c.y,
                                  lam[0] * a.z + lam[1] * bb.z + lam[2] * c.z};
            V3<double> v = sub(V3<double>{cam.eye[0], cam.eye[1], cam.eye[2]}, x);
            const double ln = sqrt(dot(n, n)), lv = sqrt(dot(v, v));
            const double cosv = (ln > 0.0 && lv > 0.0) ? fabs(dot(n, v)) / (ln * lv) : 0.0;
            const float k = (float)(0.3 + 0.7 * (cosv > 1.0 ? 1.0 : cosv));
            cr *= k;
            cg *= k;
            cb *= k;
        }
    }
    out[3 * p] = to_u8(cr);
    out[3 * p + 1] = to_u8(cg);
    out[3 * p + 2] = to_u8(cb);
}

Cam make_cam(const float* cam, int width, int height) {
    Cam c;
    for (int k = 0; k < 9; ++k) c.m[k] = cam[k];
    for (int k = 0; k < 3; ++k) c.eye[k] = cam[9 + k];
    c.f = cam[12];
    c.hw = 0.5f * (float)width;
    c.hh = 0.5f * (float)height;
    return c;
}

constexpr int RASTER_BLOCKS = 2048;                           // 256 CUs x 8 workgroups of the grid-stride pixel loop

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int64_t pps_vis_closest_slices(int64_t m, int64_t nf) { return sweep_slices(m, nf); }

int pps_vis_closest_point(const float* corners, int64_t nf, const float* query, int64_t m, int64_t slices, float* partial_d2, int32_t* partial_face,
                          float* out_d, int32_t* out_face, float* out_pt, void* stream) {
    if (nf < 1 || m < 0 || nf > INT32_MAX) return PPS_ERR_ARG;
    if (m == 0) return PPS_OK;
    if (!corners || !query || !partial_d2 || !partial_face || !out_d || !out_face || !out_pt) return PPS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t used = sweep_launch(corners, nf, m, slices, ClosestOp{query, partial_d2, partial_face}, st);
    if (!used) return PPS_ERR_ARG;
    hipLaunchKernelGGL(closest_final_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, corners, query, m, used, (const float*)partial_d2,
                       (const int32_t*)partial_face, out_d, out_face, out_pt);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

size_t pps_vis_raster_ws_bytes(int64_t nv, int64_t nf) {
    if (nv < 0 || nf < 0) return 0;
    return align256((size_t)nv * 3 * sizeof(float)) + align256((size_t)nf * 3 * sizeof(float4)) + align256((size_t)nf * sizeof(int64_t));
}

int pps_vis_raster_faces(const float* verts, int64_t nv, const int32_t* faces, int64_t nf, const float* cam, int width, int height, void* ws,
                         size_t ws_bytes, void* keys, void* stream) {
    if (nv < 0 || nf < 0 || width < 1 || height < 1 || width > 16384 || height > 16384 || nf > INT32_MAX) return PPS_ERR_ARG;
    if (nf == 0 || nv == 0) return PPS_OK;
    if (!verts || !faces || !cam || !ws || !keys || ws_bytes < pps_vis_raster_ws_bytes(nv, nf)) return PPS_ERR_ARG;
    const Cam c = make_cam(cam, width, height);
    char* w = (char*)ws;
    float* proj = (float*)w;
    float4* rec = (float4*)(w + align256((size_t)nv * 3 * sizeof(float)));
    int64_t* prefix = (int64_t*)((char*)rec + align256((size_t)nf * 3 * sizeof(float4)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, verts, nv, c, proj);
    hipLaunchKernelGGL(face_setup_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, faces, nf, nv, (const float*)proj, width, height, rec,
                       prefix);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, prefix, nf);
    hipLaunchKernelGGL(raster_faces_kernel, dim3(RASTER_BLOCKS), dim3(256), 0, st, (const float4*)rec, (const int64_t*)prefix, nf, width,
                       (unsigned long long*)keys);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_vis_raster_points(const float* pts, int64_t n, const float* cam, int width, int height, float radius, void* keys, void* stream) {
    if (n < 0 || width < 1 || height < 1 || width > 16384 || height > 16384 || n > INT32_MAX || !(radius >= 0.f && radius <= 64.f)) return PPS_ERR_ARG;
    if (n == 0) return PPS_OK;
    if (!pts || !cam || !keys) return PPS_ERR_ARG;
    hipLaunchKernelGGL(raster_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, n, make_cam(cam, width, height),
                       width, height, radius, (unsigned long long*)keys);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int pps_vis_shade(const void* keys, int width, int height, const float* verts, const int32_t* faces, const uint8_t* colors, uint32_t rgb,
                  const float* cam, uint8_t* out, void* stream) {
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return PPS_ERR_ARG;
    if (!keys || !out || !cam || (faces && !verts)) return PPS_ERR_ARG;
    const int64_t np = (int64_t)width * height;
    hipLaunchKernelGGL(shade_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)keys, width, height,
                       verts, faces, colors, rgb, make_cam(cam, width, height), out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
