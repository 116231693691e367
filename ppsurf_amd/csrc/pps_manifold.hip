// Manifold split for gfx950: an edge with three and more owners and a vertex whose faces form several fans are cut apart by duplicating
// vertices.
//
// new capability: replaces nothing -- the reference has no such stage, and the stages of sections 19 to 23 step around non-manifold geometry
// without repairing it.  Driven by ppsurf_amd/manifold.py (the pairs and their edge slots by ppsurf_amd/topology.py, the loop and the compress
// launch by ppsurf_amd/labels.py); restated in numpy by tests/manifold_spec.py (a plain union-find over
// corners), which the kernels match byte for byte.
//
// The rule: vertices V [nv,3], faces F int64 [nf,3], nv, nf <= 2^31 - 1, 3 nf <= 2^31 - 1.  A pure function of the ordered mesh.
//   corner     c = 3 f + k of a valid face f (face_valid of pps_faces.h) names the vertex F[f][k].  The corners of an invalid face take no
//              part: label -1.
//   link       for every pair (fa, fb, ea, eb) of topology.manifold_pair_edges -- an undirected edge that EXACTLY TWO valid faces hold, with
//              its slot in each (slot k is corner k -> corner k + 1 mod 3) -- and for each of the edge's two end vertices, the corner of fa
//              that names it is linked with the corner of fb that names it.  The four corners are read from F: a0 = F[fa][ea],
//              a1 = F[fa][ea + 1], b0 = F[fb][eb], b1 = F[fb][eb + 1] (slots mod 3).  fb runs the edge the same way (a0 == b0, a1 == b1):
//              corner ea links with eb and ea + 1 with eb + 1.  The other way (a0 == b1, a1 == b0): ea with eb + 1 and ea + 1 with eb.  A
//              pair whose two slots do not name the same two vertices is skipped.  Winding coherence plays no part; two copies of one
//              triangle are three pairs, hence linked corner by corner.
//   fan        a connected component of the links; its leader is its smallest corner; label[c] = the leader of c's fan (int32).  All
//              corners of a fan name one vertex (a link joins two corners that name the same vertex).
//   rows       at vertex v the fan with the smallest leader keeps row v; every other fan gets a new row, appended after the nv given rows
//              in ascending order of fan leader, which holds v's position byte for byte.  A vertex without a valid face stays.
//              source int64 [nv_out] is the given row of every output row (host: integer work on small tables, as in section 24).
//   faces      every corner of a valid face is renamed to its fan's row, newrow[label[c]]; an invalid face is copied as given; order and
//              winding are untouched.  No face is added, removed or re-wound and no vertex moves.
// Why the result is manifold: around a vertex a face has two edges, so the link graph at the vertex has degree <= 2: paths and cycles.  A
// face is a path end at an edge with fewer or more than two owners, and a component has at most two ends.  So after the split at most two
// faces of a former many-owner edge still share both its ends and no edge has three owners.  An edge that drops to two owners only closes
// a path of one fan into a cycle, so a second run finds one fan per vertex: the stage is idempotent.  The cut closes nothing: the faces of a
// many-owner edge that the fans do not pair become borders.
//
// Labelling (hook_kernel here, the compress of pps_labels.hip on the 3 nf corner labels; the argument is written out in pps_labels.h).  A
// node is a corner, a link as above, found on the fly: label[c] starts as c, -1 for a corner of an invalid face.
//   hook      one thread per pair; both of its unions are done in that thread, so no link list is materialised.  A union joins the ends of
//             its two corners (join_ends of pps_labels.h): the flag goes up only when a label fell, so a launch raises it exactly when it
//             changed a label.
//   skipped   a union onto a corner with a negative label; a pair with a face, a slot or a corner vertex out of range or without a common
//             edge.
//
// Shape: hook_kernel one thread per pair; faces_kernel one thread per face.  Plain vector loads and stores, integer atomics only, no LDS,
// no scratch.  Everything read is range-checked before it becomes an address: the face indices and the slots of a pair, the vertex indices
// of its four corners, every label, every newrow entry.
#include "pps_common.h"
#include "pps_faces.h"
#include "pps_labels.h"
#include "../../include/ppsurf_amd_ext.h"

namespace {

// the corners x, y (0 <= x, y < 3 nf, by the caller) are linked: their ends are joined
__device__ __forceinline__ void join(int32_t* label, int x, int y, int32_t* changed) {
    if (load_label(label, x) < 0 || load_label(label, y) < 0) return;                       // a corner that takes no part
    join_ends(label, x, y, changed);
}

__global__ __launch_bounds__(256) void hook_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, const int32_t* __restrict__ fa,
                                                   const int32_t* __restrict__ fb, const int32_t* __restrict__ ea, const int32_t* __restrict__ eb,
                                                   int64_t np, int32_t* label, int32_t* changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const int a = fa[i], b = fb[i], sa = ea[i], sb = eb[i];
    if (a < 0 || a >= nf || b < 0 || b >= nf || sa < 0 || sa > 2 || sb < 0 || sb > 2) return;
    const int ta = sa == 2 ? 0 : sa + 1, tb = sb == 2 ? 0 : sb + 1;                         // the slot's second corner
    const int64_t a0 = faces[3 * (int64_t)a + sa], a1 = faces[3 * (int64_t)a + ta], b0 = faces[3 * (int64_t)b + sb], b1 = faces[3 * (int64_t)b + tb];
    if (a0 < 0 || a0 >= nv || a1 < 0 || a1 >= nv || b0 < 0 || b0 >= nv || b1 < 0 || b1 >= nv) return;
    const int ca = 3 * a, cb = 3 * b;                                                      // 3 nf <= 2^31 - 1, by the entry
    if (a0 == b0 && a1 == b1) {                                                            // fb runs the edge the same way
        join(label, ca + sa, cb + sb, changed);
        join(label, ca + ta, cb + tb, changed);
    } else if (a0 == b1 && a1 == b0) {                                                     // the other way: the links cross
        join(label, ca + sa, cb + tb, changed);
        join(label, ca + ta, cb + sb, changed);
    }                                                                                       // no common edge: skipped
}

__global__ __launch_bounds__(256) void faces_kernel(const int64_t* __restrict__ faces, int64_t nf, int64_t nv, const int32_t* __restrict__ label,
                                                    const int64_t* __restrict__ newrow, int64_t nv_out, int64_t* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int64_t given[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    int64_t row[3] = {given[0], given[1], given[2]};
    if (face_valid(given[0], given[1], given[2], nv)) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t l = label[3 * f + k];
            if (l >= 3 * nf) ok = false;                                                    // no corner: the face is copied
            else if (l >= 0) row[k] = newrow[l];
        }
        if (!ok || !face_in_range(row[0], row[1], row[2], nv_out)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) row[k] = given[k];
        }
    }
    out[3 * f] = row[0];
    out[3 * f + 1] = row[1];
    out[3 * f + 2] = row[2];
}

inline bool too_many(int64_t n) { return n > (int64_t)INT32_MAX; }

}  // namespace

extern "C" {

int ppsx_manifold_hook(const int64_t* faces, int64_t nf, int64_t nv, const int32_t* fa, const int32_t* fb, const int32_t* ea, const int32_t* eb,
                       int64_t np, int32_t* label, int32_t* changed, void* stream) {
    if (nf < 0 || nv < 0 || np < 0 || too_many(nf) || too_many(nv) || too_many(np) || too_many(3 * nf)) return PPS_ERR_ARG;
    if (np == 0 || nf == 0) return PPS_OK;
    if (!faces || !fa || !fb || !ea || !eb || !label || !changed) return PPS_ERR_ARG;
    hipLaunchKernelGGL(hook_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, fa, fb, ea, eb, np, label,
                       changed);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

int ppsx_manifold_faces(const int64_t* faces, int64_t nf, int64_t nv, const int32_t* label, const int64_t* newrow, int64_t nv_out, int64_t* out,
                        void* stream) {
    if (nf < 0 || nv < 0 || nv_out < 0 || too_many(nf) || too_many(nv) || too_many(nv_out) || too_many(3 * nf)) return PPS_ERR_ARG;
    if (nf == 0) return PPS_OK;
    if (!faces || !label || !newrow || !out || out == faces) return PPS_ERR_ARG;
    hipLaunchKernelGGL(faces_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, nf, nv, label, newrow, nv_out, out);
    return hipGetLastError() == hipSuccess ? PPS_OK : PPS_ERR_LAUNCH;
}

}  // extern "C"
