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

/* ---- trim by support: faces of a mesh that a scan point stands for (csrc/pps_trim.hip) ------------------------------------------------------
 * new capability: replaces nothing -- the reference closes every surface.  Driven by ppsurf_amd/trim.py; the rule is written out at the top
 * of csrc/pps_trim.hip and in DESIGN.md section 15.  lo, hi are HOST arrays of three floats (the cloud's box), h, inv_h the cell edge and
 * 1 / h of the grid of csrc/pps_cells.h, table uint64 [capacity] with capacity a power of two > n.
 *   ppsx_trim_cell_slots    slot int64 [n]: the table slot of the cell of every point of pts f32 [n,3]; fills table.  Which slot a cell gets
 *                           depends on timing, which points share a slot does not.  A NULL pointer, n < 1, a capacity that is no power of
 *                           two > n, or a grid the rule of pps_cells.h refuses (h or inv_h not > 0, hi < lo, more than 2^20 cells along an
 *                           axis): PPS_ERR_ARG, nothing is launched or written.
 *   ppsx_trim_face_support  support u8 [nf]: 1 when the face faces[f] = (i0, i1, i2) int64 of verts f32 [nv,3] has every index in [0, nv),
 *                           finite corners and a point p of pts f32 [n,3] with d2(p, triangle) <= r * r, else 0; d2 is the squared
 *                           distance to the closest point of the triangle in fp64 (closest_on_triangle<double> of csrc/pps_tri.h on the
 *                           widened inputs, every operation rounded on its own).  order int64 [n] lists the points sorted by slot, offsets
 *                           int64 [capacity + 1] the start of every slot's run in it (table, slots from ppsx_trim_cell_slots with the same
 *                           lo, hi, h, inv_h, capacity).  A pure function of (pts, verts, faces, r): it does not depend on h, capacity,
 *                           slots or the launch; one wave per face, no atomics.  Indices outside [0, nv) are never read through, and
 *                           entries of offsets / order outside [0, n] / [0, n) are skipped.
 *                           nf < 0, nv < 0, n < 0, r not finite or not > 0, h < r, or -- with nf > 0 and n > 0 -- a NULL pointer, a bad
 *                           capacity or a refused grid: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *                           n == 0 (nf > 0, support not NULL): 0, support is zeroed. */
int ppsx_trim_cell_slots(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, uint64_t* table, int64_t capacity,
                         int64_t* slot, void* stream);
int ppsx_trim_face_support(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* pts, int64_t n, const float* lo,
                           const float* hi, float h, float inv_h, const uint64_t* table, int64_t capacity, const int64_t* order,
                           const int64_t* offsets, double r, uint8_t* support, void* stream);

/* ---- Taubin lambda|mu smoothing of a mesh (csrc/pps_smooth.hip) ----------------------------------------------------------------------------
 * new capability: replaces nothing -- the reference has no smoothing.  Driven by ppsurf_amd/smooth.py; the rule is written out at the top of
 * csrc/pps_smooth.hip and in DESIGN.md section 16.
 *   ppsx_smooth_half_edges  keys int64 [6 nf]: per face (a, b, c) of faces int64 [nf,3] the half-edges a->b, b->a, b->c, c->b, c->a, a->c as
 *                           (src << 32) | dst.  A face with an index outside [0, nv) or two equal indices is invalid: its six keys are
 *                           INT64_MAX, so they sort last.  nv <= 2^31 - 1 keeps every other key positive.
 *                           nf < 0, nv < 0, nv > 2^31 - 1, or a NULL pointer with nf > 0: PPS_ERR_ARG, nothing is launched or written.
 *                           nf == 0: 0, nothing is launched.
 *   ppsx_smooth_pass        out f64 [nv,3]: one Jacobi pass with factor s over x f64 [nv,3].  Row i of the adjacency is the entries
 *                           offsets[i] .. offsets[i + 1] - 1 (offsets int64 [nv + 1]) of nbr int32 [ne] (the neighbours, ascending) and
 *                           mult int32 [ne] (the number of valid faces on the edge).  A row with an entry of multiplicity 1 belongs to a
 *                           border vertex and admits only its entries of multiplicity 1; any other row admits all.  Per component in fp64,
 *                           in row order, every operation rounded on its own: acc = 0.0; acc = acc + x[j]; m = acc / double(count);
 *                           out[i] = x[i] + s * (m - x[i]).  A vertex that admits no neighbour: out[i] = x[i].  A pure function of its
 *                           inputs: one thread per vertex, no atomics.  A row whose offsets are not 0 <= offsets[i] <= offsets[i + 1] <= ne
 *                           is skipped whole and a neighbour outside [0, nv) is skipped; neither is read through.
 *                           nv < 0, ne < 0, s not finite, out == x, or -- with nv > 0 -- a NULL x, offsets or out, or with ne > 0 a NULL
 *                           nbr or mult: PPS_ERR_ARG, nothing is launched or written.  nv == 0: 0, nothing is launched. */
int ppsx_smooth_half_edges(const int64_t* faces, int64_t nf, int64_t nv, int64_t* keys, void* stream);
int ppsx_smooth_pass(const double* x, int64_t nv, const int64_t* offsets, const int32_t* nbr, const int32_t* mult, int64_t ne, double s,
                     double* out, void* stream);

/* ---- oriented normals: per vertex on a mesh, per point on a scan (csrc/pps_normals.hip) -----------------------------------------------------
 * new capability: replaces nothing -- the reference writes positions only.  Driven by ppsurf_amd/normals.py; the rule is written out at the
 * top of csrc/pps_normals.hip and in DESIGN.md section 17.  A face is valid when its three indices lie in [0, nv) and are pairwise distinct.
 *   ppsx_normals_corner_keys  keys int64 [3 nf]: per face t = (a, b, c) of faces int64 [nf,3] the keys (a << 32) | t, (b << 32) | t,
 *                             (c << 32) | t, in that order; INT64_MAX three times for an invalid face, so those sort last.  nv, nf <= 2^31 - 1
 *                             keeps every other key positive and distinct: sorted, they list every vertex's faces in ascending face index.
 *                             nf < 0, nv < 0, nf or nv > 2^31 - 1, or a NULL pointer with nf > 0: PPS_ERR_ARG, nothing is launched or
 *                             written.  nf == 0: 0, nothing is launched.
 *   ppsx_normals_vertex       out f32 [nv,3]: the normal of every vertex of verts f32 [nv,3].  Row i of the incidence is the entries
 *                             offsets[i] .. offsets[i + 1] - 1 (offsets int64 [nv + 1]) of inc int32 [ni], the faces that hold vertex i.  Per
 *                             vertex, in fp64 on the widened coordinates, in row order, every operation rounded on its own: acc = (0, 0, 0);
 *                             for a face t with i at corner p, n the next corner cyclically and q the one after: e1 = V[n] - V[i],
 *                             e2 = V[q] - V[i], g = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); weight 0 (area):
 *                             acc = acc + g; weight 1 (max): d = ((e1x^2 + e1y^2) + e1z^2) * ((e2x^2 + e2y^2) + e2z^2), acc = acc + g / d
 *                             when d > 0 and finite, else the face adds nothing.  L = sqrt((accx^2 + accy^2) + accz^2); out[i] =
 *                             f32(acc / L) when L > 0 and finite, else (0, 0, 0).  A pure function of its inputs: one thread per vertex, no
 *                             atomics.  A row whose offsets are not 0 <= offsets[i] <= offsets[i + 1] <= ni yields (0, 0, 0); an entry of inc
 *                             outside [0, nf), an invalid face and a face that does not hold i are skipped; none is read through.
 *                             nv < 0, nf < 0, ni < 0, nv or nf > 2^31 - 1, weight not 0 or 1, or -- with nv > 0 -- a NULL verts, offsets or
 *                             out, a NULL faces with nf > 0 or a NULL inc with ni > 0: PPS_ERR_ARG, nothing is launched or written.
 *                             nv == 0: 0, nothing is launched.  nf == 0 or ni == 0 (nv > 0): out is all zeros.
 *   ppsx_normals_blend        out f32 [m,3]: the inverse-squared-distance blend of the normals f32 [nv,3] of the k neighbours idx int64 [m,k]
 *                             with squared distances d2 f32 [m,k] (ops.KnnBlocks.query(..., return_d2=True)).  Per row, in fp64, j = 0..k-1 in
 *                             column order, every operation rounded on its own: a neighbour counts when 0 <= idx[i,j] < nv;
 *                             w = 1 / (double(d2[i,j]) + eps); T[c] = T[c] + w * double(normals[idx[i,j], c]).  L = sqrt((Tx^2 + Ty^2) + Tz^2);
 *                             out[i] = f32(T / L) when L > 0 and finite, else (0, 0, 0).  A pure function of its inputs: one thread per row,
 *                             no atomics.  Indices outside [0, nv) are skipped, never read through.
 *                             m < 0, nv < 0, k outside 1..256, eps not > 0, or -- with m > 0 -- a NULL idx, d2 or out, or a NULL normals with
 *                             nv > 0: PPS_ERR_ARG, nothing is launched or written.  m == 0: 0, nothing is launched. */
int ppsx_normals_corner_keys(const int64_t* faces, int64_t nf, int64_t nv, int64_t* keys, void* stream);
int ppsx_normals_vertex(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* inc, int64_t ni,
                        int weight, float* out, void* stream);
int ppsx_normals_blend(const int64_t* idx, const float* d2, int64_t m, int k, const float* normals, int64_t nv, double eps, float* out,
                       void* stream);

/* ---- hole filling: short border loops of a mesh are closed (csrc/pps_fill.hip) --------------------------------------------------------------
 * new capability: replaces nothing -- the reference has no mesh repair.  Driven by ppsurf_amd/fill.py and topology.rim_rows; the rule is
 * written out at the top of csrc/pps_fill.hip and in DESIGN.md section 19.  In short: a face is valid when its three indices lie in [0, nv)
 * and are pairwise distinct; the multiplicity of an edge is the number of valid faces that hold it; a loose triangle is a valid face whose
 * three edges all have multiplicity 1; a rim half-edge is a directed half-edge u->v (a->b, b->c, c->a) of a valid, non-loose face whose
 * edge has multiplicity 1; a vertex is simple when exactly one rim half-edge leaves it and exactly one enters it, and succ(u) is where the
 * one that leaves goes; a loop is a cycle s_0 .. s_{L-1} of succ over simple vertices with s_0 its smallest index (the leader), filled when
 * L <= max_edges: L == 3 by the face (s_0, s_2, s_1), L > 3 by the faces (s_{j+1}, s_j, c), j = 0..L-1, s_L = s_0, around a new vertex c =
 * f32(acc / double(L)), acc = 0.0; acc = acc + double(V[s_j]) in loop order, per component in fp64, every operation rounded on its own.
 * Loops come in ascending leader; the new vertices and faces are appended.  No entry uses atomics.
 *   ppsx_fill_rim_keys  keys int64 [3 nf]: per face (a, b, c) of faces int64 [nf,3] the keys of a->b, b->c, c->a in that order, (u << 32) | v
 *                       for a rim half-edge and INT64_MAX otherwise (an invalid face, an edge of another multiplicity, all three keys of a
 *                       loose triangle).  The multiplicity is looked up by binary search for v in row u of the adjacency: the entries
 *                       offsets[u] .. offsets[u + 1] - 1 (offsets int64 [nv + 1]) of nbr int32 [ne] (ascending) and mult int32 [ne], as
 *                       topology.adjacency_rows builds them.  A row whose offsets are not 0 <= offsets[u] <= offsets[u + 1] <= ne and a
 *                       row without v give multiplicity 0; neither is read through.
 *                       nf < 0, nv < 0, ne < 0, nf or nv > 2^31 - 1, or -- with nf > 0 -- a NULL faces or keys, a NULL offsets with
 *                       nv > 0, a NULL nbr or mult with ne > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is
 *                       launched.
 *   ppsx_fill_loops     len int32 [nc]: for every candidate v = cand[i] (int64 [nc]) the length L of the loop that v leads, else 0.  The
 *                       walk follows succ int32 [nv] from v and ends with 0 at an entry that is negative or >= nv, at the first vertex
 *                       < v (v is no leader), after max_edges steps without a return to v, and for a return after fewer than 3 steps; a
 *                       candidate outside [0, nv) gives 0.  At most nc x max_edges steps in all (a long rim whose indices ascend along
 *                       it); near the size of the rims for a typical labelling.
 *                       nc < 0, nv < 0, nc or nv > 2^31 - 1, max_edges outside 3..4096, or -- with nc > 0 -- a NULL cand or len or a NULL
 *                       succ with nv > 0: PPS_ERR_ARG, nothing is launched or written.  nc == 0: 0, nothing is launched.
 *   ppsx_fill_emit      the new vertex and the new faces of every loop i of nl: leader int64 [nl], len int32 [nl] (3..4096), vslot int64
 *                       [nl] (the row of new_verts f32 [nnew,3] of a loop with len > 3; not read for len == 3) and foff int64 [nl] (the
 *                       first of its len -- for len == 3 one -- rows of new_faces int64 [nfnew,3]).  The new vertex gets the index
 *                       nv + vslot[i].  One lane per loop walks succ int32 [nv] from the leader over verts f32 [nv,3], re-checking every
 *                       entry.  A loop that does not return to its leader after exactly len steps (an entry outside [0, nv), an earlier
 *                       return, none), a leader outside [0, nv), a len outside 3..4096, a vslot outside [0, nnew) or rows outside
 *                       [0, nfnew) writes NOTHING: its rows keep what the caller put there (fill.py: the invalid face (-1, -1, -1) and a
 *                       zero vertex).  Rows of two loops that overlap are the caller's error; they stay inside the buffers.
 *                       nv, nl, nnew or nfnew < 0 or > 2^31 - 1, or -- with nl > 0 -- a NULL leader, len, vslot or foff, a NULL verts or
 *                       succ with nv > 0, a NULL new_verts with nnew > 0 or a NULL new_faces with nfnew > 0: PPS_ERR_ARG, nothing is
 *                       launched or written.  nl == 0: 0, nothing is launched. */
int ppsx_fill_rim_keys(const int64_t* faces, int64_t nf, int64_t nv, const int64_t* offsets, const int32_t* nbr, const int32_t* mult, int64_t ne,
                       int64_t* keys, void* stream);
int ppsx_fill_loops(const int64_t* cand, int64_t nc, const int32_t* succ, int64_t nv, int max_edges, int32_t* len, void* stream);
int ppsx_fill_emit(const float* verts, int64_t nv, const int32_t* succ, const int64_t* leader, const int32_t* len, const int64_t* vslot,
                   const int64_t* foff, int64_t nl, float* new_verts, int64_t nnew, int64_t* new_faces, int64_t nfnew, void* stream);

/* ---- feature-preserving denoising: face-normal filtering, then a vertex update (csrc/pps_denoise.hip) ---------------------------------------
 * new capability: replaces nothing -- the reference has no mesh denoising.  Driven by ppsurf_amd/denoise.py; the rule (Sun, Rosin, Martin,
 * Langbein 2007) is written out at the top of csrc/pps_denoise.hip and in DESIGN.md section 20.  A face is valid when its three indices lie
 * in [0, nv) and are pairwise distinct.  Row v of the incidence is the entries offsets[v] .. offsets[v + 1] - 1 (offsets int64 [nv + 1]) of
 * inc int32 [ni], the valid faces that hold vertex v in ascending face index, as topology.incidence_rows builds them.  All arithmetic is
 * fp64, every operation rounded on its own; one thread per face or vertex, no atomics: each entry is a pure function of its inputs.
 *   ppsx_denoise_face_normals  normals f64 [nf,3]: for a valid face (a, b, c) of faces int64 [nf,3] over verts f32 [nv,3], widened:
 *                              e1 = x_b - x_a, e2 = x_c - x_a, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 *                              L = sqrt((nx^2 + ny^2) + nz^2); n / L when L > 0 and finite, else (0, 0, 0).  An invalid face gets
 *                              (0, 0, 0) and is not read through.
 *                              nv < 0, nf < 0, nv or nf > 2^31 - 1, or -- with nf > 0 -- a NULL faces or normals or a NULL verts with
 *                              nv > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *   ppsx_denoise_filter_pass   out f64 [nf,3]: one Jacobi pass of the normal filter over normals f64 [nf,3].  A valid face i = (a, b, c)
 *                              merges the rows of a, b and c: the smallest head j is taken and every row that shows j moves on, so a
 *                              face listed in several rows is visited once, in ascending index.  Per visit
 *                              d = (n_i.x n_j.x + n_i.y n_j.y) + n_i.z n_j.z, and when d > threshold: w = (d - threshold) * (d - threshold),
 *                              acc_c = acc_c + w * n_j.c.  L = sqrt((accx^2 + accy^2) + accz^2); out[i] = acc / L when L > 0 and finite,
 *                              else n_i.  An invalid face gets (0, 0, 0).  A row whose offsets are not 0 <= offsets[v] <= offsets[v + 1]
 *                              <= ni counts as empty and an entry outside [0, nf) is skipped; neither is read through.  The entries are
 *                              taken as listed: the zero normal of an invalid face gives d = 0 and adds nothing.
 *                              nv, nf or ni < 0, nv or nf > 2^31 - 1, a threshold that is NaN or outside [0, 1), out == normals, or --
 *                              with nf > 0 -- a NULL faces, normals or out, a NULL offsets with nv > 0 or a NULL inc with ni > 0:
 *                              PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *   ppsx_denoise_vertex_pass   out f64 [nv,3]: one Jacobi pass of the vertex update over x f64 [nv,3] with normals f64 [nf,3].  For the
 *                              faces k = (a, b, c) of row v in row order: c_k = ((x_a + x_b) + x_c) / 3.0 per component, dv = c_k - x_v,
 *                              t = (n_k.x dv.x + n_k.y dv.y) + n_k.z dv.z, acc = acc + n_k * t; out[v] = x_v + acc / double(count).  A
 *                              row whose offsets are not 0 <= offsets[v] <= offsets[v + 1] <= ni is skipped whole; an entry outside
 *                              [0, nf), an invalid face and a face that does not hold v are skipped and not counted; none is read
 *                              through.  A vertex that counts no face: out[v] = x[v].
 *                              nv, nf or ni < 0, nv or nf > 2^31 - 1, out == x, or -- with nv > 0 -- a NULL x, offsets or out, a NULL
 *                              faces or normals with nf > 0 or a NULL inc with ni > 0: PPS_ERR_ARG, nothing is launched or written.
 *                              nv == 0: 0, nothing is launched. */
int ppsx_denoise_face_normals(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, double* normals, void* stream);
int ppsx_denoise_filter_pass(const int64_t* faces, int64_t nf, int64_t nv, const int64_t* offsets, const int32_t* inc, int64_t ni,
                             const double* normals, double threshold, double* out, void* stream);
int ppsx_denoise_vertex_pass(const double* x, int64_t nv, const int64_t* faces, int64_t nf, const double* normals, const int64_t* offsets,
                             const int32_t* inc, int64_t ni, double* out, void* stream);

/* ---- the labelling layer: the compress step of every stage that keeps int32 labels (csrc/pps_labels.hip, csrc/pps_labels.h) -------------
 * Driven by ppsurf_amd/labels.py, whose fixed_point repeats { flag = 0; a stage's hook; flag down -> done; compress }; the argument (I1,
 * I2, stale reads, the fixed point, progress, the bounds of a walk) is written out once, in csrc/pps_labels.h, and in DESIGN.md section 26.
 *   ppsx_labels_compress  every slot x of label int32 [n] with label[x] >= 0 stores the end of its walk in label[x] -- a walk steps from x
 *                         to label[x] while 0 <= label[x] < x, reads no slot outside [0, x] and takes at most x steps; a slot with a
 *                         negative label is not touched.  Runs on the face labels of section 21, the vertex labels of section 24 and the
 *                         3 nf corner labels of section 25.  256 threads, (n + 255) / 256 blocks.
 *                         n < 0, n > 2^31 - 1 or a NULL label with n > 0: PPS_ERR_ARG, nothing is launched or written.  n == 0: 0,
 *                         nothing is launched. */
int ppsx_labels_compress(int32_t* label, int64_t n, void* stream);

/* ---- isolated pieces: face components, a table per component, the rules that drop components (csrc/pps_pieces.hip) -----------------------
 * new capability: replaces nothing -- the reference's rule, remove_small_connected_components(num_faces = 6), stays with
 * pps_mesh_small_components.  Driven by ppsurf_amd/pieces.py (the keys by ppsurf_amd/topology.py, the loop by ppsurf_amd/labels.py); the
 * rule is written out at the top of csrc/pps_pieces.hip and in DESIGN.md section 21, the argument for the labelling in csrc/pps_labels.h.  A face is valid when its three indices lie in
 * [0, nv) and are pairwise distinct; two valid faces are adjacent when they share an undirected edge that exactly two valid faces hold; a
 * component's leader is its smallest face index.
 *   ppsx_pieces_edge_keys  keys int64 [3 nf]: per valid face (a, b, c) of faces int64 [nf,3] the keys of the undirected edges ab, bc, ca in
 *                          that order, (min << 32) | max; INT64_MAX three times for an invalid face, so those sort last.  Sorted, a run of
 *                          exactly two equal keys is an edge that joins its two owners (position / 3).
 *                          nf < 0, nv < 0, nf or nv > 2^31 - 1, or a NULL pointer with nf > 0: PPS_ERR_ARG, nothing is launched or
 *                          written.  nf == 0: 0, nothing is launched.
 *   ppsx_pieces_hook       one hooking round over the pairs fa, fb int32 [np] on label int32 [nf] (label[f] = f to begin with, -1 for an
 *                          invalid face): a pair (a, b) walks label from a and from b -- a walk steps from x to label[x] while
 *                          0 <= label[x] < x -- to the ends ra, rb, and when ra != rb does atomicMin(&label[max], min) and stores 1 to
 *                          *changed (int32, device; the caller zeroes it before).  A pair with an entry outside [0, nf) or onto a face
 *                          with a negative label is skipped.  No read relies on a write of the same launch; see the .hip file.
 *                          np < 0, nf < 0, np or nf > 2^31 - 1, or -- with np > 0 and nf > 0 -- a NULL pointer: PPS_ERR_ARG, nothing is
 *                          launched or written.  np == 0 or nf == 0: 0, nothing is launched.
 *   ppsx_pieces_stats      count int64 [nc], lo, hi f32 [nc,3]: per component c the number of its faces and the box of their corners over
 *                          verts f32 [nv,3], every coordinate taken as x + 0.0f.  Face f belongs to cid[f] (int32 [nf]); a face with
 *                          label[f] < 0, an invalid face and a face with cid[f] outside [0, nc) are skipped and not read through.  A
 *                          component without a face gets 0, +inf and -inf.  Integer atomics after a combine per wave and per workgroup:
 *                          exact in any order.  Every row of the outputs is written.
 *                          nv, nf or nc < 0 or > 2^31 - 1, or -- with nc > 0 -- a NULL count, lo or hi, lo == hi, with nf > 0 a NULL
 *                          faces, label or cid, with nf > 0 and nv > 0 a NULL verts: PPS_ERR_ARG, nothing is launched or written.
 *                          nc == 0: 0, nothing is launched.
 *   ppsx_pieces_select     keep u8 [nc]: 1 when component c passes every rule whose flag is 1.  min_faces: count[c] >= min_faces.
 *                          min_diag_frac: diag2 >= (min_diag_frac * min_diag_frac) * box_diag2 in fp64, diag2 = (dx dx + dy dy) + dz dz,
 *                          dx = double(hi.x) - double(lo.x) and so on, every operation rounded on its own.  keep_largest:
 *                          0 <= rank[c] < keep_largest (rank int64 [nc]: by faces descending, then leader ascending).
 *                          nc < 0 or > 2^31 - 1, a flag that is not 0 or 1, no flag set, with its flag set a min_faces or keep_largest
 *                          outside 1..2^31 - 1 or a min_diag_frac that is NaN or outside [0, 1], a box_diag2 that is negative or not
 *                          finite, or -- with nc > 0 -- a NULL keep or a NULL table that a set rule reads: PPS_ERR_ARG, nothing is
 *                          launched or written.  nc == 0: 0, nothing is launched. */
int ppsx_pieces_edge_keys(const int64_t* faces, int64_t nf, int64_t nv, int64_t* keys, void* stream);
int ppsx_pieces_hook(const int32_t* fa, const int32_t* fb, int64_t np, int32_t* label, int64_t nf, int32_t* changed, void* stream);
int ppsx_pieces_stats(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int32_t* label, const int32_t* cid, int64_t nc,
                      int64_t* count, float* lo, float* hi, void* stream);
int ppsx_pieces_select(const int64_t* count, const float* lo, const float* hi, const int64_t* rank, int64_t nc, int has_min_faces,
                       int64_t min_faces, int has_min_diag_frac, double min_diag_frac, int has_keep_largest, int64_t keep_largest,
                       double box_diag2, uint8_t* keep, void* stream);

/* ---- edge-collapse decimation: quadric error metric, rounds of independent collapses (csrc/pps_decimate.hip) -------------------------------
 * new capability: replaces nothing -- the reference has no decimation and the vertex clustering (pps_simplify_*) stays as it is.  Driven by
 * ppsurf_amd/decimate.py (the rows by ppsurf_amd/topology.py); the rule and the argument for the independence of a round's winners are
 * written out at the top of csrc/pps_decimate.hip and in DESIGN.md section 22.  Row v of the adjacency is the entries offsets[v] ..
 * offsets[v + 1] - 1 (offsets int64 [nv + 1]) of nbr int32 [ne] (ascending) and mult int32 [ne]; src int32 [ne] is the row of every entry;
 * row v of the incidence is the entries inc_offsets[v] .. inc_offsets[v + 1] - 1 of inc int32 [ni] (ascending), as topology.adjacency_rows
 * and topology.incidence_rows build them.  A priority is three uint64 compared lexicographically: the bits of the fp64 cost, h(key) and
 * key = (a << 32) | b, h the splitmix64 finaliser of key + 0x9E3779B97F4A7C15; NONE is 2^64 - 1 three times.  All arithmetic is fp64, every
 * operation rounded on its own; one thread per entry, vertex, winner or face; no atomics: each entry is a pure function of its inputs.  A
 * row whose offsets are not 0 <= o0 <= o1 <= the count is taken as empty and an index out of range is skipped; neither is read through.
 *   ppsx_decimate_regular     regular u8 [nv]: 1 when the vertex has a face, every entry of its adjacency row has mult == 2 and its incidence
 *                             row is as long as its adjacency row, else 0.
 *                             nv < 0 or > 2^31 - 1, ne or ni < 0, or -- with nv > 0 -- a NULL offsets, inc_offsets or regular or a NULL mult
 *                             with ne > 0: PPS_ERR_ARG, nothing is launched or written.  nv == 0: 0, nothing is launched.
 *   ppsx_decimate_edges       prio u64 [ne,3], x f64 [ne,3], fell u8 [ne]: for the entry e = (a, b) = (src[e], nbr[e]) with a < b, both ends
 *                             regular, exactly two common entries c, d in the rows of a and b, and not (a face of a holds c and d and a
 *                             face of b holds c and d): the placement x relative to mid = (P_a + P_b) * 0.5 over the faces of a ascending,
 *                             then the faces of b that do not hold a (the quadric, lambda = 1e-3 trace, the cofactor solve; x = 0 and
 *                             fell = 1 when the trace is 0, x is not finite or (x_0^2 + x_1^2) + x_2^2 > |P_b - P_a|^2), the cost = the sum
 *                             of (n . x - m)^2 over the same faces in the same order, and the fold rule (every face that holds one end only
 *                             keeps a positive n . n' with that end at x).  A candidate gets its priority, x and fell; every other entry
 *                             gets NONE, x = 0 and fell = 0.  Every row of the outputs is written.  The formulas are at the top of the
 *                             .hip file.
 *                             nv or nf < 0 or > 2^31 - 1, ne or ni < 0, or -- with ne > 0 -- a NULL nbr, src, prio, x or fell, with nv > 0
 *                             a NULL pos, offsets, inc_offsets or regular, a NULL faces with nf > 0 or a NULL inc with ni > 0: PPS_ERR_ARG,
 *                             nothing is launched or written.  ne == 0: 0, nothing is launched.
 *   ppsx_decimate_vertex_min  m1 u64 [nv,3]: the minimum priority over the entries of row u; the entry (u, v) with u > v is read at its
 *                             mirror, the entry of row v that names u (a binary search; skipped when there is none).  NONE for an empty row.
 *                             nv < 0 or > 2^31 - 1, ne < 0, or -- with nv > 0 -- a NULL offsets or m1 or, with ne > 0, a NULL nbr or prio:
 *                             PPS_ERR_ARG, nothing is launched or written.  nv == 0: 0, nothing is launched.
 *   ppsx_decimate_ring_min    best u64 [nv,3]: the minimum of m1 u64 [nv,3] over w and the entries of row w.
 *                             nv < 0 or > 2^31 - 1, ne < 0, best == m1, or -- with nv > 0 -- a NULL offsets, m1 or best or a NULL nbr with
 *                             ne > 0: PPS_ERR_ARG, nothing is launched or written.  nv == 0: 0, nothing is launched.
 *   ppsx_decimate_winners     flag u8 [ne]: 1 for an entry (a, b), a < b, whose priority is not NONE and equals best[a] and best[b], else 0.
 *                             nv < 0 or > 2^31 - 1, ne < 0, or -- with ne > 0 -- a NULL src, nbr, prio or flag or a NULL best with nv > 0:
 *                             PPS_ERR_ARG, nothing is launched or written.  ne == 0: 0, nothing is launched.
 *   ppsx_decimate_move        for every winner e = win[i] (int64 [nw]) with (a, b) = (src[e], nbr[e]): pos[a] = (pos[a] + pos[b]) * 0.5 +
 *                             x[e] per component and rename[b] = a (rename int32 [nv], the identity before).  The winners of a round share
 *                             no end, so no two threads touch one row.  An e outside [0, ne) or an entry without 0 <= a < b < nv is
 *                             skipped.
 *                             nv or nw < 0 or > 2^31 - 1, ne < 0, or -- with nw > 0 -- a NULL win, with ne > 0 a NULL src, nbr or x, with
 *                             nv > 0 a NULL pos or rename: PPS_ERR_ARG, nothing is launched or written.  nw == 0 (or ne == 0, nv == 0): 0,
 *                             nothing is launched.
 *   ppsx_decimate_rename      out int64 [nf,3], keep u8 [nf]: the face with every index i replaced by rename[i], and keep = 1 when the three
 *                             new indices lie in [0, nv) and are pairwise distinct.  A face with an index outside [0, nv) is copied as it
 *                             is with keep = 0.
 *                             nv or nf < 0 or > 2^31 - 1, or -- with nf > 0 -- a NULL faces, out or keep or a NULL rename with nv > 0:
 *                             PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched. */
int ppsx_decimate_regular(const int64_t* offsets, const int32_t* mult, int64_t ne, const int64_t* inc_offsets, int64_t ni, int64_t nv,
                          uint8_t* regular, void* stream);
int ppsx_decimate_edges(const double* pos, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* nbr,
                        const int32_t* src, int64_t ne, const int64_t* inc_offsets, const int32_t* inc, int64_t ni, const uint8_t* regular,
                        uint64_t* prio, double* x, uint8_t* fell, void* stream);
int ppsx_decimate_vertex_min(const int64_t* offsets, const int32_t* nbr, int64_t ne, int64_t nv, const uint64_t* prio, uint64_t* m1, void* stream);
int ppsx_decimate_ring_min(const int64_t* offsets, const int32_t* nbr, int64_t ne, int64_t nv, const uint64_t* m1, uint64_t* best, void* stream);
int ppsx_decimate_winners(const int32_t* src, const int32_t* nbr, int64_t ne, int64_t nv, const uint64_t* prio, const uint64_t* best, uint8_t* flag,
                          void* stream);
int ppsx_decimate_move(const int64_t* win, int64_t nw, const int32_t* src, const int32_t* nbr, int64_t ne, const double* x, double* pos, int64_t nv,
                       int32_t* rename, void* stream);
int ppsx_decimate_rename(const int64_t* faces, int64_t nf, int64_t nv, const int32_t* rename, int64_t* out, uint8_t* keep, void* stream);

/* ---- isotropic remeshing: short-edge collapse and tangential relaxation (csrc/pps_remesh.hip) ----------------------------------------------
 * new capability: replaces nothing -- the reference has no remeshing, and decimate, flip, subdivide and smooth stay as they are.  Driven by
 * ppsurf_amd/remesh.py; the rules are written out at the top of csrc/pps_remesh.hip and in DESIGN.md section 30.  The rows, the regular
 * vertices and the priorities are those of the decimation above (section 22), and the rest of a collapse round is its entries.  All
 * arithmetic is fp64, every operation rounded on its own; one thread per entry or vertex; no atomics, no LDS, no square root.  A row whose
 * offsets are not 0 <= o0 <= o1 <= the count is taken as empty and an index out of range is skipped; neither is read through.
 *   ppsx_remesh_short_edges  prio u64 [ne,3]: for the entry e = (a, b) = (src[e], nbr[e]) with a < b, both ends regular, exactly two common
 *                            entries c, d in the rows of a and b and not (a face of a holds c and d and a face of b holds c and d):
 *                            len2 = (dx dx + dy dy) + dz dz of P_b - P_a must be < min2; with mid = (P_a + P_b) * 0.5 every face of a, and of
 *                            b without a, that holds one end only must keep a positive n . n' with that end at mid; and every entry w of
 *                            the rows of a and b other than a, b must have |P_w - mid|^2 <= max2 (+inf: no bound).  A candidate gets
 *                            (the bits of len2, h(key), key), every other entry NONE three times.  Every row of prio is written.
 *                            nv, nf or ne < 0 or > 2^31 - 1, ni < 0, min2 or max2 negative or a NaN, or -- with ne > 0 -- a NULL nbr, src
 *                            or prio, with nv > 0 a NULL pos, offsets, inc_offsets or regular, a NULL faces with nf > 0 or a NULL inc
 *                            with ni > 0: PPS_ERR_ARG, nothing is launched or written.  ne == 0: 0, nothing is launched.
 *   ppsx_remesh_relax_pass   y f64 [nv,3], state u8 [nv]: one Jacobi pass over x f64 [nv,3].  A vertex that is not regular is copied
 *                            (state 0).  A regular v: c = the mean of its row (summed ascending from +0.0), d = c - P_v, N = the sum of
 *                            the cross products (P_i1 - P_i0) x (P_i2 - P_i0) of its incidence row (ascending), t = d - N * ((N . d) /
 *                            (N . N)), P' = P_v + lam * t.  Copied with state 2 when N . N is 0 or not finite or a component of t is not
 *                            finite; copied with state 3 when a face of its row, its corners at v replaced by P' and the others as in x,
 *                            does not keep a positive n . n'; else y_v = P' and state 1.  Every row of y and state is written.
 *                            nv or nf < 0 or > 2^31 - 1, ne or ni < 0, lam not in (0, 1], y == x, or -- with nv > 0 -- a NULL x, offsets,
 *                            inc_offsets, regular, y or state, a NULL faces with nf > 0, a NULL nbr with ne > 0 or a NULL inc with
 *                            ni > 0: PPS_ERR_ARG, nothing is launched or written.  nv == 0: 0, nothing is launched. */
int ppsx_remesh_short_edges(const double* pos, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* nbr,
                            const int32_t* src, int64_t ne, const int64_t* inc_offsets, const int32_t* inc, int64_t ni, const uint8_t* regular,
                            double min2, double max2, uint64_t* prio, void* stream);
int ppsx_remesh_relax_pass(const double* x, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* offsets, const int32_t* nbr, int64_t ne,
                           const int64_t* inc_offsets, const int32_t* inc, int64_t ni, const uint8_t* regular, double lam, double* y,
                           uint8_t* state, void* stream);

/* ---- orientation: coherent, outward winding per component (csrc/pps_orient.hip) -----------------------------------------------------------
 * new capability: replaces nothing -- the reference has no such stage and every other stage takes the winding as it comes.  Driven by
 * ppsurf_amd/orient.py (the pairs and their edge slots by ppsurf_amd/topology.py); the rule and what the parity adds to the labelling argument of
 * csrc/pps_labels.h are written out at the top of csrc/pps_orient.hip and in DESIGN.md section 23.  Pairs: fa, fb int32 [np] the two valid faces on an
 * edge that exactly two valid faces hold, ea, eb int32 [np] the slot of that edge in each (slot k is corner k -> corner k + 1 mod 3).
 * word int64 [nf]: (parent << 1) | flip relative to the parent, -1 for an invalid face; word[f] = f << 1 to begin with.  A pair with an entry
 * outside [0, nf), a slot outside [0, 3) or onto a face with a negative word is skipped, never read through.
 *   ppsx_orient_pair_sign   sign u8 [np]: 1 when faces[fa][ea] == faces[fb][eb] (both run the edge the same way: one of them must turn),
 *                           else 0; 0 for a skipped pair.  Every row is written.
 *                           np or nf < 0 or > 2^31 - 1, or -- with np > 0 -- a NULL fa, fb, ea, eb or sign or a NULL faces with nf > 0:
 *                           PPS_ERR_ARG, nothing is launched or written.  np == 0: 0, nothing is launched.
 *   ppsx_orient_hook        one hooking round: a pair walks word from a and from b -- a walk steps from x to its parent p while
 *                           0 <= p < x and XORs the flips -- to the ends (ra, qa), (rb, qb); when ra != rb:
 *                           atomicMin(&word[max(ra, rb)], (min(ra, rb) << 1) | (qa ^ qb ^ sign)) and 1 is stored to *changed (int32, device;
 *                           the caller zeroes it before).  Every word is read by one relaxed device-scope atomic load; no read relies on a
 *                           write of the same launch; see the .hip file.
 *                           np or nf < 0 or > 2^31 - 1, or -- with np > 0 and nf > 0 -- a NULL pointer: PPS_ERR_ARG, nothing is launched or
 *                           written.  np == 0 or nf == 0: 0, nothing is launched.
 *   ppsx_orient_compress    every face f with word[f] >= 0 stores (the end of its walk << 1) | the flip accumulated on it in word[f]; a face
 *                           with a negative word is not touched.  A walk reads no slot outside [0, f] and takes at most f steps.
 *                           nf < 0, nf > 2^31 - 1 or a NULL word with nf > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0,
 *                           nothing is launched.
 *   ppsx_orient_check       after the fixed point (word[f] = (leader << 1) | flip): a pair with (flip[a] ^ flip[b]) != sign stores 1 to
 *                           bad[leader of a] (u8 [nf], zeroed by the caller; the same value from every thread).  Which pairs of a
 *                           non-orientable component fail depends on timing, that one fails does not.
 *                           np or nf < 0 or > 2^31 - 1, or -- with np > 0 and nf > 0 -- a NULL pointer: PPS_ERR_ARG, nothing is launched or
 *                           written.  np == 0 or nf == 0: 0, nothing is launched.
 *   ppsx_orient_block_sums  sums f64 [nb]: block i covers count[i] (int32, 1..256) positions of list int32 [nl] from first[i] (int64), faces
 *                           of one component in ascending index, and lead[i] (int32) is that component's leader.  R = the first corner of
 *                           face lead[i], q_k = double(P_k) - double(R), the term of a face on its corners as given is
 *                           ((q0x (q1y q2z - q1z q2y)) + (q0y (q1z q2x - q1x q2z))) + (q0z (q1x q2y - q1y q2x)), negated when flip[f] (u8 [nf])
 *                           is 1; +0.0 for an absent position, an invalid face or an index out of range.  One wave per block: lane l adds
 *                           the terms of positions 4 l .. 4 l + 3 in order from +0.0, then S[l] = S[l] + S[l + s] for s = 1, 2, 4, 8, 16, 32,
 *                           and lane 0 stores.  fp64, every operation rounded on its own.  A block whose first, count or lead is out of
 *                           range gets +0.0.  Every row is written.
 *                           nb, nl, nv or nf < 0 or > 2^31 - 1, or -- with nb > 0 -- a NULL first, count, lead or sums, a NULL list with
 *                           nl > 0, a NULL faces or flip with nf > 0, a NULL verts with nv > 0: PPS_ERR_ARG, nothing is launched or
 *                           written.  nb == 0: 0, nothing is launched.
 *   ppsx_orient_comp_sums   vol f64 [nc]: the block sums start[c] .. start[c + 1] - 1 (start int64 [nc + 1]) added in ascending order from
 *                           +0.0; +0.0 for a row that is not 0 <= start[c] <= start[c + 1] <= nb.  One thread per component.
 *                           nc or nb < 0 or > 2^31 - 1, or -- with nc > 0 -- a NULL start or vol or a NULL sums with nb > 0: PPS_ERR_ARG,
 *                           nothing is launched or written.  nc == 0: 0, nothing is launched.
 *   ppsx_orient_apply       out int64 [nf,3]: face (a, b, c) as (a, c, b) when cid[f] (int32 [nf]) lies in [0, nc) and turn[cid[f]]
 *                           (u8 [nc]) is 1 with flip[f] == 1 or 2 with flip[f] == 0; every other row is copied as it is.  Every row is written.
 *                           nf or nc < 0 or > 2^31 - 1, out == faces, or -- with nf > 0 -- a NULL faces, cid, flip or out or a NULL turn with
 *                           nc > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched. */
int ppsx_orient_pair_sign(const int64_t* faces, int64_t nf, const int32_t* fa, const int32_t* fb, const int32_t* ea, const int32_t* eb,
                          int64_t np, uint8_t* sign, void* stream);
int ppsx_orient_hook(const int32_t* fa, const int32_t* fb, const uint8_t* sign, int64_t np, int64_t* word, int64_t nf, int32_t* changed,
                     void* stream);
int ppsx_orient_compress(int64_t* word, int64_t nf, void* stream);
int ppsx_orient_check(const int32_t* fa, const int32_t* fb, const uint8_t* sign, int64_t np, const int64_t* word, int64_t nf, uint8_t* bad,
                      void* stream);
int ppsx_orient_block_sums(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const uint8_t* flip, const int32_t* list,
                           int64_t nl, const int64_t* first, const int32_t* count, const int32_t* lead, int64_t nb, double* sums, void* stream);
int ppsx_orient_comp_sums(const double* sums, int64_t nb, const int64_t* start, int64_t nc, double* vol, void* stream);
int ppsx_orient_apply(const int64_t* faces, int64_t nf, const int32_t* cid, const uint8_t* flip, const uint8_t* turn, int64_t nc, int64_t* out,
                      void* stream);

/* ---- weld: coincident and close vertices become one row (csrc/pps_weld.hip) ---------------------------------------------------------------
 * new capability: replaces nothing -- the reference has no such stage, and pps_mesh_corner_weld stays the weld of Marching Cubes in its own
 * grid index space.  Driven by ppsurf_amd/weld.py (the cell lists by trim.SupportGrid: ppsx_trim_cell_slots, a sort, ops.row_offsets; the loop by
 * ppsurf_amd/labels.py); the rule is written out at the top of csrc/pps_weld.hip and in DESIGN.md section 24, the argument for the
 * labelling in csrc/pps_labels.h.  Rows i != j of
 * pts f32 [n,3] are linked when ((dx dx + dy dy) + dz dz) <= eps * eps in fp64 on the widened f32, every operation rounded on its own; a
 * cluster is a connected component of the links and its leader is its smallest row.  lo, hi, h, inv_h, table, capacity, order, offsets are
 * those of ppsx_trim_cell_slots and ppsx_trim_face_support over the same pts; no result depends on them.
 *   ppsx_weld_hook      one hooking round on label int32 [n] (label[v] = v to begin with): vertex i visits the rows j < i of the cells its
 *                       box p_i -+ eps (1 + 2^-20), rounded outward to f32, reaches -- of all rows below i when that range holds more cells
 *                       than n -- and for every linked j walks label from i and from j -- a walk steps from x to label[x] while
 *                       0 <= label[x] < x -- to the ends ri, rj; when ri != rj: atomicMin(&label[max], min), and 1 is stored to *changed
 *                       (int32, device; the caller zeroes it before) when that made the label fall.  A vertex with a negative label
 *                       takes no part: it is skipped as i and as j.  Every label is read by one relaxed device-scope atomic load; no
 *                       read relies on a write of the same launch; see the .hip file.  A label outside [0, x] ends a walk at x, an order
 *                       entry outside [0, i) is skipped and a row of offsets that is not 0 <= o0 <= o1 <= n is taken as empty; none is
 *                       read through.
 *                       n < 0, n > 2^31 - 1, eps negative or NaN, or -- with n > 0 -- a NULL pointer, a capacity that is no power of two
 *                       > n or a grid that make_grid of pps_cells.h refuses: PPS_ERR_ARG, nothing is launched or written.  n == 0: 0,
 *                       nothing is launched.
 *   ppsx_weld_faces     out int64 [nf,3], code u8 [nf] from faces int64 [nf,3] and newrow int64 [nv] (newrow[v] = the output row of v's
 *                       leader).  code 1: the face is invalid as given -- an index outside [0, nv) or two equal indices -- or one of its
 *                       newrow entries lies outside [0, nv); code 2: valid as given and two of its new indices are equal; code 0: kept,
 *                       out = (newrow[a], newrow[b], newrow[c]).  A face with code != 0 gets its row copied as given and an invalid face is
 *                       never read through.  Every row of both outputs is written.
 *                       nf or nv < 0 or > 2^31 - 1, out == faces, or -- with nf > 0 -- a NULL faces, out or code or a NULL newrow with
 *                       nv > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched. */
int ppsx_weld_hook(const float* pts, int64_t n, const float* lo, const float* hi, float h, float inv_h, const uint64_t* table, int64_t capacity,
                   const int64_t* order, const int64_t* offsets, double eps, int32_t* label, int32_t* changed, void* stream);
int ppsx_weld_faces(const int64_t* faces, int64_t nf, int64_t nv, const int64_t* newrow, int64_t* out, uint8_t* code, void* stream);

/* ---- manifold split: many-owner edges and pinched vertices are cut apart by duplicating vertices (csrc/pps_manifold.hip) ------------------
 * new capability: replaces nothing -- the reference has no such stage.  Driven by ppsurf_amd/manifold.py (the pairs and their edge slots
 * by ppsurf_amd/topology.py, the loop by ppsurf_amd/labels.py); the rule and the argument that the result is manifold are written out at the
 * top of csrc/pps_manifold.hip and in DESIGN.md section 25, the argument for the labelling in csrc/pps_labels.h.  Corner c = 3 f + k of a valid face f names the vertex faces[f][k]; label
 * int32 [3 nf] holds one entry per corner, label[c] = c to begin with and -1 for a corner of an invalid face.  The compress launch between
 * two hooks is ppsx_labels_compress(label, 3 nf).
 *   ppsx_manifold_hook   one hooking round over the pairs fa, fb, ea, eb int32 [np] (the two valid faces on an edge that exactly two valid
 *                        faces hold and the slot of that edge in each; slot k is corner k -> corner k + 1 mod 3).  One thread per pair reads
 *                        the four corners of the two slots from faces int64 [nf,3]: when both slots name the same two vertices, the corner
 *                        of fa and the corner of fb that name one end are joined, and likewise for the other end -- slot to slot when both
 *                        faces run the edge the same way, crossed when they run it in opposite ways.  Joining x and y: walk label from x
 *                        and from y -- a walk steps from x to label[x] while 0 <= label[x] < x -- to the ends rx, ry; when rx != ry:
 *                        atomicMin(&label[max], min), and 1 is stored to *changed (int32, device; the caller zeroes it before) when that
 *                        made the label fall.  A pair with a face outside [0, nf), a slot outside [0, 3), a corner vertex outside [0, nv)
 *                        or slots that name no common edge is skipped; a join onto a corner with a negative label is skipped; none is
 *                        read through.  Every label is read by one relaxed device-scope atomic load; no read relies on a write of the
 *                        same launch; see the .hip file.
 *                        nf, nv or np < 0 or > 2^31 - 1, 3 nf > 2^31 - 1, or -- with np > 0 and nf > 0 -- a NULL pointer: PPS_ERR_ARG,
 *                        nothing is launched or written.  np == 0 or nf == 0: 0, nothing is launched.
 *   ppsx_manifold_faces  out int64 [nf,3] from faces int64 [nf,3], label int32 [3 nf] and newrow int64 [3 nf] (newrow[l] = the output row
 *                        of the fan whose leader is corner l): corner c of a face that is valid as given with label[c] >= 0 becomes
 *                        newrow[label[c]], one with a negative label keeps its entry.  A face that is invalid as given -- an index outside
 *                        [0, nv) or two equal indices -- is copied as given and not read through, and so is a face with a label >= 3 nf or
 *                        with a new entry outside [0, nv_out).  Every row of out is written.
 *                        nf, nv or nv_out < 0 or > 2^31 - 1, 3 nf > 2^31 - 1, out == faces, or -- with nf > 0 -- a NULL pointer:
 *                        PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched. */
int ppsx_manifold_hook(const int64_t* faces, int64_t nf, int64_t nv, const int32_t* fa, const int32_t* fb, const int32_t* ea, const int32_t* eb,
                       int64_t np, int32_t* label, int32_t* changed, void* stream);
int ppsx_manifold_faces(const int64_t* faces, int64_t nf, int64_t nv, const int32_t* label, const int64_t* newrow, int64_t nv_out, int64_t* out,
                        void* stream);

/* ---- Delaunay edge flips: the diagonal of a quad turns where that repairs a sliver (csrc/pps_flip.hip) ---------------------------------------
 * new capability: replaces nothing -- the reference has no such stage.  Driven by ppsurf_amd/flip.py (the edges, their owners and slots by
 * ppsurf_amd/topology.py); the rule and the argument that the winners of a round are independent are written out at the top of
 * csrc/pps_flip.hip and in DESIGN.md section 27.  Pairs: fa, fb int32 [np] the two valid faces on an edge that exactly two valid faces hold, in
 * ascending edge key and in either order, ea, eb int32 [np] the slot of that edge in each (slot k is corner k -> corner k + 1 mod 3).  A
 * priority is a u64, the smallest first, NONE = 2^64 - 1.
 *   ppsx_flip_candidates  one thread per pair, on verts f32 [nv,3] and the working faces int64 [nf,3]: with f < g the two faces and k, l
 *                         their slots, a = F[f][k], b = F[f][k + 1], c = F[f][k + 2], d = F[g][l + 2]; the pair is a candidate when
 *                         F[g][l] == b and F[g][l + 1] == a, c != d, the key (min(c, d) << 32) | max(c, d) is none of keys int64 [ne]
 *                         (ascending; a binary search), the fold guard and the crease guard with cos2 pass and the sum s of the two
 *                         opposite cotangents is below -min_gain (fp64, every operation rounded on its own; the .hip file has the formulas).
 *                         Writes prio u64 [np] = ((0x7F800000 - bits(f32(-s))) << 32) | fmix32(pair index) and quad int32 [np,4] =
 *                         (a, b, c, d), NONE and zeros for a pair that is no candidate, and does atomicMin(&vmin[v], prio) on vmin u64 [nv]
 *                         (the caller presets it to all ones) at the four quad vertices of a candidate.  A pair with a face outside [0, nf),
 *                         two equal faces, a slot outside [0, 3) or a face that is not valid for nv is no candidate and is not read through.
 *                         np, nv, nf or ne < 0, np, nv or nf > 2^31 - 1, ne > 3 (2^31 - 1), or -- with np > 0 -- a NULL fa, fb, ea, eb, prio or quad, a NULL
 *                         verts or vmin with nv > 0, a NULL faces with nf > 0 or a NULL keys with ne > 0: PPS_ERR_ARG, nothing is launched
 *                         or written.  np == 0: 0, nothing is launched.
 *   ppsx_flip_winners     flag u8 [np]: 1 when prio[i] != NONE, the four entries of quad[i] lie in [0, nv) and vmin equals prio[i] at all
 *                         four, else 0.  Every flag is written.
 *                         np or nv < 0 or > 2^31 - 1, or -- with np > 0 -- a NULL prio, quad or flag or a NULL vmin with nv > 0:
 *                         PPS_ERR_ARG, nothing is launched or written.  np == 0: 0, nothing is launched.
 *   ppsx_flip_apply       a pair with flag[i] != 0 rewrites two rows of faces int64 [nf,3] in place, with f < g its two faces and
 *                         (a, b, c, d) = quad[i]: F[f] = (a, d, c), F[g] = (b, c, d).  A pair with a face outside [0, nf), two equal faces or
 *                         a quad entry outside [0, nv) writes nothing.  The flagged pairs must share no face (the winners of a round do not).
 *                         np, nv or nf < 0 or > 2^31 - 1, or -- with np > 0 and nf > 0 -- a NULL pointer: PPS_ERR_ARG, nothing is launched
 *                         or written.  np == 0 or nf == 0: 0, nothing is launched. */
int ppsx_flip_candidates(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const int32_t* fa, const int32_t* fb, const int32_t* ea,
                         const int32_t* eb, int64_t np, const int64_t* keys, int64_t ne, double cos2, double min_gain, uint64_t* prio, int32_t* quad,
                         uint64_t* vmin, void* stream);
int ppsx_flip_winners(const uint64_t* prio, const int32_t* quad, int64_t np, const uint64_t* vmin, int64_t nv, uint8_t* flag, void* stream);
int ppsx_flip_apply(const int32_t* fa, const int32_t* fb, const int32_t* quad, const uint8_t* flag, int64_t np, int64_t nv, int64_t* faces, int64_t nf,
                    void* stream);

/* ---- subdivide: edges longer than a bound are split at their midpoint, longest first (csrc/pps_subdivide.hip) -------------------------------
 * new capability: replaces nothing -- the reference has no such stage.  Driven by ppsurf_amd/subdivide.py (the edge runs, their keys and owners
 * by ppsurf_amd/topology.py); the rule and the argument that the winners of a round are independent are written out at the top of
 * csrc/pps_subdivide.hip and in DESIGN.md section 28.  Runs: keys int64 [ne] the distinct edge keys (min << 32) | max in ascending order, the
 * sentinel 2^63 - 1 of the invalid faces last where there is one, owners int64 [ne] the faces on each (0 for the sentinel); run_of
 * int64 [3 nf] the run of key position 3 f + k (slot k of face f is corner k -> corner k + 1 mod 3).  A priority is a u64, the smallest
 * first, NONE = 2^64 - 1.
 *   ppsx_subdivide_edges    one thread per run, on verts f32 [nv,3]: with a < b the two halves of keys[e], d = P_b - P_a in fp64,
 *                           len2[e] = (dx dx + dy dy) + dz dz (f64 [ne]) and M = f32((P_a + P_b) 0.5) per component; the run is a candidate when
 *                           len2 > max2 and M differs from verts[a] and from verts[b] in some component.  prio[e] (u64 [ne]) =
 *                           ((0x7FF00000 - (bits(len2) >> 32)) << 32) | fmix32(e) for a candidate and NONE for every other run.  A key that is
 *                           negative, has a >= b or b >= nv (the sentinel is one) gives len2 0 and NONE and is not read through.  max2 = +inf
 *                           writes the lengths alone.
 *                           ne or nv < 0, ne > 2^32 - 1, nv > 2^31 - 1, a NaN max2, or -- with ne > 0 -- a NULL keys, len2 or prio or a NULL
 *                           verts with nv > 0: PPS_ERR_ARG, nothing is launched or written.  ne == 0: 0, nothing is launched.
 *   ppsx_subdivide_votes    one thread per face: choice[f] (int32 [nf]) = the slot k whose run has the smallest priority, the first of equal
 *                           ones, -1 when all three are NONE; a run_of entry outside [0, ne) counts as NONE and is not read through.  A face
 *                           with a choice adds 1 to votes[run] (int32 [ne], the caller zeroes it before): an integer atomicAdd.
 *                           nf or ne < 0, nf > 2^31 - 1, ne > 2^32 - 1, or -- with nf > 0 -- a NULL run_of or choice or a NULL prio or votes
 *                           with ne > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *   ppsx_subdivide_winners  win[e] (u8 [ne]) = 1 when prio[e] != NONE and votes[e] == owners[e], else 0.  Every flag is written.
 *                           ne < 0 or > 2^32 - 1, or -- with ne > 0 -- a NULL pointer: PPS_ERR_ARG, nothing is launched or written.
 *                           ne == 0: 0, nothing is launched.
 *   ppsx_subdivide_hits     hit[f] (u8 [nf]) = 1 when choice[f] lies in 0..2, the run of that slot lies in [0, ne) and win is set there,
 *                           else 0.  Every flag is written.
 *                           nf or ne < 0, nf > 2^31 - 1, ne > 2^32 - 1, or -- with nf > 0 -- a NULL run_of, choice or hit or a NULL win
 *                           with ne > 0: PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *   ppsx_subdivide_emit     the rows of a round, with vslot int64 [ne] and fslot int64 [nf] the exclusive prefix sums of win and hit and
 *                           nw, nh their totals.  One thread per run: a winner with a readable key and vslot[e] = i in [0, nw) writes
 *                           new_verts[i] (f32 [nw,3]) = M and ends[i] (int64 [nw,2]) = (a, b); the caller appends new_verts to verts.  One
 *                           thread per face: out int64 [nf + nh,3]; a hit face (as ppsx_subdivide_hits finds it again) with i = vslot[run] in
 *                           [0, nw) and j = fslot[f] in [0, nh) writes row f as faces[f] with entry k + 1 mod 3 replaced by nv + i and row
 *                           nf + j as faces[f] with entry k replaced by nv + i; every other row f is copied.  Rows nf .. nf + nh - 1 are
 *                           written by their hits alone.  The entries of a face are never used as an address.
 *                           a negative count, nv, nf, nv + nw or nf + nh > 2^31 - 1, ne > 2^32 - 1, nw > ne, nh > nf, out == faces, or --
 *                           with ne > 0 -- a NULL keys, win or vslot, a NULL verts with nv > 0, a NULL new_verts or ends with nw > 0, or
 *                           -- with nf > 0 -- a NULL faces, run_of, choice, hit, fslot or out: PPS_ERR_ARG, nothing is launched or written.
 *                           ne == 0 and nf == 0: 0, nothing is launched. */
int ppsx_subdivide_edges(const int64_t* keys, int64_t ne, const float* verts, int64_t nv, double max2, double* len2, uint64_t* prio, void* stream);
int ppsx_subdivide_votes(const int64_t* run_of, int64_t nf, const uint64_t* prio, int64_t ne, int32_t* choice, int32_t* votes, void* stream);
int ppsx_subdivide_winners(const uint64_t* prio, const int32_t* votes, const int64_t* owners, int64_t ne, uint8_t* win, void* stream);
int ppsx_subdivide_hits(const int64_t* run_of, const int32_t* choice, int64_t nf, const uint8_t* win, int64_t ne, uint8_t* hit, void* stream);
int ppsx_subdivide_emit(const float* verts, int64_t nv, const int64_t* keys, const uint8_t* win, const int64_t* vslot, int64_t ne, int64_t nw,
                        const int64_t* faces, int64_t nf, const int64_t* run_of, const int32_t* choice, const uint8_t* hit, const int64_t* fslot,
                        int64_t nh, float* new_verts, int64_t* ends, int64_t* out, void* stream);

/* ---- intersect: which pairs of faces of a mesh cross (csrc/pps_intersect.hip) ------------------------------------------------------------------
 * new capability: replaces nothing -- the reference has no such check.  Driven by ppsurf_amd/intersect.py (the cell lists by trim.SupportGrid over
 * the box lower corners of the small faces); the rule -- live faces, boxed pairs, the admitted edge-against-triangle tests in fp64 -- and the
 * argument that the cell range misses no partner are written out at the top of csrc/pps_intersect.hip and in DESIGN.md section 29; restated in
 * numpy by tests/intersect_spec.py, which the entries match bit for bit.  No result depends on h, on the capacity, on which live face is in
 * `small` and which in `large`, or on the order in which the partners are met.
 *   ppsx_intersect_boxes  one thread per face of verts f32 [nv,3] / faces int64 [nf,3]: live[f] (u8 [nf]) = 1 when the face is valid for nv
 *                         (indices in [0, nv), pairwise distinct) and its nine coordinates are finite; lo, hi (f32 [nf,3]) the box of its three
 *                         corners; ext[f] (f32 [nf]) the largest of the three fp64 differences hi - lo, rounded up to f32 (+inf above the
 *                         largest float).  A face that is not live is not read through and gets zeros in all four.
 *                         nf or nv < 0 or > 2^31 - 1, or -- with nf > 0 -- a NULL faces, lo, hi, ext or live or a NULL verts with nv > 0:
 *                         PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *   ppsx_intersect_count  one wave per face f, four faces per workgroup, with lo, hi, live from ppsx_intersect_boxes.  Partners: small int64 [ns]
 *                         lists faces with ext <= h, whose box lower corners (in that order) are the ns points of the cell lists glo, ghi, h,
 *                         inv_h, table, capacity, order, offsets (those of ppsx_trim_cell_slots and ppsx_trim_face_support, over n = ns
 *                         points); large int64 [nl] lists further faces, of any extent; no face is listed twice.  Every listed g != f that
 *                         is live and in [0, nf) is met exactly once when its box overlaps f's.  flag[f] (u8 [nf]) = 1 when some partner
 *                         crosses f; count[f] (int32 [nf]) = the crossing partners g > f; boxed[f] (int32 [nf]) = the boxed partners g > f.
 *                         A face that is not live gets zeros.  An entry of order, offsets, small, large or faces that is out of range is
 *                         skipped, never used as an address.
 *                         a negative count, nf or nv > 2^31 - 1, ns + nl > nf, h < 0 or NaN, or -- with nf > 0 -- a NULL faces, lo, hi,
 *                         live, flag, count or boxed, a NULL verts with nv > 0, a NULL large with nl > 0, or -- with ns > 0 -- a NULL
 *                         small, table, order or offsets, a capacity that is no power of two > ns, or a grid that pps_cells.h refuses
 *                         (h == 0 among them): PPS_ERR_ARG, nothing is launched or written.  nf == 0: 0, nothing is launched.
 *   ppsx_intersect_emit   the same walk with count from ppsx_intersect_count and pair_offsets int64 [nf] its exclusive prefix sum: the crossing
 *                         pair (f, g), g > f, goes to row pair_offsets[f] + p of pairs int64 [np,2], p its position among the pairs of f in
 *                         the order of the walk (a ballot prefix); the caller sorts the rows.  A pair is written only while p < count[f], and
 *                         a face with count[f] <= 0, pair_offsets[f] < 0 or pair_offsets[f] + count[f] > np writes nothing.
 *                         the rules of ppsx_intersect_count, and np < 0, a NULL count or pair_offsets, a NULL pairs with np > 0: PPS_ERR_ARG,
 *                         nothing is launched or written.  nf == 0 or np == 0: 0, nothing is launched. */
int ppsx_intersect_boxes(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, float* lo, float* hi, float* ext, uint8_t* live,
                         void* stream);
int ppsx_intersect_count(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* lo, const float* hi, const uint8_t* live,
                         const int64_t* small, int64_t ns, const float* glo, const float* ghi, float h, float inv_h, const uint64_t* table,
                         int64_t capacity, const int64_t* order, const int64_t* offsets, const int64_t* large, int64_t nl, uint8_t* flag,
                         int32_t* count, int32_t* boxed, void* stream);
int ppsx_intersect_emit(const float* verts, int64_t nv, const int64_t* faces, int64_t nf, const float* lo, const float* hi, const uint8_t* live,
                        const int64_t* small, int64_t ns, const float* glo, const float* ghi, float h, float inv_h, const uint64_t* table,
                        int64_t capacity, const int64_t* order, const int64_t* offsets, const int64_t* large, int64_t nl, const int32_t* count,
                        const int64_t* pair_offsets, int64_t np, int64_t* pairs, void* stream);

/* ---- tile claims of the split-precision decoder (csrc/pps_decode.hip, csrc/pps_common.h) ---------------------------------------------------------
 * changes no entry: inside pps_decode_fwd_mixed_f32 the persistent split-precision kernels take their next unit of work from counters in the
 * head of the workspace `ws` instead of walking a fixed share of the units.  int32 words of that head: [0] range flag, [1] fall-back count (as
 * before), [2] workgroups of the kernel in flight that are done, [3..10] the interpolation kernel's counters (one per XCD range), [11] STN rows,
 * [12] STN head, [13] fc3 + feature rows, [14] tail.  The caller zeroes the head once, as before; every kernel leaves words 2..14 at zero.  The
 * single entries (pps_interp_pool_f16x3, pps_pointnet_f16x3, pps_decode_tail_f16x3) keep the fixed share.  A query's results do not depend on
 * the unit or the workgroup that evaluates it.  Environment, read per call: PPS_TILE_CLAIMS=0 keeps the fixed share everywhere; a number selects
 * kernels by bit (1 interpolation, 2 STN rows, 4 STN head, 8 fc3 + feature rows, 16 tail).  PPS_INTERP_AHEAD=0 (here and in pps_interp_pool_f16x3)
 * lets every trip of the fixed-share interpolation kernel fetch its own neighbour ids and G rows instead of one trip ahead: same bits.
 *   ppsx_decode_units  HOST function, launches nothing; units, count are HOST pointers.  Lists the units of kernel 0 interp_pool_f16x3,
 *                      1 pointnet_stn_rows (split precision, one launch), 2 pointnet_stn_head_h, 3 pointnet_fc3_feat_rows, 4 decode_tail_h for
 *                      q queries with patches of p points on a chip that holds wgs workgroups of that kernel, in the order the counters hand
 *                      them out, computed by the functions the kernels call: units int64 [capacity,3] = (first query, query count, mode);
 *                      mode is patch_packing's for STN rows (1: packed wave groups, only among the queries below the split point, which is
 *                      the whole rounds over wgs workgroups; 2: the packed arithmetic, one query per wave; 0: padded tiles) and 0 elsewhere.
 *                      *count = the number of units; at most `capacity` of them are written.
 *                      kernel outside 0..4, q < 0, p < 1, wgs < 1, capacity < 0, count NULL, or units NULL with capacity > 0: PPS_ERR_ARG. */
int ppsx_decode_units(int kernel, int64_t q, int p, int wgs, int64_t* units, int64_t capacity, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* PPSURF_AMD_EXT_H */
