// Shared between sas_kernels.hip, sas_tile.hip, sas_mesh.hip, sas_query.hip, sas_match.hip, sas_cloud.hip, sas_fuse.hip, sas_grad.hip, sas_fit.hip, sas_loss.hip, sas_density.hip, sas_mcmc.hip, sas_order.hip, sas_knn.hip, sas_skin.hip (device code + launchers: through sas_device.h) and sas_api.cpp (context, C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define SAS_TILE 16
// record / colour strides in float4: a 32-byte record and a colour array of its own.  (Measured against the colour inside a
// 48-byte record as rounds 1-4 had it, the two roles of the projection each writing part of every line: projection +5 us, tile
// kernel +1.5 us, pair bench -5 %: profiles/r05_ab_record_layout.txt.)
#define SAS_RS 2
#define SAS_CS 1
#define SAS_MAX_GROUP 4   // views per launch group (SasMulti)

// Per-frame camera constants, computed on the host with the same f32 operations the oracle uses.
struct SasCam {
    float R[9], t[3];
    float campos[3];
    float fx, fy, cx, cy;
    float lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg;
    float Wf, Hf;
    int W, H, tw, th;      // tw x th tiles of tile_px pixels
    int tile_px;           // SAS_TILE; 8 in the quad layout, whose 8x8 quadrants are binned as tiles of their own
};

// Scene in HBM.  At upload the Gaussians are re-ordered along a 3-D Hilbert curve (per splat
// group) so that the 256 Gaussians of one workgroup project to a compact screen window, and
// re-laid out into 16-byte planes so that lane i of a wave reads
// bytes [16 i, 16 i + 16) of every plane: each wave-instruction is one contiguous 1 KiB.
//   g0[n] = (mean.x, mean.y, mean.z, opacity)
//   g1[n] = quat wxyz                     | cov xx xy xz yy
//   g2[n] = (scale.x, scale.y, scale.z, group id bits) | (cov yz, cov zz, 0, group id bits)
//   col[p*n_pad + n] = floats 4p..4p+3 of the Gaussian's flattened [K,3] coefficient block
struct SasScene {
    const float4 *g0, *g1, *g2, *col;
    const uint8_t *gid8;    // [n_pad] group id per slot once more, one byte each: the projection's colour role needs only that of g2
    const int *perm;        // [n] slot j holds the caller's Gaussian perm[j] (Hilbert order, by group)
    int64_t n;
    int64_t n_pad;     // plane stride
    int sh_degree;     // -1: col plane 0 holds final rgb
    int cov_mode;      // 1: g1/g2 hold a covariance
    int n_groups;      // 0: no splat groups (the poses themselves belong to a frame: SasFrame::group_Rt)
};

// Per-frame scratch owned by the context.
//   rec[2n..2n+1]  projected record of Gaussian n, 32 B, written by the projection's GEOMETRY role:
//        (mean2d.x, mean2d.y, conic.a, conic.b) (conic.c, opacity, skip_threshold, depth)
//   col[n]         (r, g, b, -), 16 B, written by the projection's COLOUR role (round 5: the two roles are different
//                  workgroups of one launch, so the colour has an array of its own -- every store instruction of either
//                  role covers whole cache lines)
//   info[n]        (x0 | x1<<16, y0 | y1<<16, radius x, radius y): tile rectangle and radii (parity hook), 0 if culled
//   stats          device counters: [5] workgroups whose screen window did not fit the LDS histogram (direct atomics),
//                  reset by the projection's tail
//   tickets        [65 * 32] words: 64 sub-tickets (one cache line each) + the master ticket of the projection's
//                  workgroups (who is last?); each is reset by its last taker
//   stats_host     PINNED host words the frame reports through, written by the projection's tail (no copy at the
//                  end of a frame): [0] n_visible [1] keys written (= n_isect at 16-pixel binning) [2] overflow [3] n_isect of the contract's 16-pixel
//                  tiles (quad layout) [4] max tile length [5] window misses;
//                  [6] tiles the lazy kernel had to order completely (one depth bucket > chunk): zeroed by the tail,
//                  counted by the tile kernel with a system-scope atomic (rare)
// INVARIANT: tile_count[] and tile_big[] are all zero between frames -- the tile kernel (k_blend on the full path)
// clears the counts of the tile it has just rendered, so a frame needs no memset in front of its projection.
// SINGLE-PASS BINNING (seg > 0; round 4, the product path): every tile owns a segment of `seg` keys at keys + tile * seg
// (HBM is plentiful: 1.6 GB per slot at config 3), so a key's place is known the moment its tile's count atomic returns
// -- the projection emits the keys itself: there is no scatter kernel, no wg_base, no offset scan.  A tile longer than
// `seg` sets the overflow flag (the projection's tail sees the counts); the frame is then rendered again with larger
// segments, like a frame that outgrew `cap` on the two-pass path below.
// TWO-PASS binning (seg == 0: SAS_FULL_SORT frames -- their lists are compact, the parity hooks read them -- and frames whose
// segments would not fit the memory budget), by RESERVATION:
// a projection workgroup counts its intersections per tile in an LDS window and adds each
// window bin to tile_count with ONE returning atomic; what it gets back -- where its run starts inside the tile's
// segment -- goes to wg_base[workgroup][bin].  k_scatter (same workgroups, same windows) then needs no global atomic
// and no counting pass: position = tile_offset + wg_base + rank in LDS.  Gaussians outside the window scheme (large
// rectangles) count into tile_big with one atomic per intersection and are placed behind the tile's window runs
// through tile_cursor, as before.
struct SasFrame {
    float4 *rec;
    float4 *col;
    uint4 *info;
    int *tile_count;   // [tiles] window intersections per tile (+ zero padding the tail's 16-byte loads may touch)
    int *tile_big;     // [tiles] per-intersection counts of Gaussians outside the window scheme (same padding)
    int *wg_base;      // [n_wg * SAS_WIN_BINS] start of each projection workgroup's run inside its tiles' segments
    int *class_cursor; // [16] next free position in tile_order per list-length class (descending), set by the projection's tail
    int *tile_offset;  // [tiles+1]
    int *tile_cursor;  // [tiles] next free position for a tile's `big` entries: starts at tile_offset + tile_count
    int *tile_order;   // [tiles] tiles by descending list-length class (blend launch order)
    int *sort_class;   // [6] starts of the large / mid / small sort class in tile_order, tiles; then {0, tiles}
    unsigned long long *keys;  // [cap]  depth bits << 32 | storage slot
    int *sorted_ids;           // [cap]  storage slots, per tile, front to back
    long long cap;
    int seg;                   // > 0: single-pass binning, tile t's keys (and ids) live at [t * seg, t * seg + count); cap = tiles * seg
    int cull;                  // (single-pass binning only) 1: tiles of its rectangle a Gaussian cannot reach are left out of the lists
    int group_fill;            // 1 (frames that share the chip with others: SAS_ASYNC, batches): ONE workgroup paints the four tiles of an all-empty tile group;
                               // 0 (a blocking frame alone on the GPU): every tile has its own workgroup -- the kernel's end is shorter, its slot time larger
    int keep_info;             // 1: the geometry role writes info[] (two-pass frames: k_scatter reads it; the parity hook; -DSAS_TUNE_STATS builds).
                               // Single-pass product frames skip it: nothing on the device reads it, 16 B per Gaussian less to write
    unsigned *stats;           // [8] device counters
    unsigned *tickets;         // [65 * 32]
    unsigned *stats_host;      // [8] pinned
    int *wg_vis;               // [ceil(n/256)] visible Gaussians per projection workgroup
    int *wg_isect16;           // quad layout (8-pixel binning) only, else nullptr: [ceil(n/256)] intersections with the 16-pixel
                               // tiles of the contract per projection workgroup (the n_isect the frame reports)
    unsigned *tile_max;        // [tiles] per-tile max expected depth (bits), written when depth is filled
    const float *group_Rt;     // [n_groups,12] poses of the splat groups for THIS view (device), or nullptr
    const float *group_host;   // the same rows on the host (the slot's pinned snapshot): small pose blocks ride in the
                               // projection's argument segment instead of being uploaded (sas_poses_inline)
    int n_wg;
    int n_tiles;               // tw * th
};

struct SasOutputs {
    float *rgb, *alpha, *depth;
    uint8_t *rgb8;
    // uint8 frame wanted in PINNED HOST memory and every tile complete (W, H multiples of 16): the tile kernel packs its
    // tile's rows in LDS and stores them to the host itself (16 bytes per lane; 8 in the quad layout), tile by tile while
    // the kernel runs -- no device staging frame, no copy kernel behind the frame.  nullptr otherwise.
    uint8_t *rgb8_host;
    float bg[3];
    // RGB-D tail (sas_render_rgbd): camera-frame points [H,W,3] and depth mask [H,W], or nullptr
    float *points;
    uint8_t *mask;
    float max_depth;      // mask = depth < max_depth when use_max_depth, else all ones
    int use_max_depth;
    long long n_pixels;   // W * H
};

// Per-frame parameters.  They travel in the ARGUMENT SEGMENT of every kernel of the frame (scalar loads, no
// upload in front of the frame).
struct SasParams {
    SasCam cam;
    SasOutputs out;
};

// Up to SAS_MAX_GROUP same-sized views rendered by ONE set of launches: the cameras of a Gym step.  Passed to the
// *_multi kernels by value.
constexpr int kMultiInlineRows = 32;   // pose rows (all views together) a launch group carries in its argument segment
constexpr int kProjInlineRows = 16;    // ... a single view / a view pair
struct SasMulti {
    SasFrame f[SAS_MAX_GROUP];
    SasParams P[SAS_MAX_GROUP];
    int nv;
    int mix_k;                                  // geometry blocks per 8 leading blocks of the projection launch (set by the launcher)
    int pose_inline;                            // 1: view k's poses are pose_rows + pose_off[k] (set by the launcher)
    int pose_off[SAS_MAX_GROUP];
    float pose_rows[12 * kMultiInlineRows];
};
// Will the projection launch carry the poses itself (no upload kernel, no dependent-kernel gap in front of it)?
static inline bool sas_poses_inline(int n_groups, int n_views, bool multi)
{
    return n_groups > 0 && (multi ? n_groups * n_views <= kMultiInlineRows : n_groups <= kProjInlineRows);
}

// Group poses of the views of a launch: ONE small kernel copies each view's [rows, 12] block into that view's device
// buffer -- from its own argument segment when the rows of all views fit (SAS_POSE_INLINE_ROWS), else from PINNED
// host memory.  Frames of scenes without splat groups have no prologue at all.
#define SAS_POSE_INLINE_ROWS 64
struct SasPoseUpload {
    int nv;
    float *dst[SAS_MAX_GROUP];
    const float *src_host[SAS_MAX_GROUP];   // pinned
    int floats[SAS_MAX_GROUP];              // 12 * rows of view k
};
void sas_launch_pose_upload(hipStream_t st, const SasPoseUpload &u);

// Frames wanted on the host (sas_render_batch_host, pinned destination): copied by a kernel behind the tile kernel,
// host_bytes each -- a runtime copy between two kernels costs two switches between the compute queue and a copy
// engine, longer than the copy.
struct SasHostCopy {
    int nv;
    const uint8_t *src[SAS_MAX_GROUP];
    uint8_t *dst[SAS_MAX_GROUP];
    size_t bytes;
};
void sas_launch_host_copy(hipStream_t st, const SasHostCopy &h);

// Per-Gaussian feature channels (sas_scene_features / sas_render_features; DESIGN.md 3, "Feature channels").
// The store is [chunks][n_pad][SAS_FEAT_K] float32 in slot order, channels c >= C zero; k_blend_features composites one chunk
// of SAS_FEAT_K channels per workgroup, from the complete lists a SAS_FULL_SORT frame keeps, through the frame's own compositing
// loop (blend_range) with the chunk's channels in the colours' place.
#define SAS_FEAT_K 8
#define SAS_MAX_FEATURES 256
struct SasFeatures {
    const float *store;   // [chunks][n_pad][SAS_FEAT_K]
    float *out;           // [H,W,C] device
    long long n_pad;
    int C, chunks;
    float bg[SAS_MAX_FEATURES];   // feature background, [C] (rest zero)
};
static inline int sas_feature_chunks(int C) { return (C + SAS_FEAT_K - 1) / SAS_FEAT_K; }
// store <- features [n,C] of the caller's order (device; nullptr: one-hot of gid8 with C = n_groups), through perm, finite_colour
void sas_launch_feature_store(hipStream_t st, int64_t n, int64_t n_pad, const int *perm, const uint8_t *gid8, const float *src,
                              int C, float *store);
// after sas_launch_blend, on the same frame: the features of every pixel, one workgroup per (tile, chunk)
// ... of a frame with meshes (sas_scene_mesh_features): what k_blend_mesh_scene resolved per pixel, and the per-triangle rows that take the
// feature background's place where a triangle shows
struct SasMeshFeatures {
    const unsigned long long *win;   // [H W] (depth bits << 32 | record) of the pixel's triangle, ~0: none (SasMeshExtra::win)
    const float *store;              // [chunks][nt][SAS_FEAT_K]
    long long nt;
};
// MF: nullptr for a frame without meshes
void sas_launch_blend_features(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f,
                               const SasFeatures &F, bool fast_exp, const SasMeshFeatures *MF);
// Label frames (sas_render_batch_labels; DESIGN.md 3, "Label frames"): the argmax over the channels of what sas_launch_blend_features
// would write with a zero feature background, kept per pixel as one byte.  One workgroup per tile walks the chunks of the store.
struct SasLabels {
    const float *store;   // [chunks][n_pad][SAS_FEAT_K]: the one-hot group store
    long long n_pad;
    int C, chunks;
    uint8_t *out;         // [H,W] device
    float min_alpha;      // 255 where alpha < min_alpha
    int surface;          // SAS_MESH_SURFACE: alpha of a pixel that shows a triangle is 1
};
// after sas_launch_blend / sas_launch_blend_mesh (whose SasMeshExtra::win MF names), on the same frame; MF: nullptr without meshes
void sas_launch_blend_labels(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f, const SasLabels &B,
                             bool fast_exp, const SasMeshFeatures *MF);
// Label lifting (sas_lift_labels; DESIGN.md 3, "Label lifting"): the transpose of a label frame.  Every weight the frame's
// compositing adds at a pixel goes, as q = floor(weight 2^32), to the entry's Gaussian (caller's index perm[slot]): seen[i] += q and,
// where the pixel's label is below n_labels, votes[i, label] += q.  64-bit integer atomics: the sums do not depend on their order.
struct SasLift {
    const uint8_t *labels;        // [H,W] device: the view's label image
    unsigned long long *votes;    // [n,n_labels] device (the caller's int64), or nullptr
    unsigned long long *seen;     // [n] device, or nullptr
    long long n;                  // Gaussians of the scene
    int n_labels;                 // 1..256
};
// after sas_launch_blend, on the same frame (no meshes): one workgroup per tile
void sas_launch_lift_labels(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f, const SasLift &B,
                            bool fast_exp);
// Feature lifting (sas_lift_features; DESIGN.md 3, "Feature lifting"): sas_lift_labels with C real-valued channels in one label's
// place.  Every weight the frame's compositing adds at a pixel goes, as q = floor(weight 2^24), to the entry's Gaussian: weight[i] += q
// and sums[i,k] += q fq[p,k], fq the pixel's channels quantised to [-32767, 32767] by `scale`.  64-bit integer atomics as there.
struct SasLiftFeatures {
    const float *images;          // [H,W,C] device: the view's feature image
    const uint8_t *mask;          // [H,W] device, or nullptr: a pixel with mask 0 adds nothing
    unsigned long long *sums;     // [n,C] device (the caller's int64, two's complement), or nullptr
    unsigned long long *weight;   // [n] device, or nullptr
    long long n;                  // Gaussians of the scene
    int C;                        // 1..SAS_MAX_FEATURES
    float scale;                  // feature_scale
};
// after sas_launch_blend, on the same frame (no meshes): one workgroup per (tile, chunk of SAS_FEAT_K channels)
void sas_launch_lift_features(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f,
                              const SasLiftFeatures &B, bool fast_exp);
// Backward pass (sas_render_backward_screen; DESIGN.md 3, "Backward pass"): the derivative of a frame's raw accumulators with respect to
// what the projection staged per Gaussian.  Every output is float32 in the caller's Gaussian order and is ADDED to (float atomics).
struct SasGrad {
    const float *g_rgb;      // [H,W,3] device, or nullptr: gradient of sum c alpha T
    const float *g_alpha;    // [H,W] or nullptr: of 1 - T_final
    const float *g_depth;    // [H,W] or nullptr: of sum z alpha T
    float *d_means2d;        // [n,2] or nullptr
    float *d_conics;         // [n,3] (a, b, c) or nullptr
    float *d_opacities;      // [n] or nullptr
    float *d_colors;         // [n,3] or nullptr
    float *d_depths;         // [n] or nullptr
    long long n;             // Gaussians of the scene
};
// after sas_launch_blend, on the same frame (no meshes): one workgroup per tile (sas_grad.hip)
void sas_launch_grad_tiles(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f, const SasGrad &B,
                           bool fast_exp);
// ... and the chain through the view's projection (sas_render_backward): from the screen-space sums of sas_launch_grad_tiles (s_*, all
// five required, the caller's order) to the uploaded arrays and the view matrix.  Every output is ADDED to and may be nullptr.
struct SasGradProj {
    const float *s_means2d, *s_conics, *s_opacities, *s_colors, *s_depths;
    float *d_means;          // [n,3]
    float *d_opacities;      // [n]
    float *d_sh;             // [n,(L+1)^2,3]; [n,3] for a scene of plain colours
    float *d_quats;          // [n,4]  (scenes uploaded as quaternion and scale)
    float *d_scales;         // [n,3]
    float *d_cov6;           // [n,6]  (scenes uploaded as covariances)
    float *partial;          // [ceil(n / 256)][12] scratch: one row per workgroup, or nullptr: no view-matrix gradient
    float *d_viewmat;        // [3,4] rows [R | t] (with partial)
    long long n;
};
// ... and to the poses of up to SAS_MAX_POSE_GRAD_GROUPS selected groups (sas_render_backward_poses): slot q of the selection is group
// (ids[q / 4] >> 8 (q % 4)) & 255.  n_sel == 0: no pose gradient, the other fields are not read.
#ifndef SAS_MAX_POSE_GRAD_GROUPS
#define SAS_MAX_POSE_GRAD_GROUPS 32   // (include/sim_a_splat_amd.h)
#endif
struct SasPoseSel {
    int n_sel;
    unsigned ids[SAS_MAX_POSE_GRAD_GROUPS / 4];
    float *partial;          // [ceil(n / 256)][n_sel][12] scratch: one row per (workgroup, slot)
    float *d_group_poses;    // [n_sel,12] rows [R | t], in the selection's order
};
// behind sas_launch_grad_tiles on the same frame, which keeps its info records and has its group poses on the device
void sas_launch_grad_project(hipStream_t st, const SasScene &s, const SasParams &P, const SasFrame &f, const SasGradProj &B,
                             const SasPoseSel &S);
// store <- features [nt,C] (device; nullptr: one-hot of the triangles' pose groups), through finite_colour
void sas_launch_mesh_feature_store(hipStream_t st, int64_t nt, const int4 *tri, const float *src, int C, float *store);

// launchers (sas_kernels.hip)
void sas_launch_relayout(hipStream_t st, int64_t n, int64_t n_pad, const int *perm, const float *means, const float *quats,
                         const float *scales, const float *cov6, const float *opac, const float *colors,
                         int coeff_floats, int planes, const uint8_t *gid, float4 *g0, float4 *g1, float4 *g2,
                         float4 *col, uint8_t *gid8);
// The projection's LAST workgroup to finish also scans the tile counts (offsets, scatter cursors, tile order,
// statistics to stats_host) and resets the ticket: there is no scan kernel.
void sas_launch_project(hipStream_t st, const SasScene &s, const SasParams &P, const SasFrame &f);
// two views of the scene in one pass over the Gaussians (same scene and group poses, same image grid not required)
void sas_launch_project2(hipStream_t st, const SasScene &s, const SasParams &P0, const SasFrame &f0, const SasParams &P1,
                         const SasFrame &f1);
// one launch for all views of a group (same image size): project (one pass over the scene per view), scatter,
// lazy tile kernel
void sas_launch_project_multi(hipStream_t st, const SasScene &s, const SasMulti &mf);
void sas_launch_scatter_multi(hipStream_t st, const SasScene &s, int tw, const SasMulti &mf);
void sas_launch_tiles_lazy_multi(hipStream_t st, const SasScene &s, int tiles, const SasMulti &mf, bool fast_exp, bool want_max,
                                 bool quad, hipEvent_t ev_start, hipEvent_t ev_stop);
void sas_launch_scatter(hipStream_t st, const SasScene &s, int tw, const SasFrame &f);
struct SasSortStreams {
    hipStream_t side[2];   // nullptr: run the classes back to back on the frame's stream
    hipEvent_t fork, join[2];
};
void sas_launch_sort(hipStream_t st, const SasScene &s, int tiles, const SasFrame &f, const SasSortStreams &ss);
void sas_launch_blend(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f,
                      bool fast_exp, bool want_max);
// ev_start/ev_stop (optional): stamped with the kernel's own begin/end (hipExtLaunchKernelGGL).
// quad: the frame was projected and binned in 8-pixel tiles (SasCam::tile_px == 8; `tiles` counts those): one workgroup
// per 8x8 quadrant of a 16-pixel tile (small frames; sas_tiles_lazy_quad_ok says whether the build has that layout for
// the requested exponential).
bool sas_tiles_lazy_quad_ok(bool fast_exp);
void sas_launch_tiles_lazy(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f,
                           bool fast_exp, bool want_max, bool quad, hipEvent_t ev_start, hipEvent_t ev_stop);
// depth tail: fill depth where nothing was composited (fill) and/or unproject it (points)
void sas_launch_depth_tail(hipStream_t st, int tiles, const SasParams &P, const SasFrame &f, bool fill, bool points);
// size in ints of a frame's counter block ([8 statistics words][tile counts + zero padding]) and of one of the
// three per-tile int arrays of `tilebuf` (offsets, cursors, order; 16-byte aligned strides)
#define SAS_TICKET_INTS (65 * 32)
#define SAS_WIN_BINS 2048   // bins of a binning workgroup's LDS window (8 KiB)
static inline size_t sas_count_stride(int tiles) { return (((size_t)tiles + 1 + 1023) & ~(size_t)1023) + 1024; }
// [tickets][8 statistics words + 16 class cursors + 8 pad][tile_count][tile_big]
static inline size_t sas_counter_ints(int tiles) { return SAS_TICKET_INTS + 32 + 2 * sas_count_stride(tiles); }
static inline size_t sas_tile_stride(int tiles) { return ((size_t)tiles + 1 + 3) & ~(size_t)3; }

// Triangle meshes (sas_scene_meshes; DESIGN.md 3, "Meshes").  A frame of a context that holds meshes is a SAS_FULL_SORT frame
// plus three launches in front of its k_blend: k_mesh_setup (one thread per triangle: pose, view, near clip at kNear, shading,
// screen-space records, per-tile counts), k_mesh_scan (offsets; overflow of the list capacity to the pinned status words) and
// k_mesh_scatter (record indices into per-tile lists).  k_blend_mesh then resolves every pixel's nearest triangle in its tile
// prologue and composites the splats in front of it.
// A record (4 float4 per clipped triangle, 2 per triangle: a triangle crossing the near plane leaves at most two):
//   [0] (a0, b0, c0, a1) [1] (b1, c1, a2, b2) [2] (c2, za, zb, zc) [3] (r, g, b, -)
// edge i: E_i(x, y) = a_i x + b_i y + c_i > 0 inside (ties: a_i > 0, or a_i == 0 and b_i > 0; (a_i, b_i) a unit vector),
// 1/z = za x + zb y + zc, at the pixel centre (x + 0.5, y + 0.5) taken relative to the image centre (W/2, H/2).  Its tile rectangle is kept beside it (x0, y0, x1, y1; x0 > x1: no record).
struct SasMeshScene {
    const float4 *vert;     // [nv] mesh-local vertices (x, y, z, 0), the handle's scale applied
    const int4 *tri;        // [nt] (i0, i1, i2, pose group)
    const float4 *color;    // [nt] (r, g, b, 0)
    int nv, nt;
    int n_groups;           // the scene's (0: no splat groups, every triangle unposed)
    float ka, kd;
    // vertex attributes (sas_scene_mesh_vertex_attributes; DESIGN.md 3, "Meshes", rule 2b), nullptr: none
    const float4 *vnormal;  // [nv] mesh-local unit normals (x, y, z, 0); zero: the vertex has none
    const float4 *vcolor;   // [nv] (r, g, b, 0), or nullptr: a smooth triangle takes color[t] at its three vertices
};
struct SasMeshFrame {
    float4 *rec;            // [2 nt * 4]
    int4 *rect;             // [2 nt]
    int *tile_count;        // [tiles] zeroed in front of the setup
    int *tile_offset;       // [tiles + 1]
    int *tile_cursor;       // [tiles]
    int *list;              // [cap]
    long long cap;
    int n_rec;              // 2 nt
    unsigned *status_host;  // pinned [2]: [0] entries the lists needed, [1] 1 when that exceeds cap
};
// What a mesh frame with a features output and / or SAS_MESH_SURFACE asks of its blend kernel beyond the frame (k_blend_mesh_scene;
// plain mesh frames run k_blend_mesh, which knows neither)
struct SasMeshExtra {
    unsigned long long *win;   // feature frames: [H W] every pixel's (depth bits << 32 | record), ~0: none, for k_blend_features_mesh; else nullptr
    int surface;               // SAS_MESH_SURFACE: alpha / depth of a covered pixel close on the triangle
};
// Attribute planes of a frame whose meshes carry vertex attributes (rule 2b), an array of its own beside the records -- frames of
// flat meshes neither allocate nor read it.  3 float4 per record, in the records' image-centre frame:
//   [0] (Ar, Br, Cr, smooth) [1] (Ag, Bg, Cg, -) [2] (Ab, Bb, Cb, -)     shade / z = A x + B y + C per channel,
// smooth != 0: the record's triangle is smooth and the pixel's colour is (A x + B y + C) / (za x + zb y + zc); 0: flat, rec[3].
#define SAS_MESH_PLANE_STRIDE 3
// planes: nullptr for a frame without vertex attributes
void sas_launch_mesh_bin(hipStream_t st, const SasMeshScene &m, const SasParams &P, const SasFrame &f, const SasMeshFrame &mf,
                         float4 *planes);
// sas_launch_blend for a frame with meshes (planes != nullptr: k_blend_mesh_smooth)
void sas_launch_blend_mesh(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f,
                           const SasMeshFrame &mf, const SasMeshExtra &x, const float4 *planes, bool fast_exp, bool want_max);

// Point-to-mesh queries (sas_query_meshes; DESIGN.md 3, "Mesh queries").  The host keeps a mesh's triangles with three finite vertices
// as records of three float4 (A, B, C; w unused) and the float32 box of their vertices; both kernels take the whole query by value.
#define SAS_QUERY_CHUNK 256   // triangles k_query_eval stages in LDS at a time (12 KiB)
struct SasQueryMesh {
    float lo[3], hi[3];   // box over the vertices of the kept triangles (lo > hi: none)
    int start, count;     // its records: tri[3 start .. 3 (start + count))
};
struct SasQuery {
    const float *points;        // [n,3]
    const float4 *tri;          // [3 n_tri]
    const SasQueryMesh *mesh;   // [n_meshes]
    int *list;                  // [n_meshes][n] candidate point ids per mesh, count[m] of them, in no particular order
    int *count;                 // [n_meshes]
    float *distance, *winding;  // [n_meshes][n] device, either may be nullptr
    long long n, n_tri;
    int n_meshes;
    float max_distance;
};
// count <- 0, the box pass (culled pairs read +inf / 0), the evaluation of the candidates
void sas_launch_query(hipStream_t st, const SasQuery &q);

// The 3x4 map A|t of the calls that need no scene, and a depth frame's view: its intrinsics and the map between the camera and the
// call's frame.  sas_affine_row (sas_device.h) is the one spelling of A p + t; it finds the map as the member `m` of its record.
struct SasAffine {
    float A[9], t[3];
};
struct SasDepthView {
    float fx, fy, cx, cy;
    SasAffine m;
};
static_assert(sizeof(SasDepthView) == 64, "a view's row is one 64-byte line");

// Point matching (sas_match_points; DESIGN.md 3, "Point matching").  All three kernels take the whole call by value.
#define SAS_MATCH_CHUNK 256     // targets k_match_slice stages in LDS at a time (4 KiB)
#define SAS_MATCH_MOMENTS 18    // n, sum p' (3), sum q (3), sum q p'^T (9, row-major), sum |p'|^2, sum d2
struct SasMatch {
    const float *source;        // [n_source,3]
    const float *target;        // [n_target,3]
    unsigned long long *keys;   // [slices][n_source] slice minima: bits(d2) << 32 | target index (d2 = +inf: none)
    int *index;                 // [n_source] device or nullptr
    float *dist2;               // [n_source] device or nullptr
    double *partial;            // [n_blocks][SAS_MATCH_MOMENTS] one row per workgroup of k_match_merge, or nullptr: no moments wanted
    double *moments;            // [SAS_MATCH_MOMENTS] device (with partial)
    long long n_source, n_target;
    long long n_blocks;         // ceil(n_source / 256)
    long long slice_targets;    // targets per slice, a multiple of SAS_MATCH_CHUNK
    int slices;                 // slices * slice_targets >= n_target
    SasAffine m;                // p' = A p + t
    float md2;                  // max_distance^2 in float32 (INFINITY: every match holds)
};
// keys <- slice minima, index / dist2 / partial <- the merge, moments <- the partial rows in workgroup order
void sas_launch_match(hipStream_t st, const SasMatch &m);

// Point clouds (sas_sample_points; DESIGN.md 3, "Point clouds").  Every kernel takes the whole call by value; the per-view and per-cloud
// rows live in one device block beside the keep table.
#define SAS_CLOUD_RESIDENT 16384   // survivors k_cloud_fps keeps in registers: 16 per lane of its 1024 (4 registers each; 128 are a lane's share)
struct SasCloudView {
    SasDepthView cam;      // cam.m: camera -> output frame
    int cloud, pad;
    long long base;        // first row of its cloud in rows / dist (SasCloud::cloud_base[cloud])
};
static_assert(sizeof(SasCloudView) == 80 && offsetof(SasCloudView, cloud) == 64, "the view's row, then its cloud");
struct SasCloud {
    const float *depth;         // [C,H,W]
    const uint8_t *rgb8;        // [C,H,W,3] or nullptr
    const uint8_t *labels;      // [C,H,W] or nullptr
    const SasCloudView *view;   // [C] device
    const long long *cloud_base;   // [E] device: S times the views of the clouds before
    const uint8_t *keep;        // [256] device, or nullptr
    unsigned *grid;             // [E][cells] lowest p per cell, 0xffffffff: empty (voxel > 0)
    float4 *cand;               // [C S] (w, cell bits; 0xffffffff: no candidate) per strided pixel
    unsigned *blk_count, *blk_off;   // [C bpv] survivors per block of k_cloud_compact, and where its first goes within its cloud
    float4 *rows;               // [C S] survivors (w, bits(p)), cloud e's from cloud_base[e], in p order
    float *dist;                // [C S] running distances of k_cloud_fps<false>, laid out as rows
    int *m_count;               // [E] survivors per cloud
    float *points;              // outputs (device): [E,K,3] or nullptr
    int32_t *index;             // [E,K]
    uint8_t *colors;            // [E,K,3] or nullptr
    uint8_t *labels_out;        // [E,K] or nullptr
    int32_t *count;             // [E] or nullptr
    long long S;                // strided pixels per view, Ws * Hs
    long long n_rows;           // C S
    long long n_pix;            // C H W
    long long n_blocks;         // C bpv
    long long cells, n_grid;    // nx ny nz, E cells
    int bpv;                    // ceil(S / 256)
    int C, E, W, H, Ws, stride, K;
    int has_bounds;
    int n[3];
    float lo[3], hi[3], voxel;
};
// ev (optional, 4 events): stamped in front of k_cloud_mark, k_cloud_compact, k_cloud_fps and behind the last kernel
void sas_launch_cloud(hipStream_t st, const SasCloud &q, hipEvent_t *ev);

// Depth fusion (sas_fuse_depth; DESIGN.md 3, "Depth fusion").  The kernel takes the whole call by value; the per-view rows live in one
// device block beside the keep table.
#define SAS_FUSE_THREADS 256      // voxels per workgroup of k_fuse
#define SAS_FUSE_MAX_ROWS 4096    // per-view rows of one launch: a call of more views is served by launches in view order
struct SasFuse {
    const float *depth;         // [C,H,W], the first view of this launch
    const uint8_t *rgb8;        // [C,H,W,3] or nullptr
    const uint8_t *labels;      // [C,H,W] or nullptr
    const SasDepthView *view;   // [C] device; m: volume frame -> camera
    const uint8_t *keep;        // [256] device, or nullptr (non-null only with labels)
    float *tsdf, *weight;       // [nz,ny,nx]
    float *color;               // [nz,ny,nx,3] or nullptr (non-null only with rgb8)
    long long n_vox;            // nx ny nz
    long long n_pix;            // C H W
    int n_rows;                 // rows of `view`
    int C, W, H;
    int nx, ny, nz;
    float lo[3], voxel, trunc, near_z, pixel_centre, max_weight;
};
void sas_launch_fuse(hipStream_t st, const SasFuse &q);

// Floats of a Gaussian's coefficient block (sh_degree < 0: a plain colour) and the colour planes (float4 per Gaussian) that hold them.
static inline int sas_coeff_floats(int sh_degree) { return sh_degree < 0 ? 3 : 3 * (sh_degree + 1) * (sh_degree + 1); }
static inline int sas_colour_planes(int sh_degree) { return (sas_coeff_floats(sh_degree) + 3) / 4; }

// The optimiser state the context keeps for the resident scene, in slot order: the one list of its buffers, on the host (Adam in sas_api.cpp)
// and in the kernels' arguments.  A group that has no state has nullptr.
struct SasAdamState {
    float4 *means_m, *means_v;     // [n_pad] (x, y, z, -) first and second moments
    float4 *opac;                  // [n_pad] (m, v, logit(opacity), -)
    float4 *quats_m, *quats_v;     // [n_pad]
    float4 *scales_m, *scales_v, *scales_raw;   // [n_pad] (x, y, z, -); raw = log(scale)
    float4 *sh_m, *sh_v;           // [planes][n_pad], laid out as col
};

// Optimiser step (sas_scene_adam_step; DESIGN.md 3, "Optimiser step").  k_adam_scene takes the whole call by value: the planes of the resident
// scene (written in place), the caller's gradients, and the state the context keeps in slot order.  A group whose gradient is nullptr is
// neither read nor written, and its state pointers may be nullptr.
struct SasAdam {
    float4 *g0, *g1, *g2, *col;    // the scene's planes (SasScene), writable
    const int *perm;               // [n] slot -> caller's index
    long long n, n_pad;
    int coeff_floats, planes;      // floats of a Gaussian's coefficient block, colour planes
    const float *d_means, *d_opac, *d_sh, *d_quats, *d_scales;   // gradients in the caller's order (device), nullptr: not stepped
    SasAdamState s;                // the state of the groups that are stepped
    float lr_means, lr_opac, lr_sh_dc, lr_sh_rest, lr_quats, lr_scales;
    float beta1, beta2, omb1, omb2;   // omb = 1 - beta (float32)
    float bc1, bc2;                   // 1 - beta^step (float64 on the host, rounded once)
    float eps;
    int visible_only;
    int sh_aligned;                   // coeff_floats % 4 == 0 and d_sh 16-byte aligned: the coefficient gradients load as float4
};
void sas_launch_adam_scene(hipStream_t st, const SasAdam &a);
// fresh.opac / fresh.scales_raw (either may be nullptr) <- (0, 0, logit(g0.w), 0) / (log(g2.xyz), 0); NaN where the value is outside the domain
void sas_launch_adam_init(hipStream_t st, int64_t n, const float4 *g0, const float4 *g2, const SasAdamState &fresh);
// sas_scene_read: the inverse of sas_launch_relayout.  Every output is a device array in the caller's order, or nullptr.
struct SasGather {
    const float4 *g0, *g1, *g2, *col;
    const int *perm;
    long long n, n_pad;
    int coeff_floats, planes;
    float *means, *quats, *scales, *cov6, *opac, *colors;
};
void sas_launch_scene_gather(hipStream_t st, const SasGather &q);

// Photometric loss (sas_photometric_loss; DESIGN.md 3, "Photometric loss"): (1 - lambda) L1 + lambda (1 - SSIM) of a frame against a target
// and its gradient with respect to the frame, prechained to the raw accumulators where `gate` is set.  Three launches on one stream:
// k_loss_stats (per-tile statistics, partial maps, per-workgroup sums), k_loss_tail (the sums in a fixed order -> terms and D),
// k_loss_grad (the second stencil and the composition).  lambda == 0 runs the L1 variants, which have no stencil and no maps.
struct SasLoss {
    const float *x, *y;            // [H][W][3] frame and target
    const unsigned char *mask;     // [H][W] or nullptr: != 0 counts
    int W, H, tiles_x, tiles_y;    // 16x16 pixel tiles
    float lambda;
    float win[11];                 // the Gaussian window, computed in double on the host and rounded once
    float bg[3];
    int gate;                      // prechain: g = 0 where x >= 1, g_alpha = -sum_c g[c] bg[c]
    float *maps;                   // [9][H W] scratch: (d/dmu_x, d/dsigma_x^2, d/dsigma_xy) x channel, times w; nullptr: terms only
    float *partial;                // [tiles][4] scratch: (sum w |x-y|, sum w ssim, sum w (x-y)^2, sum w) per workgroup
    float *norm;                   // [1] scratch: D = max(3 sum w, 1), written by the tail
    float *terms;                  // [4] (loss, l1, ssim, mse); ssim is NaN (not computed) when lambda == 0
    float *g_rgb, *g_alpha;        // [H][W][3], [H][W] or nullptr
};
void sas_launch_loss(hipStream_t st, const SasLoss &q);

// Density control (sas_density_accumulate, sas_scene_densify, sas_scene_reset_opacity; DESIGN.md 3, "Density control").  Every kernel takes
// its call by value.
struct SasDensityStats {
    const uint4 *info;          // [n] the backward frame's info records (slot order): z, w = the radii, 0: culled
    const int *perm;            // [n] slot -> caller's index
    const float *d_means2d;     // [n,2] the frame's screen-space gradient (caller's order)
    float *grad_sum;            // [n] caller's order, ADDED to
    int *count;                 // [n]
    float *max_radius;          // [n] or nullptr
    long long n;
    float half_w, half_h;       // 0.5 W, 0.5 H
};
void sas_launch_density_accumulate(hipStream_t st, const SasDensityStats &q);

#define SAS_DENSIFY_GROW 1u
#define SAS_DENSIFY_PRUNE_OPACITY 2u
#define SAS_DENSIFY_PRUNE_SCALE 4u
// What a densify call makes of its class totals: the growth candidates are ranked clones first, then splits, each by parent index; the
// first `budget` of them happen (every one adds one Gaussian), the others stay survivors.  Host and device compute it alike.
struct SasDensityPlan {
    long long survivors, clones, splits, n_new;
};
static inline __host__ __device__ SasDensityPlan sas_density_plan(long long kept, long long clone_cand, long long split_cand, long long max_gaussians)
{
    long long budget = clone_cand + split_cand;
    if (max_gaussians > 0) {
        const long long room = max_gaussians > kept ? max_gaussians - kept : 0;
        budget = budget < room ? budget : room;
    }
    SasDensityPlan p;
    p.clones = clone_cand < budget ? clone_cand : budget;
    p.splits = split_cand < budget - p.clones ? split_cand : budget - p.clones;
    p.survivors = kept - p.splits;
    p.n_new = p.survivors + p.clones + 2 * p.splits;
    return p;
}
struct SasDensity {
    const float4 *g0, *g1, *g2, *col;   // the old scene's planes
    const uint8_t *gid8;
    const int *perm;            // [n] old slot -> caller's index
    int *inv;                   // [n] scratch: caller's index -> old slot
    long long n, n_pad;
    int coeff_floats, planes, cov_mode;
    const float *grad_sum;      // [n] the caller's statistics
    const int *count;           // [n]
    float grow_grad2d, grow_scale, prune_opacity, prune_scale;   // the scale thresholds are times the extent already
    float split_factor;
    unsigned flags, seed;
    long long max_gaussians;
    uint8_t *cls;               // [n] scratch: class bits per Gaussian
    unsigned *blk_count, *blk_off;   // [3][nb] scratch: kept, clone candidates, split candidates per workgroup, and their exclusive offsets
    unsigned *totals;           // [3] scratch
    long long nb;               // ceil(n / 256)
    // the new scene in the caller's order (sas_launch_density_scatter), as sas_scene_upload takes it
    float *means, *quats, *scales, *cov6, *opac, *colors;
    uint8_t *gid;               // or nullptr: no groups
    int *parents;               // [n_new]
    long long n_new;
};
// inv, cls, blk_count, blk_off, totals <- the classes of the old set
void sas_launch_density_classes(hipStream_t st, const SasDensity &q);
// ... and, once the host has sized the new scene from the totals, its rows
void sas_launch_density_scatter(hipStream_t st, const SasDensity &q);
// The optimiser state of the new scene, in its storage order: a survivor's is its parent's, a clone's and a child's is fresh (zero
// moments, raw values from the new planes as sas_launch_adam_init computes them).  A group without state has nullptr on both sides.
struct SasDensityState {
    const int *perm_new, *parents, *inv_old;
    const float4 *g0_new, *g2_new;
    long long n_new, n_survivors, n_old, n_pad_old, n_pad_new;
    int planes;
    SasAdamState old_, new_;   // (old_ is only read)
};
// fresh: [n_new] in the new caller's order, non-zero marks the fresh rows (sas_scene_mcmc_refine); nullptr: the rows from n_survivors on
void sas_launch_density_state(hipStream_t st, const SasDensityState &q, const uint8_t *fresh = nullptr);
// inv[perm[slot]] = slot
void sas_launch_density_inverse(hipStream_t st, int64_t n, const int *perm, int *inv);
// opacity <- min(opacity, cap) in g0; opac (nullptr: no state) <- (0, 0, logit(cap), -) where it changed
void sas_launch_opacity_reset(hipStream_t st, int64_t n, float cap, float4 *g0, float4 *opac);

// MCMC density control (sas_scene_mcmc_noise, sas_scene_mcmc_refine; DESIGN.md 3, "MCMC density control").  Every kernel takes its call
// by value.
struct SasMcmcNoise {
    float4 *g0;                 // the means are written in place
    const float4 *g1, *g2;
    const int *perm;            // [n] slot -> caller's index
    long long n;
    int cov_mode;
    float scale;
    unsigned seed, step;
};
void sas_launch_mcmc_noise(hipStream_t st, const SasMcmcNoise &q);

#define SAS_MCMC_MAX_N 51   /* gsplat's binomial table: a source is relocated as min(copies + 1, 51) Gaussians */
// What a refine call makes of the alive count (the product in binary64, as gsplat's int(grow_factor * N)).
struct SasMcmcPlan {
    long long n_dead, n_grow, draws, n_new;
};
static inline SasMcmcPlan sas_mcmc_plan(long long n, long long n_alive, long long cap_max, double grow_factor)
{
    SasMcmcPlan p;
    const double want = floor(grow_factor * (double)n);
    const long long target = want < (double)cap_max ? (long long)want : cap_max;
    p.n_dead = n - n_alive;
    p.n_grow = target > n ? target - n : 0;
    p.draws = p.n_dead + p.n_grow;
    p.n_new = n_alive + p.draws;
    return p;
}
struct SasMcmc {
    const float4 *g0, *g1, *g2, *col;   // the old scene's planes (quaternions and scales)
    const uint8_t *gid8;
    const int *inv;             // [n] caller's index -> old slot (sas_launch_density_inverse)
    long long n, n_pad;
    int coeff_floats, planes;
    float min_opacity;
    unsigned seed;
    // scratch, in the caller's order
    unsigned *weight;           // [n] alive ? (uint32)(o 2^24) : 0
    unsigned long long *prefix; // [n] inclusive sums of weight
    unsigned *copies;           // [n] draws that selected i (zeroed by the caller)
    float4 *reloc;              // [n] (o', scale'), written for the sources
    unsigned *blk_alive, *blk_alive_off;          // [nb] alive per workgroup, and the exclusive offsets
    unsigned long long *blk_weight, *blk_weight_off;   // [nb] weight per workgroup, and the exclusive offsets
    unsigned long long *totals; // [2] (alive, weight)
    long long nb;               // ceil(n / 256)
    // once the host has sized the new scene from the totals: the draws and the new rows in the caller's order
    long long n_alive, draws, n_new;
    unsigned long long total_weight;
    int *source;                // [draws] the old index draw d selected
    float *means, *quats, *scales, *opac, *colors;
    uint8_t *gid;               // or nullptr: no groups
    int *parents;               // [n_new]
    uint8_t *fresh;             // [n_new] 1: a source or a child (its optimiser state starts anew)
};
// weight, blk_*, totals <- the alive set and its weights
void sas_launch_mcmc_weights(hipStream_t st, const SasMcmc &q);
// ... and, once the host has read the totals: prefix, copies, source, reloc, and the rows of the new scene
void sas_launch_mcmc_rows(hipStream_t st, const SasMcmc &q);
// parents[i] = i (a call with nothing to do)
void sas_launch_mcmc_identity(hipStream_t st, int64_t n, int *parents);

// Storage order on the device (sas_storage_order, and behind sas_scene_upload, sas_scene_densify and sas_scene_mcmc_refine; DESIGN.md 3,
// "Storage order"): the permutation storage_order() of sas_api.cpp gives on the host.  Every kernel takes its call by value.
#define SAS_ORDER_TILE 2048         // keys a workgroup of a sort pass ranks (eight per lane); Gaussians per workgroup of the bounds pass
#define SAS_ORDER_SCAN_ROUND 1024   // entries of the [256][tiles] histogram table the one-workgroup scan takes per round (four per lane)
#define SAS_ORDER_PARTIAL 8         // ints of a workgroup's partial bounds: lo[3], hi[3] (as ordered ints), the first bad index, one unused
struct SasOrderRecord {
    float lo[3], hi[3], inv[3];   // per axis over the finite coordinates; inv = hi > lo ? 1023 / (hi - lo) : 0
    int bad_index, bad_id;        // the smallest i with gid[i] >= n_groups and that id; -1, 0: none
};
struct SasOrder {
    const float *means;           // [n,3] caller's order
    const uint8_t *gid;           // [n] or nullptr: no groups (and no fifth pass)
    long long n, n_tiles;         // n_tiles = ceil(n / SAS_ORDER_TILE)
    int n_groups;                 // ids at or above it are reported in rec (256: none can be)
    int *perm;                    // [n] out: slot -> caller's index
    // scratch
    unsigned long long *key[2];   // [n] each: group << 32 | Hilbert index, ping and pong
    int *idx[2];                  // [n] each: the caller's indices that travel with the keys
    unsigned *table;              // [256][n_tiles] digit-major histogram of a pass, then its exclusive offsets (16-byte aligned)
    int *partial;                 // [n_tiles][SAS_ORDER_PARTIAL]
    SasOrderRecord *rec;
};
// bounds, keys and the sort: 3 + 3 x (4 or 5) launches on st, nothing else
void sas_launch_order(hipStream_t st, const SasOrder &q);
// the first two launches of sas_launch_order alone: q.rec <- lo, hi, inv (and the group record) of q.means; reads means, gid, n, n_tiles, n_groups,
// writes partial and rec (sas_knn.hip takes its grid's bounds from it)
void sas_launch_order_bounds(hipStream_t st, const SasOrder &q);

// k nearest neighbours within one cloud (sas_knn_points; DESIGN.md 3, "Scene from points").  Every kernel takes its call by value; what the
// device decides (the grid, the leftover count) lives in one record the kernels read.
#define SAS_KNN_MAX_K 8
#define SAS_KNN_MAX_AXIS 1024           // cells per axis at most: the stop bound's rounding margin is derived for it (sas_knn.hip)
#define SAS_KNN_MAX_CELLS (1 << 21)     // the table budget: cells of a grid at most (8 MiB of starts)
#define SAS_KNN_SCAN_BLOCK 2048         // table entries per workgroup of the scan kernels (eight per lane)
#define SAS_KNN_RING_LIMIT 4            // a lane still searching after this Chebyshev ring goes to the leftover list
#define SAS_KNN_CHUNK 256               // candidates k_knn_brute stages in LDS at a time (4 KiB)
#define SAS_KNN_COARSE 32               // cells per axis of the occupancy bitmask the grid rule reads
struct SasKnnGrid {
    float lo[3];          // the finite bounds' lower corner
    float inv, h_lo;      // cell(v) = min((int)((v - lo) * inv), n - 1); h_lo: a float below the real 1 / inv
    int n[3], n_cells;    // cells per axis (x fastest) and their product
    int brute;            // 1: no grid (forced, or no extent to divide): every point goes through k_knn_brute, in the caller's order
    unsigned left_count;  // points the ring search handed to k_knn_brute
    int occupied[2];      // occupied cells of the 32^3 and the 16^3 coarse grid (what the rule saw)
};
struct SasKnn {
    const float *points;          // [n,3] caller's order
    long long n;
    int k, forced_g;              // forced_g > 0: SAS_KNN_GRID
    float *dist2;                 // [n,k] out
    int *index;                   // [n,k] out or nullptr
    // scratch
    const SasOrderRecord *bounds; // of sas_launch_order_bounds
    unsigned *occ;                // [32 * 32] words: bit x of word z * 32 + y is coarse cell (x, y, z)
    SasKnnGrid *grid;
    unsigned *table;              // [table_len] counts, then starts, then ends per cell; table[-1] == 0; cell n_cells holds the non-finite points
    unsigned *blk;                // [table_len / SAS_KNN_SCAN_BLOCK] block sums, then their exclusive offsets
    float4 *pts;                  // [n] (x, y, z, bits(index)) in cell order
    int *left;                    // [n] positions in pts of the leftover points, in no particular order
    unsigned long long *keys;     // [slices][n][K] slice results of k_knn_brute
    long long cells_cap;          // cells the grid may have: table_len >= cells_cap + 1
    long long table_len;          // a multiple of SAS_KNN_SCAN_BLOCK
    long long slice_points;       // candidates per slice, a multiple of SAS_KNN_CHUNK
    int slices;
};
void sas_launch_knn(hipStream_t st, const SasKnn &q);

// Deformable splats (sas_knn_cross, sas_scene_skin, sas_scene_deform; DESIGN.md 3, "Deformation"; sas_skin.hip).  Every kernel takes its call
// by value.
#define SAS_KNN_CROSS_MAX_NODES 65536   // nodes of the second cloud at most: every lane walks them all
#define SAS_SKIN_MAX_K 8                // entries per Gaussian at most; the planes hold 4 (k <= 4) or 8
#define SAS_SKIN_LDS_BYTES 16384        // node records k_deform stages in LDS at most (256 records): the SAS_SKIN_LDS budget's default and ceiling
// k nearest nodes of another cloud for every point: sas_knn.hip's contract, nothing left out by index, and a cut at md2
struct SasKnnCross {
    const float *points;   // [n,3]
    const float *nodes;    // [m,3]
    long long n;
    int m, k;
    float md2;             // max_distance^2 in float32 (INFINITY: no cut)
    float *dist2;          // [n,k] out
    int *index;            // [n,k] out or nullptr
};
void sas_launch_knn_cross(hipStream_t st, const SasKnnCross &q);
// A node's record: the rows [R | t] as given and the unit quaternion wxyz of R
struct SasSkinNode {
    float Rt[12], q[4];
};
static_assert(sizeof(SasSkinNode) == 64, "a node's record is one 64-byte line");
// The skin planes, slot order: plane p of idx / w holds entries 4p .. 4p + 3 of every slot, stride n_pad
struct SasSkinBind {
    const int *perm;        // [n] slot -> caller's index
    const int *indices;     // [n,k] caller's order
    const float *weights;   // [n,k]
    long long n, n_pad;
    int k, kp;              // kp = 4 or 8: entries k .. kp - 1 read (-1, 0)
    int4 *idx;              // [kp / 4][n_pad]
    float4 *w;              // [kp / 4][n_pad]
};
void sas_launch_skin_bind(hipStream_t st, const SasSkinBind &q);
// ... and back in the caller's order (sas_scene_skin_read)
struct SasSkinRead {
    const int *perm;
    const int4 *idx;
    const float4 *w;
    long long n, n_pad;
    int k;
    int *indices;           // [n,k] out
    float *weights;         // [n,k] out
};
void sas_launch_skin_read(hipStream_t st, const SasSkinRead &q);
struct SasDeform {
    const float *node_Rt;        // [m,12] the caller's rows
    SasSkinNode *nodes;          // [m] scratch: written by k_skin_nodes, read by k_deform
    const float4 *r0, *r1, *r2;  // the rest planes
    float4 *g0, *g1, *g2;        // the scene's planes, written
    const int4 *idx;
    const float4 *w;
    long long n, n_pad;
    int m, kp, cov_mode;
    int lds;                     // 1: the node records pass through LDS (m * 64 B within the budget)
};
void sas_launch_deform(hipStream_t st, const SasDeform &q);
void sas_launch_deform_planes(hipStream_t st, const SasDeform &q);   // k_deform alone, on the records q.nodes holds already (node_Rt unused)
// The adjoint to the REST arrays (sas_scene_deform_backward_rest): per-Gaussian gradients of the deformed arrays -> of the rest arrays, added
struct SasDeformRestGrad {
    const int *perm;             // [n] slot -> caller's index
    const float *d_means;        // [n,3] caller's order, or nullptr
    const float *d_quats;        // [n,4] or nullptr (quaternion scenes)
    const float *d_cov6;         // [n,6] or nullptr (covariance scenes)
    const SasSkinNode *nodes;    // [m] the last sas_scene_deform's records
    const int4 *idx;
    const float4 *w;
    long long n, n_pad;
    int m, kp;
    int lds;                     // 1: the node records pass through LDS (m * 64 B within the budget)
    int bound_only;              // 1: a Gaussian without a live entry adds nothing (0: its gradient passes through)
    float *o_means;              // [n,3] added to; given exactly where d_means is
    float *o_quats;              // [n,4]
    float *o_cov6;               // [n,6]
};
void sas_launch_deform_rest_grad(hipStream_t st, const SasDeformRestGrad &q);
// The adjoint of the two (sas_scene_deform_backward): per-Gaussian gradients -> per-node [R | t] gradients
#define SAS_SKIN_GRAD_ROW 16              // floats a live entry adds to its node's accumulator row: dt 3, the mean path's dR 9, dq 4
#define SAS_SKIN_GRAD_LDS_MAX 131072      // accumulator bytes k_deform_grad keeps in LDS at most (2048 nodes): the SAS_SKIN_GRAD_LDS budget's ceiling
#define SAS_SKIN_GRAD_LDS_BYTES 131072    // ... and its default: at 2048 nodes the LDS path is still 2.4x the global one (profiles/deform_grad.txt)
#define SAS_SKIN_GRAD_STAGED_LDS_BYTES 16384   // LDS path: accumulator bytes up to which the rows are staged (256 nodes: staged 0.39 ms, own rows 0.47; at 1024 0.50 and 0.46)
struct SasDeformGrad {
    const int *perm;             // [n] slot -> caller's index
    const float *d_means;        // [n,3] caller's order, or nullptr
    const float *d_quats;        // [n,4] or nullptr (quaternion scenes)
    const float *d_cov6;         // [n,6] or nullptr (covariance scenes)
    const SasSkinNode *nodes;    // [m] the last sas_scene_deform's records
    const float4 *r0, *r1, *r2;  // the rest planes
    const int4 *idx;
    const float4 *w;
    long long n, n_pad;
    int m, kp, cov_mode;
    int lds;                     // 1: the accumulator rows are summed in LDS and flushed once per workgroup
    int staged;                  // 1: a workgroup's rows pass through LDS and are added 16 lanes per row
    int blocks;                  // workgroups of the persistent grid
    float *acc;                  // [m,16] zeroed by the caller on the stream
    float *out;                  // [m,12] written
};
size_t sas_deform_grad_lds_bytes(int m, bool lds, bool staged);   // dynamic LDS of one workgroup
void sas_launch_deform_grad(hipStream_t st, const SasDeformGrad &q);

// The node optimiser on the device (sas_nodes_rigidity, sas_nodes_twist_step; DESIGN.md 3, "Deformation"; sas_nodes.hip).  The state is binary64.
#define SAS_NODES_MAX_K 8                 // neighbours per node of the rigidity term at most
#define SAS_NODES_MAX_PARTIALS 256        // workgroups of k_nodes_rigidity at most: one partial sum of the value each (the context's 2 KiB)
struct SasNodesRigidity {
    const float *nodes;      // [m,3] rest positions
    const double *Rt;        // [m,12] rows [R | t]
    const int *nb;           // [m,kn] neighbour table; an entry outside [0, m) is ignored
    const int *rev_start;    // [m + 1] node -> its range of rev_edge
    const int *rev_edge;     // edge numbers i * kn + slot with nb[i][slot] == node, ascending per node; the first rev_start[m] <= m kn are read
    int m, kn;
    double *d_Rt;            // [m,12] written
    double *partial;         // [SAS_NODES_MAX_PARTIALS] scratch: a workgroup's sum of |r|^2
    double *value;           // [1] written
};
void sas_launch_nodes_rigidity(hipStream_t st, const SasNodesRigidity &q);   // two launches
struct SasNodesStep {
    const float *nodes;      // [m,3]
    const float *d32;        // [m,12] or nullptr
    const double *d64;       // [m,12] or nullptr: the gradient is double(d32) + weight * d64
    double weight;
    double *Rt, *m1, *m2;    // [m,12], [m,6], [m,6] in place
    float *Rt32;             // [m,12] written: float(Rt)
    int m;
    double lr_rot, lr_trans, beta1, beta2, gain1, gain2, c1, c2, eps;   // sas_node_step_config
};
void sas_launch_nodes_step(hipStream_t st, const SasNodesStep &q);
// The node driver (sas_nodes_fit_rigid): every node's rigid [R | t] from moved node positions.
#define SAS_NODES_FIT_GAP 1e-9            // eigenvalues of Horn's matrix within this times the largest |eigenvalue| of the top one span the quaternion's space
#define SAS_NODES_FIT_HALF_TURN 1e-12     // a projection of (1,0,0,0) onto that space with a squared norm below this is an exact half turn
// Cyclic Jacobi sweeps, FIXED.  Counted on the CPU by tests/tools/node_fit_ref.py (sweeps_needed): the smallest count after which the largest
// off-diagonal entry stays within four roundings (4 * 2^-53) of the largest |eigenvalue| is 12 over the kit's 22 668 matrices and 11 over 100 000
// drawn ones (full rank, rank two, rank one, a repeated singular value, scales 1e-20 .. 1e20).  Both counts belong to rank-one matrices (two
// members, a rope): the double top eigenvalue's pair converges linearly there, halving per sweep from up to 2.5e-13 of the scale -- an entry
// between two eigenvectors that are both in the quaternion's span, so it never reaches the result.  Every matrix of another kind is at 1e-14
// after five sweeps and at an exact zero after eight.  Plus two: 14.
#define SAS_NODES_FIT_SWEEPS 14
#define SAS_NODES_FIT_MAX_LANES (1 << 30)  // steps * m at most: one lane each, in 256-lane workgroups of one grid
struct SasNodesFit {
    const float *nodes;      // [m,3] rest positions
    const float *moved;      // [steps,m,3]
    const int *nb;           // [m,kn] neighbour table; an entry outside [0, m) is ignored
    int steps, m, kn;
    double *Rt64;            // [steps,m,12] written, or nullptr
    float *Rt32;             // [steps,m,12] written: float(Rt64)
};
void sas_launch_nodes_fit(hipStream_t st, const SasNodesFit &q);
