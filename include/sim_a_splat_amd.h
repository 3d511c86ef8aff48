/*
 * sim_a_splat_amd.h -- C ABI of the MI355X (gfx950) Gaussian-splat rasterizer that sits behind
 * sim_a_splat's render-image calls.
 *
 * The reference reaches its renderer through two Python call sites and has no native FFI of its
 * own, so every entry point cites the reference call it serves
 * (paths relative to the reference tree):
 *
 *   Door A  GaussianSplat.render(pose) -> pipeline.model.get_outputs_for_camera(cameras, obb_box=None)
 *           sim_a_splat/ns_utils/nerfstudio_utils.py:123-177 (call at :166-172)
 *   Door B  client.get_render(height, width, wxyz, position)
 *           sim_a_splat/env/splat/splat_env_wrapper.py:148-157, sim_a_splat/splat/splat_handler.py:339-344
 *           scene.add_gaussian_splats(...) registration      sim_a_splat/splat/splat_handler.py:106-141
 *           handle.wxyz / handle.position updates             sim_a_splat/splat/splat_handler.py:283-288
 *
 * Conventions: plain C types only.  `means`, `quats`, ... of sas_scene_upload may be host or
 * device pointers (copied with hipMemcpyDefault).  Output pointers of sas_render are DEVICE
 * pointers owned by the caller (e.g. torch tensors' data_ptr()).  viewmat / K / background /
 * group poses are small HOST arrays.  No exceptions cross the ABI: every call returns 0 or a
 * negative sas_status and sas_last_error() describes the failure.  One ctx per (device, stream);
 * calls on one ctx are not re-entrant.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 */
#ifndef SIM_A_SPLAT_AMD_H
#define SIM_A_SPLAT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sas_ctx sas_ctx;

typedef enum {
    SAS_OK = 0,
    SAS_ERR_INVALID = -1,   /* bad argument */
    SAS_ERR_HIP = -2,       /* a HIP runtime call failed */
    SAS_ERR_NO_SCENE = -3,  /* render before sas_scene_upload */
    SAS_ERR_OOM = -4,       /* device allocation failed */
    SAS_ERR_NO_DEVICE = -5  /* no gfx950 device visible */
} sas_status;

/* sas_render flags */
#define SAS_DEPTH_FILL_MAX 1u /* depth = where(alpha > 0, ED, max(ED)): nerfstudio get_outputs (T0) */
#define SAS_ASYNC 2u          /* enqueue only (<= 4 frames in flight).  Frames COMPLETE in submission order, inside later
                                 sas_render* calls (when a slot is needed) or sas_wait(): completion = the host has checked
                                 that the frame fitted its intersection buffer (a frame that did not is rendered again
                                 first).  A frame's outputs may be consumed -- by the host after a synchronisation, or by
                                 work put on `stream` afterwards, which is then ordered behind the frame -- only once it
                                 is complete; sas_frames_completed() tells how many are. */
#define SAS_FAST_EXP 4u       /* v_exp_f32 instead of the contract polynomial: NOT bit-exact with the oracle */
#define SAS_TIMING 8u         /* record per-stage hipEvents (readable with sas_stage_times) */
#define SAS_TIME_TILES 32u    /* HIP events around the tile kernel only (SAS_T_BLEND); frames still pipeline */
#define SAS_FULL_SORT 16u     /* order every tile list completely and keep it (sas_read_tile_lists); same image */
#define SAS_MESH_SURFACE 64u  /* frames with meshes: alpha, depth and the RGB-D points / mask describe the whole scene -- where a
                                 triangle shows it closes the ray as a last entry of opacity 1 (sas_scene_meshes); nothing else changes */

/* sas_stage_times slots (milliseconds of the last completed frame rendered with SAS_TIMING).  SAS_T_SCAN reads ~0:
 * the offsets scan is the tail of the projection kernel (its last workgroup), not a launch of its own.  SAS_T_SCATTER
 * reads ~0 as well on the product path (single-pass binning: the projection emits the intersection keys itself into
 * fixed-stride tile segments); it times k_scatter for SAS_FULL_SORT frames and with SAS_DIRECT=0 in the environment
 * (two-pass binning: count, scan, scatter), which also serves frames whose segments would exceed SAS_DIRECT_BUDGET_MB
 * (default 6144 MB per frame in flight). */
enum { SAS_T_PROJECT = 0, SAS_T_SCAN, SAS_T_SCATTER, SAS_T_SORT /* full path only */,
       SAS_T_BLEND /* k_tile_lazy, or k_blend on the full path */, SAS_T_TAIL /* depth fill */,
       SAS_T_TOTAL, SAS_T_COUNT };

/* sas_frame_stats slots (int64) of the last completed frame.  SAS_S_NISECT counts Gaussian x 16-pixel-tile intersections
 * (gsplat's isect count) whatever the frame's own binning; SAS_S_NKEYS what the frame actually binned (fewer on single-pass
 * frames, whose lists leave out the tiles of a rectangle the Gaussian cannot reach -- no pixel changes; SAS_CULL=0 bins whole
 * rectangles -- and more in the quad layout, which bins in 8-pixel tiles); SAS_S_MAX_TILE_LEN is the longest list of the frame's own tiles;
 * SAS_S_CAPACITY the keys the frame's buffer holds (single-pass binning: tiles x segment; two-pass: the compact buffer). */
enum { SAS_S_NVISIBLE = 0, SAS_S_NISECT, SAS_S_MAX_TILE_LEN, SAS_S_CAPACITY, SAS_S_REGROWS,
       SAS_S_WINDOW_MISSES /* workgroups that binned with per-intersection atomics */,
       SAS_S_FALLBACK_TILES /* tiles the lazy kernel had to order completely */,
       SAS_S_QUAD_LAYOUT /* 1: the frame ran in the quad layout (views of a few hundred tiles): binned in 8-pixel tiles, one
                            workgroup per 8x8 quadrant with one wave per 4x4 block */,
       SAS_S_LAUNCH_VIEWS /* views that shared the frame's launches (1, or the size of its launch group) */,
       SAS_S_NKEYS /* intersection keys written at the frame's own tile size */, SAS_S_COUNT };

/* Create / destroy a rasterizer context on HIP device `device`. */
int sas_create(int device, sas_ctx **out);
int sas_destroy(sas_ctx *ctx);

/*
 * Upload (replace) the scene.  Serves GSplatLoader -> scene registration
 * (sim_a_splat/splat/splat_utils.py:33-45, splat_handler.py:106-141).
 *   means      [n,3]   world positions
 *   quats      [n,4]   wxyz, any norm   } Door A form (gsplat normalises), or both NULL and
 *   scales     [n,3]   exp() applied    }
 *   cov6       [n,6]   xx xy xz yy yz zz  Door B form (viser takes 3x3 covariances)
 *   opacities  [n]     sigmoid() applied
 *   colors     sh_degree >= 0: [n,(sh_degree+1)^2,3] SH coefficients (features_dc ++ features_rest)
 *              sh_degree <  0: [n,3] final RGB in 0..1 (Door B: SH2RGB already applied)
 *   group_id   [n] uint8 splat-group index, or NULL (single static group)
 *   n_groups   number of groups (<= 256); poses start as identity
 * Values are taken as they are (no validation pass over the scene): every float32 is defined input.  A Gaussian whose projection
 * is not finite is culled; NaN / Inf / out-of-range opacities and colours render exactly as the oracle renders them (DESIGN.md 3,
 * "Inputs outside the reference's range"; colours leave the projection clamped to +-FLT_MAX); no input makes a kernel leave its
 * buffers (tests/tools/oracle_fuzz.py poisons scenes on the bounds-checked build).
 */
int sas_scene_upload(sas_ctx *ctx, int64_t n, const float *means, const float *quats, const float *scales,
                     const float *cov6, const float *opacities, const float *colors, int sh_degree,
                     const uint8_t *group_id, int n_groups);

/* Per-group rigid poses, [n_groups,12] row-major (R|t), host pointer.  Serves the per-step
 * `splat_links_handler[i].wxyz/.position = ...` assignments (splat_handler.py:283-288).
 * The poses apply to the frames submitted AFTER the call: every frame carries a snapshot of the poses it was
 * submitted with, so frames in flight (SAS_ASYNC) are neither disturbed nor waited for. */
int sas_set_group_poses(sas_ctx *ctx, int n_groups, const float *Rt);

/*
 * The per-link pose algebra of SplatHandler.draw_handler (splat_handler.py:239-288) inside the library, float64:
 *   R_k = Ri Rm_k Rfk_k^T Ri^T,   t_k = ti - R_k ti + s Ri (tm_k - Rm_k Rfk_k^T tfk_k),   tm_k = p_msg_k + weld,
 * with Rm_k the rotation of the message quaternion; the rotation is rounded through a unit quaternion, as the
 * reference's handles store one (handle.wxyz = ..., :283-288).
 * sas_set_link_constants, once per scene (after sas_scene_upload, which forgets them): the ICP similarity (scale s,
 *   rotation Ri [9], translation ti [3]: splat_handler.py:66-83), per link k the forward kinematics of its visual mesh
 *   at mask time (Rfk [n_links,9], tfk [n_links,3]: :147-200), the weld translation (:229; NULL = 0) and the splat
 *   group each link drives (NULL: group k).
 * sas_set_link_poses, per env step: the first k_links links' message poses (q_msg [k,4] wxyz any norm, p_msg [k,3])
 *   become the poses of their groups (the other groups keep theirs), exactly as sas_set_group_poses would set them;
 *   Rt_out (or NULL) receives all current group poses [n_groups,12].
 * sas_get_group_poses: the current poses.
 */
int sas_set_link_constants(sas_ctx *ctx, int n_links, double scale, const double *Ri, const double *ti, const double *Rfk,
                           const double *tfk, const double *weld, const int *group);
int sas_set_link_poses(sas_ctx *ctx, int k_links, const double *q_msg, const double *p_msg, float *Rt_out);
int sas_get_group_poses(sas_ctx *ctx, int n_groups, float *Rt);
/* Camera riding on a link (SplatHandler.get_attached_frame, splat_handler.py:316-332) with the context's ICP
 * similarity: pose = icp o SE3(q_link, (p_link + local_xyz) * s) -- the local offset is ADDED in world axes, as the
 * reference does.  Outputs: unit quaternion wxyz [4] and position [3] of the camera-to-world pose. */
int sas_link_attached_frame(sas_ctx *ctx, const double *q_link, const double *p_link, const double *local_xyz,
                            double *wxyz_out, double *xyz_out);

/* The same algebra as pure functions (no context, no GPU; float64 in, what the GPU gets out): the CPU tests hold them
 * against the NumPy forms of sim_a_splat_amd/poses.py.
 *   sas_link_group_poses   k link message poses -> Rt_out [k,12] float32 (the expression of sas_set_link_constants)
 *   sas_attached_frame     as sas_link_attached_frame with the similarity given
 *   sas_camera_matrices    n camera-to-world poses (wxyz [n,4] any norm, position [n,3], OpenCV axes) + vertical field of
 *                          view -> viewmats [n,16] and Ks [n,9] float32: V = [R^T | -R^T p], f = (H/2) / tan(fov/2),
 *                          principal point at the image centre (what get_render's camera means) */
int sas_link_group_poses(int k_links, double scale, const double *Ri, const double *ti, const double *Rfk, const double *tfk,
                         const double *weld, const double *q_msg, const double *p_msg, float *Rt_out);
int sas_attached_frame(double scale, const double *Ri, const double *ti, const double *q_link, const double *p_link,
                       const double *local_xyz, double *wxyz_out, double *xyz_out);
int sas_camera_matrices(int n, const double *wxyz, const double *position, double fov, int width, int height,
                        float *viewmats, float *Ks);

/*
 * Render one view.  Serves get_outputs_for_camera (Door A) and get_render (Door B).
 *   viewmat     [16] row-major world->camera, OpenCV axes (+z forward)
 *   K           [9]  row-major intrinsics
 *   background  [3]
 *   rgb   [H,W,3] f32 or NULL     clamp(render + (1-alpha)*background, 0, 1)
 *   alpha [H,W]   f32 or NULL     accumulation
 *   depth [H,W]   f32 or NULL     expected depth (see SAS_DEPTH_FILL_MAX)
 *   rgb8  [H,W,3] u8  or NULL     floor(rgb*255 + 0.5)
 *   stream      hipStream_t (NULL = default stream): the frame's writes to the output buffers are ordered
 *               behind everything enqueued on it before the call (the scene itself is synchronised by
 *               sas_scene_upload / sas_set_group_poses, which return only when their data is in place)
 * Without SAS_ASYNC the call returns after the frame is complete.
 */
int sas_render(sas_ctx *ctx, const float *viewmat, const float *K, int width, int height,
               const float *background, unsigned flags, float *rgb, float *alpha, float *depth,
               uint8_t *rgb8, void *stream);

/*
 * sas_render with the RGB-D consumer fused into the depth pass.  Replaces the unprojection of
 * GaussianSplat.generate_RGBD_point_cloud (ns_utils/nerfstudio_utils.py:424-445):
 *   points [H,W,3]  camera-frame (x, y, z) = ((u - cx) * d / fx, (v - cy) * d / fy, d), d = the depth output
 *                   (after the SAS_DEPTH_FILL_MAX fill when that flag is set); u, v integer pixel indices
 *   mask   [H,W]    uint8: d < *max_depth, or all ones when max_depth is NULL
 * `depth` is required when points or mask is given; points / mask may each be NULL.
 */
int sas_render_rgbd(sas_ctx *ctx, const float viewmat[16], const float K[9], int width, int height,
                    const float background[3], unsigned flags, const float *max_depth, float *rgb, float *alpha,
                    float *depth, float *points, uint8_t *mask, void *stream);

/*
 * Per-Gaussian feature channels, composited through exactly the frame's own weights.  Serves Door A's
 * get_outputs_for_camera(..., compute_semantics) (ns_utils/nerfstudio_utils.py:123, :166-172) for feature-splat models, whose
 * per-Gaussian vectors (the point-cloud helpers' clip_embeds, :343-402) are alpha-blended as the colours are, and the per-link
 * splat groups of the segmentation step (splat_handler.py:62-83) as masks: one-hot group features.
 * sas_scene_features, after sas_scene_upload (a new upload forgets the features, as it forgets the link constants):
 *   features  [n,channels] float32, host or device, the caller's Gaussian order, 1 <= channels <= 256; NaN becomes -FLT_MAX and
 *             +-Inf +-FLT_MAX (the colours' finite mapping); NULL: one-hot of the scene's group ids, channels == n_groups
 *   SAS_ERR_NO_SCENE without a scene; SAS_ERR_INVALID when n is not the scene's, channels is out of range, or one-hot is
 *   asked of a scene without groups.  Returns when the store is in place (frames in flight are completed first).
 * sas_render_features: sas_render's frame (rgb / alpha / depth bit-identical to it; SAS_FULL_SORT is implied: the channels are
 *   composited from the complete tile lists) plus
 *   features  [H,W,channels] f32 device, required:  F[p,k] = sum_i vis_i f[i,k] (front to back) + (1 - alpha_p) fbg[k]
 *             with the weights vis_i of the frame's own compositing; NOT clamped.  For features in [0,1], clamp(F[..,3j:3j+3],
 *             0, 1) is bit-identical to the rgb of the scene recoloured with those three channels (sh_degree < 0, fbg = bg)
 *   feature_background [channels] host array, or NULL (zeros)
 *   Flags as sas_render (SAS_ASYNC, SAS_FAST_EXP, SAS_DEPTH_FILL_MAX, SAS_TIMING).  SAS_ERR_INVALID when no features are set
 *   for the current scene or `features` is NULL.
 */
int sas_scene_features(sas_ctx *ctx, int64_t n, int channels, const float *features);
int sas_render_features(sas_ctx *ctx, const float *viewmat, const float *K, int width, int height, const float *background,
                        const float *feature_background, unsigned flags, float *rgb, float *alpha, float *depth,
                        float *features, void *stream);

/*
 * Triangle meshes composited into every frame ("Meshes"): the task object and the robot's URDF visuals that the
 * reference's viser scene holds beside the splats (splat_handler.py:145-219) and poses at every draw message (:238-263,
 * :296-314).  sas_scene_meshes, after sas_scene_upload (a new upload forgets the meshes):
 *   vertices  [n_vertices,3] float32, mesh-local (the handle's scale applied); triangles [n_triangles,3] int32 vertex indices
 *   colors    [n_triangles,3] float32, one colour per triangle
 *   group     [n_triangles] uint8: the pose group ([n_groups,12] block of sas_set_group_poses / sas_set_link_poses / the pose
 *             sets of the *_posed calls) that moves the triangle; a scene without splat groups takes group 0, unposed
 *   ambient, diffuse: shading m = clamp(c (ambient + diffuse |n . v|), 0, 1), n the unit world-space face normal, v the unit
 *             ray from the camera centre to the triangle's centroid (ambient 1, diffuse 0: flat colour)
 *   All pointers host or device.  n_triangles == 0 clears the meshes.  SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID
 *   for an index out of range, a group >= max(n_groups, 1), or a non-finite ambient / diffuse.
 * Every render call then composites the meshes: per pixel the nearest triangle whose interior holds the pixel centre (depth
 * interpolated linear in 1/z, ties to the smaller (depth bits, triangle index), shared edges by a top-left rule, triangles
 * clipped at z = 0.01, non-finite or degenerate ones dropped) hides every splat at or behind its depth and takes the
 * background's place: rgb = clamp(C + T m).  alpha, depth and the RGB-D points / mask describe the splats in front of it,
 * unless the frame is rendered with SAS_MESH_SURFACE: then a pixel that shows a triangle of depth z_m has
 *   depth = fma(z_m, T, d) (the depth chain's own step, weight T) and alpha = 1.0f exactly,
 * the tile maximum, the SAS_DEPTH_FILL_MAX fill and the RGB-D tail take that depth, rgb / rgb8 and every pixel without a
 * triangle keep their bits.  The flag is accepted by sas_render, sas_render_rgbd, sas_render_batch[_posed] and
 * sas_render_features; it does nothing without meshes or in the *_host calls (rgb8 only).
 * Frames with meshes are SAS_FULL_SORT frames (batches take them one view at a time); sas_render_features refuses a context
 * with meshes (SAS_ERR_INVALID) until the meshes have feature rows:
 * sas_scene_mesh_features, after sas_scene_upload, sas_scene_meshes and sas_scene_features (each of which forgets the rows):
 *   features  [n_triangles,channels] float32, host or device, one row per triangle, through the colours' finite mapping and NOT
 *             shaded (ambient / diffuse belong to colours); NULL: one-hot of each triangle's pose group
 *   SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID without meshes, without a feature store, when n_triangles is not the
 *   meshes' or channels not the store's, or (one-hot) when a triangle's group is >= channels.  Frames in flight are completed first.
 * sas_render_features then renders the frame with its meshes (rgb / alpha / depth bit-identical to sas_render) and
 *   F[p,k] = sum_{i < cut(p)} vis_i f[i,k] + (1 - alpha_p) m[p,k],  m[p,k] = the row of the pixel's triangle, fbg[k] elsewhere,
 * cut(p) the first list entry at or behind the triangle: the frame's own compositing loop, triangle and stop rule.
 */
int sas_scene_meshes(sas_ctx *ctx, int64_t n_vertices, const float *vertices, int64_t n_triangles, const int32_t *triangles,
                     const float *colors, const uint8_t *group, float ambient, float diffuse);
int sas_scene_mesh_features(sas_ctx *ctx, int64_t n_triangles, int channels, const float *features);

/*
 * Vertex attributes of the meshes: smooth shading ("Meshes", rule 2b) -- what the reference hands viser for the
 * robot's URDF visuals (vertex normals and vertex colours, splat_handler.py:181-189).  After sas_scene_meshes:
 *   n_vertices  the uploaded meshes' vertex count (SAS_ERR_INVALID otherwise)
 *   normals     [n_vertices,3] float32 unit normals, mesh-local, or NULL; a zero or non-finite normal means "none"
 *   colors      [n_vertices,3] float32, or NULL: a smooth triangle takes its own colour at its three vertices
 *   Host or device pointers.  Both NULL clears the attributes and frees their device copies.
 * A triangle whose three vertices carry a normal is SMOOTH: per vertex s_k = clamp(c_k (ambient + diffuse |n'_k . v_k|), 0, 1),
 * n'_k the normal under the 3x3 block of the triangle's pose row, renormalised, v_k the unit ray from the camera centre to the
 * posed vertex; per pixel m = sum_k beta_k s_k with the perspective-correct barycentric coordinates of the ray's hit point
 * (s / z is affine in the pixel).  Every other triangle keeps the flat shade above.  Coverage, depth, ties, occlusion,
 * SAS_MESH_SURFACE and mesh feature rows are untouched: a smooth frame differs from the flat one in rgb / rgb8 only.
 * sas_scene_meshes and sas_scene_upload forget the attributes.  Frames in flight are completed first.
 */
int sas_scene_mesh_vertex_attributes(sas_ctx *ctx, int64_t n_vertices, const float *normals_or_null, const float *colors_or_null);

/*
 * Point-to-mesh queries ("Mesh queries"): for every (mesh, point) pair the unsigned distance to the mesh and the mesh's
 * generalised winding number at the point.  Serves the segmentation step that makes the per-link masks (match_splat.py:240-251:
 * per link mesh, occupancy > 0.5 or distance < 0.015 of every Gaussian centre).
 *   points        [n_points,3] float32; vertices [n_vertices,3] float32, ALREADY in the points' frame; triangles [n_triangles,3] int32
 *                 vertex indices: host or device pointers
 *   mesh_offsets  [n_meshes+1] HOST: mesh m owns triangles mesh_offsets[m] .. mesh_offsets[m+1]-1; non-decreasing, first 0, last
 *                 n_triangles; an empty mesh is allowed; 1 <= n_meshes <= 256
 *   max_distance  >= 0, INFINITY allowed: beyond it a distance need not be known (see culling)
 *   distance      [n_meshes,n_points] f32 DEVICE or NULL: Euclidean distance to the nearest point of any kept triangle of the mesh
 *   winding       [n_meshes,n_points] f32 DEVICE or NULL: sum_k Omega_k / (4 pi), Omega_k = 2 atan2(a . (b x c), |a||b||c| + (a . b)|c|
 *                 + (b . c)|a| + (c . a)|b|) the signed solid angle of triangle k from the point (a, b, c: its vertices minus the
 *                 point): 1 inside a closed mesh whose triangles are counter-clockwise seen from outside, 0 outside
 * Kept triangles: those with three finite vertices.  A zero-area triangle (its edge cross product is zero in float32) counts for the
 * distance with its three edges as segments, and for no solid angle.
 * Culling: a pair is culled exactly when the point lies outside the box of the mesh's kept triangles' vertices inflated by
 * max_distance -- p < lo - max_distance or p > hi + max_distance on some axis, in float32 -- when the mesh has no kept triangle, or
 * when a coordinate of the point is not finite.  A culled pair reads distance = +inf, winding = 0; max_distance = INFINITY culls by
 * the last two rules only.  No NaN is written.
 * Two calls with the same inputs return the same bits, and a pair's result does not depend on the other meshes or points of the call.
 * No scene is required and nothing the context stores is touched.  Frames in flight are completed first; the call returns with the
 * outputs in place (`stream`: the caller's, behind whose pending work the outputs are written).
 * SAS_ERR_INVALID: a vertex index out of range, bad offsets, n_meshes out of range, a negative or NaN max_distance, both outputs
 * NULL, a negative size or a missing array.  n_points == 0 is SAS_OK.
 */
int sas_query_meshes(sas_ctx *ctx, int64_t n_points, const float *points, int64_t n_vertices, const float *vertices,
                     int64_t n_triangles, const int32_t *triangles, int n_meshes, const int64_t *mesh_offsets, float max_distance,
                     float *distance, float *winding, void *stream);

/*
 * Nearest-neighbour matching of two point clouds, with the moments a closed-form similarity fit needs: the hot path of the ICP
 * registration (match_splat.py:208-223 runs open3d's registration_icp; sim_a_splat_amd/register.py runs the loop around this call).
 * DESIGN.md 3, "Point matching".
 *   source        [n_source,3] f32, host or device
 *   target        [n_target,3] f32, host or device
 *   transform     [12] HOST, row-major A|t (3x4: the upper rows of a 4x4), finite; NULL = identity.  Source point p is matched as
 *                 p' = A p + t, each component ((A_k0 x + A_k1 y) + A_k2 z) + t_k in float32, nothing fused
 *   max_distance  >= 0, INFINITY allowed: a match holds only if d2 <= max_distance * max_distance (the product in float32)
 *   slices        0: the library's choice; > 0: the target is searched in that many slices (clamped to its number of chunks of
 *                 SAS_MATCH_CHUNK = 256 targets).  No output depends on it
 *   index         [n_source] i32, host or device, or NULL: the matched target, -1 without a held match
 *   dist2         [n_source] f32, host or device, or NULL: d2 of the held match, +inf without one
 *   moments       [18] f64 HOST or NULL, over the held matches, from the float32 p', q and d2 widened: n, sum p' (3), sum q (3),
 *                 sum q p'^T (9, row-major), sum |p'|^2, sum d2
 * Per source point: d2 to target j = ((dx dx + dy dy) + dz dz), d = q_j - p', in float32.  A target whose d2 is not < INFINITY (a
 * non-finite coordinate, overflow) never matches, and a source with a non-finite p' has no match.  The match is the target with
 * the smallest d2, among equal d2 the lowest index.  No NaN is written.
 * Two calls with the same inputs return the same bits in all three outputs, and a point's result does not depend on the other
 * source points of the call nor on `slices`.  No scene is required and nothing the context stores is touched.  Frames in flight
 * are completed first; the call returns with the outputs in place (`stream`: the caller's).
 * SAS_ERR_INVALID: a negative size or one beyond 2^31 - 256, a missing array, a negative or NaN max_distance, a non-finite
 * transform, slices < 0, all three outputs NULL.  n_source == 0 is SAS_OK; n_target == 0 is SAS_OK with every index -1 and n = 0.
 */
int sas_match_points(sas_ctx *ctx, int64_t n_source, const float *source, int64_t n_target, const float *target,
                     const float *transform, float max_distance, int slices, int32_t *index, float *dist2, double *moments,
                     void *stream);

/*
 * Fixed-size point clouds from depth frames: the pixels of n_views same-sized views are unprojected, moved into an output frame,
 * cropped, thinned on a voxel grid and cut to n_points points per cloud by farthest-point sampling, with colour and label.  The
 * consumer behind sas_render_batch_labels: depth, rgb8 and labels are read where they are.  DESIGN.md 3, "Point clouds".
 *   depth       [n_views,H,W] f32 DEVICE
 *   rgb8        [n_views,H,W,3] u8 DEVICE or NULL;  labels  [n_views,H,W] u8 DEVICE or NULL
 *   Ks          [n_views,9] HOST, row-major (fx = K[0], cx = K[2], fy = K[4], cy = K[5]), finite, fx and fy > 0
 *   transform   [n_views,12] HOST, row-major A|t, camera -> output frame, any finite affine map; NULL = identity
 *   cloud       [n_views] HOST, the cloud in [0,n_clouds) a view feeds; NULL: every view feeds cloud 0
 *   keep        [256] HOST or NULL: with labels, a pixel is looked at only if keep[labels[p]] != 0
 *   bounds      [6] HOST lo[3], hi[3] (lo <= hi) or NULL;  voxel >= 0 (0: no grid; > 0 needs bounds);  stride >= 1
 *   flags       SAS_TIMING only: sas_stage_times then reads the call's kernels, k_cloud_mark as SAS_T_PROJECT, the compaction as
 *               SAS_T_SCATTER, k_cloud_fps as SAS_T_BLEND, all of them as SAS_T_TOTAL (the other slots 0)
 *   points      [n_clouds,n_points,3] f32, index [n_clouds,n_points] i32, colors [n_clouds,n_points,3] u8 (needs rgb8), labels_out
 *               [n_clouds,n_points] u8 (needs labels), count [n_clouds] i32: DEVICE, in pick order; any but index may be NULL
 * Per pixel, flat index p = (c H + v) W + u, all arithmetic float32 with nothing fused:
 *   stride      only u % stride == 0 and v % stride == 0 are looked at
 *   candidate   d = depth[p] with d > 0 and d < INFINITY (a NaN, 0, a negative and Inf drop out), and the keep rule
 *   camera      x = ((float)u - cx) d / fx, y = ((float)v - cy) d / fy, z = d: the bits of sas_render_rgbd's points
 *   output      w_k = ((A_k0 x + A_k1 y) + A_k2 z) + t_k; a candidate with a non-finite w drops out
 *   crop        with bounds: lo_k <= w_k <= hi_k for every k
 *   voxel grid  n_k = max(1, (int)ceilf((hi_k - lo_k) / voxel)), n_x n_y n_z <= 2^24; cell i_k = min((int)floorf((w_k - lo_k) /
 *               voxel), n_k - 1); of a cloud's candidates in one cell the one with the lowest p survives
 *   order       a cloud's survivors sorted by p have ranks 0 .. M - 1; count = M
 *   sampling    pick 0 is rank 0; dist_i starts at +inf; after a pick s, dist_i = fminf(dist_i, (dx dx + dy dy) + dz dz), d = w_i -
 *               w_s; the next pick is the unpicked survivor with the largest dist, among equals the lowest rank; min(n_points, M)
 *               picks.  Rows beyond them are padding: points 0, index -1, colors 0, labels_out 255
 * A cloud's result depends on its own views' pixels only; the first K' rows of a K-point result are the K'-point result; two calls
 * return the same bytes.  No scene is required and nothing else the context stores is touched.  Frames in flight are completed
 * first; the call returns with the outputs in place (`stream`: the caller's, behind whose pending work the inputs are read).
 * SAS_ERR_INVALID: a negative size, an image size <= 0 or n_views H W > 2^31 - 256 (n_views > 65535), n_points < 0, stride < 1,
 * n_clouds < 1, a cloud[v] out of range, a non-finite transform or K entry, fx or fy not > 0, lo_k > hi_k, a NaN, infinite or negative
 * voxel, voxel > 0 without bounds, a grid of more than 2^24 cells, a missing depth, Ks or index, colors without rgb8, labels_out
 * without labels, any other flag.  n_points == 0 and n_views == 0 are SAS_OK (no view: every count 0, all rows padding).
 */
int sas_sample_points(sas_ctx *ctx, int n_views, int width, int height, const float *depth, const uint8_t *rgb8,
                      const uint8_t *labels, const float *Ks, const float *transform, const int32_t *cloud, int n_clouds,
                      const uint8_t *keep, const float *bounds, float voxel, int stride, int n_points, unsigned flags,
                      float *points, int32_t *index, uint8_t *colors, uint8_t *labels_out, int32_t *count, void *stream);

/*
 * Depth fusion: n_views same-sized depth frames are integrated, in view order, into a truncated-signed-distance (TSDF) volume the
 * CALLER owns as device arrays.  The consumer behind sas_render_batch_labels that gives a splat geometry: a surface is extracted from
 * the volume on the host (sim_a_splat_amd.reconstruct.surface_nets).  DESIGN.md 3, "Depth fusion".
 *   depth       [n_views,H,W] f32 DEVICE
 *   rgb8        [n_views,H,W,3] u8 DEVICE or NULL;  labels  [n_views,H,W] u8 DEVICE or NULL
 *   Ks          [n_views,9] HOST, row-major (fx = K[0], cx = K[2], fy = K[4], cy = K[5]), finite, fx and fy > 0
 *   transform   [n_views,12] HOST, row-major A|t, VOLUME frame -> camera, any finite affine map (a similarity such as the robot
 *               frame folds in); NULL = identity.  trunc and near_z are in camera units
 *   keep        [256] HOST or NULL (needs labels): a pixel with keep[labels[p]] == 0 shows something else -- it carves, see below
 *   lo, voxel, dims   the volume: dims = (nx, ny, nz), each in [1,1024], nx ny nz <= 2^27; voxel (i,j,k) has flat index
 *               g = (k ny + j) nx + i and centre c_x = lo_x + ((float)i + 0.5f) voxel, likewise y and z
 *   pixel_centre  0.5: where the rasterizer samples a pixel; 0: the convention of sas_render_rgbd's points
 *   flags       SAS_TIMING only: sas_stage_times then reads the call's launches as SAS_T_BLEND and SAS_T_TOTAL (the other slots 0)
 *   tsdf, weight  [nz,ny,nx] f32 DEVICE, in/out;  color  [nz,ny,nx,3] f32 DEVICE in/out, or NULL (needs rgb8 when given)
 * Per voxel, for the views v = 0 .. n_views - 1 in ascending order, all arithmetic float32 with nothing fused:
 *   camera      q_m = ((A_m0 c_x + A_m1 c_y) + A_m2 c_z) + t_m
 *   in front    q_z >= near_z (near_z > 0), else the view is skipped for this voxel
 *   pixel       uf = ((fx (q_x / q_z)) + cx) - pixel_centre, then uf = uf + 0.5f; vf likewise from fy, q_y, cy.  The voxel proceeds
 *               only if uf >= 0 && uf < (float)W && vf >= 0 && vf < (float)H (a NaN fails; tested before any conversion); then
 *               u = (int)floorf(uf), v = (int)floorf(vf), p = (view H + v) W + u
 *   depth       d = depth[p] with d > 0 and d < INFINITY (a NaN, 0, a negative and Inf skip the view)
 *   distance    sdf = d - q_z
 *   surface     (no labels, no keep, or keep[labels[p]] != 0)  sdf < -trunc: skip; else val = fminf(1.0f, sdf / trunc)
 *   carving     (keep[labels[p]] == 0)  sdf >= trunc: val = 1.0f; else skip
 *   update      w = weight[g]; tsdf[g] = ((tsdf[g] w) + val) / (w + 1.0f); with color, on a surface update, every channel
 *               col = ((col w) + (float)rgb8[3 p + ch]) / (w + 1.0f) (a carving update leaves the colour); weight[g] = fminf(w + 1.0f,
 *               max_weight)
 * A voxel's result depends on its own pixels only; one call with views 0 .. C - 1 returns the bytes of C one-view calls in that
 * order; two equal calls on equal volumes return equal bytes; a voxel no view updates keeps its bytes (a NaN the caller left there
 * included).  No atomics.  No scene is required and nothing the context stores is touched.  Frames in flight are completed first; the
 * call returns with the volume updated (`stream`: the caller's, behind whose pending work the inputs are read).
 * SAS_ERR_INVALID: a negative n_views, an image size <= 0 or n_views H W > 2^31 - 256, a dims entry < 1 or > 1024 or nx ny nz > 2^27,
 * a non-finite lo, transform or K entry, fx or fy not > 0, voxel, trunc, near_z or max_weight not finite and > 0, max_weight < 1, a
 * non-finite pixel_centre, keep without labels, color without rgb8, a missing depth, Ks, tsdf or weight, any other flag.
 * n_views == 0 is SAS_OK and changes nothing.
 */
int sas_fuse_depth(sas_ctx *ctx, int n_views, int width, int height, const float *depth, const uint8_t *rgb8,
                   const uint8_t *labels, const float *Ks, const float *transform, const uint8_t *keep, const float lo[3],
                   float voxel, const int dims[3], float trunc, float near_z, float pixel_centre, float max_weight,
                   unsigned flags, float *tsdf, float *weight, float *color, void *stream);

/*
 * Render n_views views of the same size in one call.  Serves the per-camera loops of
 * SplatHandler.render / SplatEnvWrapper.render (splat_handler.py:337-345, splat_env_wrapper.py:147-158).
 *   viewmats [n_views,16], Ks [n_views,9] host arrays; outputs are [n_views,H,W,...] device arrays
 *   (any may be NULL).  Scenes of >= 0.5 M Gaussians: the views go through the frame slots two at a time, a pair
 * sharing one projection pass over the scene, consecutive pairs overlapping on the GPU.  Smaller scenes: launch
 * groups of (by default) two views that share every launch -- one projection, one scatter, one tile kernel with the
 * views interleaved in dispatch order.  The call returns when all views are complete unless SAS_ASYNC is given (then
 * see SAS_ASYNC: views complete in order inside later calls).
 */
int sas_render_batch(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, int width, int height,
                     const float *background, unsigned flags, float *rgb, float *alpha, float *depth,
                     uint8_t *rgb8, void *stream);

/*
 * sas_render_batch for frames that are wanted on the HOST: get_render returns np.uint8 arrays
 * (splat_handler.py:339-344, splat_env_wrapper.py:148-157).  rgb8_host [n_views,H,W,3] is HOST memory (pinned --
 * hipHostMalloc, torch pin_memory -- for speed; pageable memory works through the runtime's staging).  When
 * width and height are multiples of 16 and the destination is pinned, the tile kernel stores each finished tile
 * straight into rgb8_host (its rows packed in LDS, 16 B per lane); otherwise the frames are rendered into a
 * staging buffer of the context and copied out on the frames' own streams right behind the tile kernels.  Either
 * way the call returns with the pixels in place and no second round trip (device-to-host copy issued by the
 * caller after the frame) is needed.  Blocking only (SAS_ASYNC is rejected).  Nothing of the caller's on the device is
 * read or written, so the frames are NOT ordered against work pending on `stream` (two event records and two
 * stream waits per step that a 120-microsecond Gym step notices: docs/EXPERIMENTS.md 5.34).
 */
int sas_render_batch_host(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, int width, int height,
                          const float *background, unsigned flags, uint8_t *rgb8_host, void *stream);

/*
 * sas_render_batch / sas_render_batch_host with PER-VIEW pose sets: view v is rendered with the group poses
 * Rt[pose_set[v]] ([n_sets, n_groups, 12] row-major (R|t), host).  Serves vectorised Gym rollouts -- E envs, each with
 * its own link poses, C cameras per env (splat_env_wrapper.py:121-159 poses the scene per env step): one call renders
 * all E*C views, nothing drains between envs, and views of different envs may share a launch group.  The context's
 * current poses (sas_set_group_poses) are not changed.
 */
int sas_render_batch_posed(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, const int *pose_set,
                           int n_sets, const float *Rt, int width, int height, const float *background, unsigned flags,
                           float *rgb, float *alpha, float *depth, uint8_t *rgb8, void *stream);
int sas_render_batch_host_posed(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, const int *pose_set,
                                int n_sets, const float *Rt, int width, int height, const float *background,
                                unsigned flags, uint8_t *rgb8_host, void *stream);

/*
 * Label frames: sas_render_batch[_posed] plus, for every view, which pose group (robot link, mesh) each pixel shows, as one byte
 * per pixel.  Serves the per-link segmentation a policy observes beside rgb and depth (splat_handler.py:62-83 makes the link
 * groups; splat_env_wrapper.py:147-158 is the per-camera loop the observation comes from).  The contract, for every view v and
 * pixel p:
 *     labels[v,p] = L(w_v[p,:], a_v[p])
 * where w_v [G] and a_v are bit for bit the features and alpha sas_render_features delivers for that view under that view's poses
 * with the one-hot stores -- sas_scene_features(NULL) and, when the context holds meshes, sas_scene_mesh_features(NULL) -- a zero
 * feature background and the call's flags (SAS_MESH_SURFACE included), and L is the smallest g with w_g == max_k w_k, clamped to
 * 255, and 255 where a < min_alpha (a float32 compare).  G is the store's channel count (the scene's n_groups, 1..256); with 256
 * groups, group 255 reads as "none".  No [H,W,G] array is written anywhere.
 *   labels     [n_views,H,W] uint8 DEVICE, required
 *   min_alpha  0 never labels a pixel 255 by the alpha rule
 *   rgb / alpha / depth / rgb8: optional, as sas_render_batch[_posed], and bit-identical to it with the same flags
 *   flags      SAS_MESH_SURFACE, SAS_DEPTH_FILL_MAX, SAS_FAST_EXP, SAS_TIMING; blocking only (SAS_ASYNC is rejected); any other
 *              flag is SAS_ERR_INVALID.  n_views == 1 is the single-view call.
 * The call selects no store itself: SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID without a feature store, with a store of
 * the caller's own features, with meshes that lack their one-hot rows, or without `labels` (sas_last_error says which).
 * Label frames are SAS_FULL_SORT frames: the views go through the frame slots one at a time, each with a snapshot of its own
 * pose set; nothing drains between views and the context's current poses are not changed.
 */
int sas_render_batch_labels(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, int width, int height,
                            const float *background, float min_alpha, unsigned flags, float *rgb, float *alpha, float *depth,
                            uint8_t *rgb8, uint8_t *labels, void *stream);
int sas_render_batch_labels_posed(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, const int *pose_set,
                                  int n_sets, const float *Rt, int width, int height, const float *background, float min_alpha,
                                  unsigned flags, float *rgb, float *alpha, float *depth, uint8_t *rgb8, uint8_t *labels,
                                  void *stream);

/*
 * Label lifting: the transpose of a label frame, pixel -> Gaussian.  Serves per-Gaussian masks for objects without a mesh
 * (splat_handler.py:62-83 takes {"link": bool[N]}): label a few images, push the labels back through the renderer.  The contract:
 * for view v, pixel p inside the image, and every list entry i (a Gaussian, in the CALLER's order) that the frame's compositing ADDS
 * at p, let vis be the float32 weight -- the same weight that multiplies the colours in sas_render and the channels in
 * sas_render_features, under the context's current group poses and the call's flags -- and
 *     q = (int64) floorf(vis * 2^32)          (SAS_LIFT_ONE; the product is exact in float32 and 0 <= vis < 1).
 * Then seen[i] += q and, if labels[v,p] < n_labels, votes[i, labels[v,p]] += q.  Nothing is added for: entries skipped for
 * alpha < 1/255 or sigma < 0; the entry that trips T' <= 1e-4 and everything behind it; pixels of a ragged tile beyond W or H;
 * labels >= n_labels (so 255 means "unlabelled" for every n_labels <= 255).
 *   labels    [n_views,H,W] uint8 DEVICE, required
 *   n_labels  1..256
 *   votes     [N,n_labels] int64 DEVICE, or NULL
 *   seen      [N] int64 DEVICE, or NULL; at least one of votes and seen
 *   flags     SAS_FAST_EXP and SAS_TIMING only.  The call is blocking: SAS_ASYNC and every other flag is SAS_ERR_INVALID.
 * The call ADDS to what the buffers hold: the caller zeroes them once and may accumulate over many calls.  The sums are integers,
 * so the result does not depend on any order of addition: two calls with the same inputs give the same bits, and n_views views in
 * one call equal the same views one call each.  No overflow occurs while the pixels accumulated into one buffer (sum of W*H over
 * the views) stay below 2^31; the call does not check it.
 * Frames in flight are completed first.  Lift frames are SAS_FULL_SORT frames, one view at a time through the frame slots, as label
 * frames are.  SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID for n_labels out of range, missing labels, both outputs NULL,
 * n_views < 1, non-positive sizes, or a context that holds meshes (occlusion by meshes is not lifted: clear the meshes first).
 * After any error the context stays usable.
 */
#define SAS_LIFT_ONE 4294967296.0f   /* 2^32: the fixed-point unit of a vote */
int sas_lift_labels(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, int width, int height,
                    const uint8_t *labels, int n_labels, unsigned flags, int64_t *votes, int64_t *seen, void *stream);

/*
 * Feature lifting: sas_lift_labels with `channels` real-valued channels in one label's place -- per-Gaussian embeddings from the
 * feature maps (DINO / CLIP patch features, or colours) of a few views, each Gaussian taking the compositing-weighted mean of the
 * pixels it shows in.  The contract: for view v, pixel p inside the image, and every list entry i (a Gaussian, in the CALLER's
 * order) that the frame's compositing ADDS at p, let vis be the float32 weight that multiplies the colours in sas_render, under the
 * context's current group poses and the call's flags, and
 *     q         = (int64) floorf(vis * 2^24)          (SAS_LIFT_FEATURE_ONE; the product is exact in float32 and 0 <= vis < 1)
 *     fq[v,p,k] = (int32) rintf(min(max(images[v,p,k] * feature_scale, -32767), 32767))
 *                 (the float32 product, rounded half to even; NaN -> 0, +-Inf -> +-32767).
 * Then, where mask is NULL or mask[v,p] != 0:  weight[i] += q  and  sums[i,k] += q * fq[v,p,k] for k < channels.  Nothing is added
 * for: entries skipped for alpha < 1/255 or sigma < 0; the entry that trips T' <= 1e-4 and everything behind it; pixels of a ragged
 * tile beyond W or H; pixels whose mask is 0.  The weighted mean of Gaussian i is sums[i,k] / (weight[i] * feature_scale).
 *   images         [n_views,H,W,channels] float32 DEVICE, required
 *   channels       1..256
 *   feature_scale  finite, > 0: what one unit of the features is worth in fq (32767 / max|f| uses the whole range)
 *   mask           [n_views,H,W] uint8 DEVICE, or NULL
 *   sums           [N,channels] int64 DEVICE, or NULL
 *   weight         [N] int64 DEVICE, or NULL; at least one of sums and weight
 *   flags          SAS_FAST_EXP and SAS_TIMING only.  The call is blocking: SAS_ASYNC and every other flag is SAS_ERR_INVALID.
 * The call ADDS to what the buffers hold: the caller zeroes them once and may accumulate over many calls (with ONE feature_scale).
 * The sums are integers, so the result does not depend on any order of addition or batching of views and calls.
 * |sums[i,k]| <= 32767 * weight[i], so no sum can have overflowed while weight[i] < 2^48: check weight afterwards (it cannot wrap
 * before 2^63 itself) instead of budgeting pixels in advance; the call does not check it.
 * Frames in flight are completed first.  Lift frames are SAS_FULL_SORT frames, one view at a time through the frame slots; a frame
 * whose first rendering outgrew its key buffer adds nothing until it is rendered again.  SAS_ERR_NO_SCENE before an upload;
 * SAS_ERR_INVALID for channels or feature_scale out of range, images NULL, both outputs NULL, n_views < 1, non-positive sizes, any
 * other flag, or a context that holds meshes.  After any error the context stays usable.
 */
#define SAS_LIFT_FEATURE_ONE 16777216.0f   /* 2^24: the fixed-point unit of a feature-lift weight */
int sas_lift_features(sas_ctx *ctx, int n_views, const float *viewmats, const float *Ks, int width, int height,
                      const float *images, int channels, float feature_scale, const uint8_t *mask, unsigned flags,
                      int64_t *sums, int64_t *weight, void *stream);

/*
 * Backward pass of one view's compositing, in screen space ("Backward pass").  Given the gradients of a loss with
 * respect to the frame's RAW accumulators per pixel --
 *   g_rgb    [H,W,3] float32 DEVICE or NULL: of  sum_i c_i alpha_i T_i        (sas_render's rgb before background and clamp)
 *   g_alpha  [H,W]   float32 DEVICE or NULL: of  1 - T_final
 *   g_depth  [H,W]   float32 DEVICE or NULL: of  sum_i z_i alpha_i T_i        (sas_render's depth before the division by alpha)
 * -- the call ADDS, for every Gaussian i in the CALLER's order, the gradients with respect to what the projection hands the tile
 * kernel (contract T2/T3): d_means2d [N,2], d_conics [N,3] (a, b, c), d_opacities [N], d_colors [N,3] (the SH colour after its
 * clamp, or the uploaded colour), d_depths [N]; float32 DEVICE, each may be NULL, not all.  With contract T6's
 *   sigma = (a dx^2 + c dy^2) / 2 + b dx dy,   alpha = min(0.999, o e^-sigma),   w_i = alpha_i T_i,
 *   S_i = sum_{j>i} w_j (c_j . g_rgb + z_j g_depth):
 *   dL/dalpha_i = T_i (c_i . g_rgb + z_i g_depth) - S_i / (1 - alpha_i) + g_alpha T_final / (1 - alpha_i)
 *   dL/dsigma_i = -alpha_i dL/dalpha_i,   dL/do_i = e^-sigma_i dL/dalpha_i,   d_colors_i += w_i g_rgb,   d_depths_i += w_i g_depth.
 * Decisions are constants of the derivative: an entry skipped for alpha < 1/255 or sigma < 0, the entry that trips
 * T (1 - alpha) <= 1e-4 and everything behind it, and culled Gaussians receive nothing; a clamped alpha (o e^-sigma > 0.999) passes
 * nothing to o, the conic or the mean.  The sums over pixels are float32 atomic additions: they vary in their last bits from run
 * to run (the lift calls' integer exactness is NOT promised here).  Gradients with respect to K and to mesh vertices are not
 * computed; those of the group poses come from sas_render_backward_poses.
 *   flags   SAS_FAST_EXP and SAS_TIMING only.  Blocking, one view per call; several views sum by calling again on the same buffers.
 * The frame is a SAS_FULL_SORT frame like a lift frame's: frames in flight are completed first, a frame that outgrew its key buffer
 * adds nothing until it is rendered again, the context's current group poses apply.  SAS_ERR_NO_SCENE before an upload;
 * SAS_ERR_INVALID for all three gradients NULL, all outputs NULL, non-positive sizes, any other flag, or a context that holds meshes.
 */
int sas_render_backward_screen(sas_ctx *ctx, const float *viewmat, const float *K, int width, int height, unsigned flags,
                               const float *g_rgb, const float *g_alpha, const float *g_depth, float *d_means2d, float *d_conics,
                               float *d_opacities, float *d_colors, float *d_depths, void *stream);

/*
 * ... and chained through the view's projection (contract T1 / T2), cull and clamp decisions as constants: the pinhole EWA Jacobian
 * (its tx / ty clamp a constant where it binds), Sigma2 = J Sigma_c J^T + 0.3 I, the conic as its inverse, mean2d, the depth,
 * Sigma_c = R Sigma3 R^T, the group pose of posed groups, and the SH colour max(SH(d) . coeffs + 0.5, 0) with
 * d = normalize(mean - campos), through d to the mean and to the camera position.  The call ADDS, in the CALLER's order and with
 * respect to the arrays last uploaded (the canonical ones: before any group pose):
 *   d_means [N,3], d_opacities [N], d_sh [N,(L+1)^2,3] ([N,3] for a scene of plain colours),
 *   d_quats [N,4] (the quaternion as uploaded, not normalised) and d_scales [N,3] -- or d_cov6 [N,6] (xx xy xz yy yz zz, each of the
 *   six taken as one variable), whichever form the scene was uploaded in; asking for the other form is SAS_ERR_INVALID,
 *   d_viewmat [3,4] row-major rows [R | t] of the view matrix, its twelve entries taken as independent, summed over the Gaussians
 *   in a fixed order (no atomics): reproducible given the screen-space sums.
 * float32 DEVICE, each may be NULL, not all.  A culled Gaussian receives exact zeros.  NOT differentiated: K, mesh vertices, joint
 * angles, and every decision (culls, the radius' ceil, the tile rectangle, the compositing thresholds); the group poses themselves
 * are differentiated by sas_render_backward_poses, which this call is with n_sel = 0.
 * Everything else is as in sas_render_backward_screen, whose sums this call keeps in scratch of the context.
 */
int sas_render_backward(sas_ctx *ctx, const float *viewmat, const float *K, int width, int height, unsigned flags,
                        const float *g_rgb, const float *g_alpha, const float *g_depth, float *d_means, float *d_opacities,
                        float *d_sh, float *d_quats, float *d_scales, float *d_cov6, float *d_viewmat, void *stream);

/*
 * ... and to the poses of up to SAS_MAX_POSE_GRAD_GROUPS splat groups: sel [n_sel] uint8 HOST names distinct group ids, and the call
 * ADDS to d_group_poses [n_sel,12] float32 DEVICE, in sel's order, the gradient with respect to the rows [R | t] of each named group's
 * current pose (sas_set_group_poses / sas_set_link_poses), its twelve entries taken as independent, exactly as d_viewmat treats the
 * view matrix:  dL/dt = sum_i gm_i,  dL/dR = sum_i gm_i m0_i^T + 2 GSw_i R S0_i  over the group's Gaussians, gm the gradient of the
 * posed mean (the SH direction term included), GSw that of the posed covariance, m0 and S0 the canonical mean and covariance.  A culled
 * Gaussian adds exact zeros, a group whose Gaussians are all culled gets a zero row, groups that are not named are not reduced.  The
 * sums run in a fixed order without atomics: reproducible given the screen-space sums.  d_group_poses alone, every other output NULL,
 * is a valid call; more than 32 groups: call again with the next 32.  Everything else is sas_render_backward.  SAS_ERR_INVALID also
 * for n_sel outside 0..SAS_MAX_POSE_GRAD_GROUPS, n_sel > 0 with sel or d_group_poses NULL, a duplicate id, an id >= n_groups, and a
 * scene uploaded without group ids.  After any error the context stays usable.
 */
#define SAS_MAX_POSE_GRAD_GROUPS 32
int sas_render_backward_poses(sas_ctx *ctx, const float *viewmat, const float *K, int width, int height, unsigned flags,
                              const float *g_rgb, const float *g_alpha, const float *g_depth, float *d_means, float *d_opacities,
                              float *d_sh, float *d_quats, float *d_scales, float *d_cov6, float *d_viewmat,
                              int n_sel, const uint8_t *sel /* host */, float *d_group_poses /* device [n_sel,12] */, void *stream);

/*
 * Optimiser step on the resident scene ("Optimiser step"): one fused Adam update, in place, of the planes the frames read.
 * The gradients are what sas_render_backward writes -- float32 DEVICE arrays in the CALLER's order, with respect to the activated arrays
 * last uploaded; summed over as many views as the caller likes -- and each may be NULL.
 *   VARIABLES  means [N,3]; log(scales) [N,3]; logit(opacities) [N]; quats [N,4] as uploaded (not normalised); the SH coefficients
 *              [N,(L+1)^2,3] (or the plain colour [N,3]), whose DC triple steps with lr_sh_dc and the rest with lr_sh_rest.  The
 *              gradients are chained through the activations: d_logit = d_o o (1 - o), d_logscale = d_s s, per element.
 *   FIXED      the covariances of a scene uploaded as cov6 (d_quats or d_scales is then SAS_ERR_INVALID; means, opacities and colours
 *              step), the group ids, N and the storage order, and a group whose gradient is NULL or whose learning rate is 0: it is
 *              neither read nor written and holds no state.  An opacity outside (0, 1), and a scale component that is not a positive
 *              finite number, have no raw value: they stay as they are.
 *   UPDATE     per element, with t = step (1-based), all in float32:  m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,
 *              x -= lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps);  then scales = exp, opacities = 1 / (1 + exp(-x)).
 *              A non-finite gradient element (after the chain) leaves its variable and both moments untouched.
 *              SAS_ADAM_VISIBLE_ONLY: a Gaussian whose gradient is an exact zero in every stepped array is skipped whole -- the
 *              backward pass gives exact zeros to culled Gaussians, so momentum does not drag what no view of the batch saw.
 *   STATE      the moments, log(scale) and logit(opacity) belong to the context, in storage order, allocated for a group the first
 *              time it is stepped (the raw values then come from the resident ones; later steps never invert an activation).
 *              sas_scene_upload and sas_scene_adam_reset drop it; the caller owns the step count.
 * The call completes the frames in flight, then only enqueues on `stream` (behind whatever produced the gradients there); frames
 * submitted afterwards run behind the step.  No host copy, no sort, no device-wide synchronisation.  It INVALIDATES the last frame:
 * sas_read_projection and sas_read_tile_lists report SAS_ERR_NO_SCENE until a frame has been rendered again.  Features, meshes, group
 * poses and link constants stay.  SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID for cfg NULL, every gradient NULL, step < 1, a
 * negative or non-finite learning rate, beta outside [0, 1), a negative or non-finite eps, an unknown flag, d_quats or d_scales on a
 * cov6 scene.
 */
#define SAS_ADAM_VISIBLE_ONLY 1u
typedef struct sas_adam_config {
    float lr_means, lr_opacities, lr_sh_dc, lr_sh_rest, lr_quats, lr_scales;
    float beta1, beta2, eps;
    int step;         /* 1-based */
    unsigned flags;   /* SAS_ADAM_VISIBLE_ONLY */
} sas_adam_config;
int sas_scene_adam_step(sas_ctx *ctx, const sas_adam_config *cfg, const float *d_means, const float *d_opacities, const float *d_sh,
                        const float *d_quats, const float *d_scales, void *stream);

/* Free the optimiser state: the next step of a group starts from zero moments and the resident values.  Frames in flight are completed. */
int sas_scene_adam_reset(sas_ctx *ctx);

/*
 * Density control on the resident scene ("Density control"): the adaptive densification, pruning and opacity reset of 3DGS
 * training (Kerbl et al. 2023) in the form of gsplat's default strategy, with the optimiser state carried along.
 *
 * STATISTICS are the caller's: float32 / int32 DEVICE arrays of N entries in the CALLER's order, zeroed by the caller, ADDED to.
 * sas_density_accumulate adds, for every Gaussian i the last backward frame saw (radius > 0),
 *   grad_sum[i] += sqrt((0.5 W du)^2 + (0.5 H dv)^2),   count[i] += 1,   max_radius[i] = max(max_radius[i], radius),
 * radius the larger of the two pixel radii sas_read_projection reports.  (du, dv) = d_means2d_or_null [N,2] (float32 DEVICE), what
 * sas_render_backward_screen wrote for that frame; NULL: the screen-space sums the last sas_render_backward left in the context's scratch.
 * IEEE binary32, nothing fused, correctly rounded sqrt, one add per call.  The call only enqueues on `stream`; frames submitted
 * afterwards run behind it.  SAS_ERR_NO_SCENE when no backward frame has been made since the last upload, optimiser step, densify or
 * opacity reset (or any other frame was rendered since), and for NULL d_means2d when that frame came from sas_render_backward_screen.
 */
int sas_density_accumulate(sas_ctx *ctx, int width, int height, const float *d_means2d_or_null, float *grad_sum, int32_t *count,
                           float *max_radius_or_null, void *stream);

/*
 * sas_scene_densify replaces the resident scene of N Gaussians by one of N_new.  Every decision is made on the OLD set, per Gaussian:
 *   avg = grad_sum / max(count, 1);  high = count > 0 && avg > grow_grad2d;  small = max(scale) <= grow_scale3d * scene_extent;
 *   prune_o = opacity < prune_opacity;  prune_s = max(scale) > prune_scale3d * scene_extent;
 *   PRUNED  prune_o || (prune_s && !(high && !small))      CLONED  high && small && !pruned      SPLIT  high && !small && !pruned
 * (a flag that is not set makes its test false: SAS_DENSIFY_GROW high, SAS_DENSIFY_PRUNE_OPACITY prune_o, SAS_DENSIFY_PRUNE_SCALE
 * prune_s).  The new scene, in the new caller's order: the survivors (neither pruned nor split) in their old order; one clone per cloned
 * Gaussian, in parent order, a bit-identical copy; two adjacent children per split Gaussian, in parent order:
 *   mean + R(q / |q|) (scale * xi),  scale / split_factor,  quaternion, opacity, coefficients and group id inherited bit for bit,
 * xi three standard normals of the counter-based generator of DESIGN.md, keyed by (seed, the parent's old index, child, axis).
 * max_gaussians > 0: the growth candidates are ranked clones first, then splits, each by parent index; those whose rank is beyond
 * max_gaussians - (N - pruned) stay as they are, as survivors.
 *   OPTIMISER STATE  survivors keep moments and raw values bit for bit; clones and children get zero moments and, where a group has raw
 *                    values, fresh ones from their new resident values.  Groups never stepped stay without state.
 *   parents_out_or_null  int32 DEVICE with room for 2 N entries (the most a call can make); [0, N_new) <- each new Gaussian's old index.
 *   counts_out       HOST: (N_new, cloned, split, pruned).
 * The storage order is computed anew from the new means (so a call that changes nothing renews it, state kept).  Group poses, link
 * constants, meshes and sh_degree stay; the feature store and the last frame are dropped as an upload drops them -- upload
 * features[parents] again; the statistics arrays have the old length: make new ones.  Blocking; completes the frames in flight.
 * SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID for cfg / grad_sum / count / counts_out NULL, unknown flags, a negative or
 * non-finite threshold, scene_extent <= 0, split_factor <= 1, max_gaussians < 0, SAS_DENSIFY_GROW or SAS_DENSIFY_PRUNE_SCALE on a cov6
 * scene (it has no scales), an empty scene, and N_new == 0: pruning everything is refused and the scene stays as it is.
 */
#define SAS_DENSIFY_GROW 1u
#define SAS_DENSIFY_PRUNE_OPACITY 2u
#define SAS_DENSIFY_PRUNE_SCALE 4u
typedef struct sas_densify_config {
    float grow_grad2d, grow_scale3d, prune_opacity, prune_scale3d, scene_extent;
    float split_factor;       /* 1.6 */
    int64_t max_gaussians;    /* 0: no cap */
    unsigned seed;
    unsigned flags;           /* SAS_DENSIFY_* */
} sas_densify_config;
int sas_scene_densify(sas_ctx *ctx, const sas_densify_config *cfg, const float *grad_sum, const int32_t *count,
                      int32_t *parents_out_or_null, int64_t counts_out[4], void *stream);
/* Host clock of the last successful sas_scene_densify, ms[0..n) of: the classes and their totals' read-back; the scatter's enqueue; the
 * storage order's enqueue; allocation, relayout, state and commit, whose wait is the first behind the scatter's and the order's kernels
 * (tools/densify_probe.py).  Under SAS_ORDER=0 (the storage order on the host) ms[1] ends behind the read-back of the new means and group
 * ids and ms[2] is the host sort. */
int sas_scene_densify_times(sas_ctx *ctx, float *ms, int n);

/*
 * Every opacity > max_opacity becomes max_opacity (the published reset: min(o, 0.01)); where the opacities have optimiser state, the
 * raw logit of a changed Gaussian is set anew and both its moments are zeroed.  Only enqueues on `stream`, behind the frames in flight;
 * invalidates the last frame as sas_scene_adam_step does.  SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID unless 0 < max_opacity < 1.
 */
int sas_scene_reset_opacity(sas_ctx *ctx, float max_opacity, void *stream);

/*
 * MCMC density control on the resident scene ("MCMC density control"): the strategy of "3D Gaussian Splatting as Markov
 * Chain Monte Carlo" (Kheradmand et al. 2024) in the form of gsplat's MCMCStrategy -- the number of Gaussians is a budget.  It needs no
 * gradient statistics.
 *
 * sas_scene_mcmc_noise moves every mean by noise shaped by the Gaussian's own covariance and switched off by its opacity.  For the
 * Gaussian with CALLER's index i, all in float32, nothing fused:
 *   g = 1 / (1 + expf(-100 ((1 - o) - 0.995)))        (an overflow of expf makes g exactly 0: the mean keeps its bits)
 *   n_k = (xi_k g) scale,   xi three standard normals of the counter-based generator keyed by (seed, step, i, axis)
 *   mean_k += (C_k0 n_0 + C_k1 n_1) + C_k2 n_2,   C = M M^T, M = R(q / |q|) diag(s); for a scene uploaded as cov6, C is the stored one.
 * The key holds the caller's index, never the slot: the result does not depend on the storage order.  Only the means change; the
 * optimiser state is not touched.  The call only enqueues on `stream`, behind the frames in flight; it invalidates the last frame as
 * sas_scene_adam_step does.  scale == 0 changes nothing.  SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID for a negative or
 * non-finite scale and for step < 1.
 */
int sas_scene_mcmc_noise(sas_ctx *ctx, float scale, int step, unsigned seed, void *stream);

/*
 * sas_scene_mcmc_refine replaces the resident scene of N Gaussians by one of N_new = N + n_grow: dead Gaussians are re-born on alive
 * ones, and the set grows towards cap_max.  Every decision is made on the OLD set, in ONE pass (gsplat relocates, then samples again
 * for the growth; here both draw from the same old opacities).
 *   DEAD     o <= min_opacity, or NaN; alive otherwise.   n_grow = max(0, min(cap_max, (int64)floor(grow_factor N)) - N), in binary64.
 *   DRAWS    D = n_dead + n_grow, proportional to opacity, exactly: w_i = alive ? (uint32)(o_i 2^24) : 0; P_i the inclusive prefix of w
 *            in the caller's order (uint64); draw d takes the 64-bit u_d of the generator keyed by (seed, d), t = mulhi64(u_d, total),
 *            and selects the i with P_(i-1) <= t < P_i.  copies_i = the draws that selected i.
 *            (An opacity above 1 is outside the contract; it weighs as 1.)
 *   SOURCES  copies_i > 0 (gsplat's compute_relocation): n = min(copies_i + 1, 51), o' = 1 - (1 - o)^(1/n),
 *            denom = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1), both in binary64 in that order; o' and o / denom
 *            rounded once to float32; o' <- min(max(o', min_opacity), 1 - FLT_EPSILON); scale' = (o / denom) scale per axis in float32.
 *   NEW SCENE, in the new caller's order: the alive Gaussians in their old order (a source carries o' and scale', everything else bit
 *            for bit), then D children in draw order, each a bit-identical copy of its modified source, mean included (the noise
 *            separates them afterwards).  Group ids are inherited.
 *   OPTIMISER STATE  an alive Gaussian that is no source keeps moments and raw values bit for bit; sources and children get zero moments
 *            in every group (gsplat leaves a relocated Gaussian's moments in place) and fresh raw values from their new resident values.
 *   parents_out_or_null  int32 DEVICE with room for max(N, min(cap_max, floor(grow_factor N))) entries; [0, N_new) <- each new Gaussian's
 *            old index.   counts_out  HOST: (N_new, relocated = n_dead, added = n_grow).
 * D == 0 leaves the scene untouched: parents = 0 .. N-1, counts (N, 0, 0).  Otherwise storage order, feature store, last frame, group
 * poses, link constants, meshes and sh_degree are treated as sas_scene_densify treats them.  Blocking; completes the frames in flight.
 * SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID -- the scene stays as it was -- for cfg / counts_out NULL, min_opacity outside
 * [0, 1) (NaN included), cap_max < 1 or > 2^31 - 256, grow_factor < 1 or not finite, a cov6 scene (it has no scales to relocate), an
 * empty scene, and no alive Gaussian.
 */
typedef struct sas_mcmc_config {
    int64_t cap_max;       /* the budget, >= 1 */
    double grow_factor;    /* 1.05 */
    float min_opacity;     /* 0.005 */
    unsigned seed;
} sas_mcmc_config;
/* (sas_scene_densify_times then reports this call's laps: the weights and their totals' read-back; the draws' and the rows' enqueue; the
 * storage order's enqueue; allocation, relayout, state and commit -- see there, also for SAS_ORDER=0.) */
int sas_scene_mcmc_refine(sas_ctx *ctx, const sas_mcmc_config *cfg, int32_t *parents_out_or_null, int64_t counts_out[3], void *stream);

/*
 * Photometric loss of 3DGS training and its gradient ("Photometric loss"): for a delivered frame x = rgb [H,W,3] and a
 * target y [H,W,3] (float32 DEVICE, 0..1) and an optional mask w [H,W] (uint8 DEVICE, non-zero counts; NULL: every pixel counts),
 *   loss = (1 - lambda) l1 + lambda (1 - ssim),   l1 = sum w |x - y| / D,   ssim = sum w ssim_p / D,   mse = sum w (x - y)^2 / D,
 *   D = max(3 sum w, 1),
 * where ssim_p is the per pixel and channel SSIM map under the 11x11 Gaussian window (sigma 1.5, normalised, ZERO padding) with
 * C1 = 0.01^2, C2 = 0.03^2.  The mask weights the map; the window statistics see the whole image.
 *   terms          float32[4] DEVICE: (loss, l1, ssim, mse).  lambda == 0 does no SSIM work: ssim is then NaN, loss == l1.
 *   g_rgb_or_null  [H,W,3] DEVICE: the exact derivative of loss with respect to x (sign(0) = 0; none with respect to y).
 *   alpha_or_null  non-NULL selects the PRECHAINED form (its values are not read: with no depth gradient the prechain needs none): g_rgb is the gradient of the raw accumulator sas_render_backward takes -- 0 where x >= 1, where
 *                  the frame's clamp binds -- and g_alpha_or_null [H,W] = -sum_c g_rgb[c] background[c].  g_alpha requires alpha.
 * Both gradient pointers NULL: only the terms are computed (the metrics path: no second stencil).
 * Nothing is summed with atomics: the same inputs give the same bits in every output.  A non-finite value in x or y propagates: the
 * terms become NaN, and so do the gradients within 10 pixels of it (only the pixel's own when lambda == 0); nothing else changes.
 * The call only enqueues on `stream` and never waits for the host; its scratch belongs to the context (calls of one context are
 * ordered by one stream).  It needs no uploaded scene.  SAS_ERR_INVALID for a non-positive size, NULL rgb / target / terms, lambda
 * outside [0, 1] (NaN included), g_alpha without alpha, alpha without a background.
 */
int sas_photometric_loss(sas_ctx *ctx, int width, int height, const float *rgb, const float *target, const uint8_t *mask_or_null,
                         const float *alpha_or_null, const float *background, float lambda_dssim, float *terms,
                         float *g_rgb_or_null, float *g_alpha_or_null, void *stream);

/*
 * The resident scene, in the CALLER's order and the upload's shapes: means [N,3], quats [N,4] and scales [N,3] or cov6 [N,6], opacities
 * [N], colors [N,(L+1)^2,3] ([N,3] plain colours), float32, HOST or DEVICE, each may be NULL.  Straight after an upload these are the
 * uploaded bits; after optimiser steps, the fitted scene (how it is saved, or uploaded again to renew the storage order).  The form the
 * scene was not uploaded in is SAS_ERR_INVALID; SAS_ERR_NO_SCENE before an upload.  Blocking; frames in flight are completed.
 */
int sas_scene_read(sas_ctx *ctx, float *means, float *quats, float *scales, float *cov6, float *opacities, float *colors);

/*
 * The storage order ("Storage order"): the permutation slot -> caller's index in which a scene's Gaussians are stored,
 * ordered by (group id, Hilbert index of the mean at 10 bits per axis over the finite coordinates' box, caller's index).  Computed on the
 * device; the same bits as the host function the library keeps as its reference (SAS_ORDER=0 selects that one for uploads, densify and
 * refine calls of a context).
 *
 * sas_storage_order needs no scene: means [n,3] float32, group_id [n] uint8 or NULL, perm_out [n] int32, all DEVICE.  Non-finite
 * coordinates quantise to 0.  It only ENQUEUES, on `stream`: perm_out is complete when the stream reaches it.  n == 0 does nothing.  The
 * scratch is the context's: a call on another stream runs behind the one before, and a call with a larger n than any before it grows
 * the scratch first -- hipFree and hipMalloc, which wait for the device (so no earlier call loses its buffers) and are not allowed
 * inside a stream capture: call once at the largest n before capturing.  SAS_ERR_INVALID for n < 0 or > 2^31 - 1, means or perm_out NULL.
 *
 * sas_scene_order copies the resident scene's permutation to perm_out [N] int32, HOST or DEVICE.  Blocking; frames in flight are
 * completed.  SAS_ERR_NO_SCENE before an upload; an empty scene writes nothing.
 */
int sas_storage_order(sas_ctx *ctx, int64_t n, const float *means, const uint8_t *group_id_or_null, int32_t *perm_out, void *stream);
int sas_scene_order(sas_ctx *ctx, int32_t *perm_out);

/*
 * Nearest neighbours within one cloud ("Scene from points"): for every point of points [n,3] its k nearest OTHER points of the
 * same cloud, exactly.  d2 = (dx dx + dy dy) + dz dz in IEEE binary32, nothing fused, d = candidate - point; candidates are compared by the
 * key bits(d2) << 32 | index: the k smallest keys win, in ascending order, so equal distances go to the lower index.  The point itself is
 * left out by INDEX: a duplicate is a neighbour at d2 = 0.  A candidate whose d2 is NaN or +inf never counts, so a point with a non-finite
 * coordinate neither is a neighbour nor has one.  Missing neighbours read dist2 = +inf, index = -1.  No result depends on the grid the
 * library searches with, on the launch shape or on the order in which its workgroups run.
 *
 * points, dist2_out [n,k] float32 and index_out_or_null [n,k] int32 are DEVICE arrays.  Needs no scene.  It only ENQUEUES, on `stream`, and
 * shares sas_storage_order's rules for the context's scratch (a larger n grows it first, which waits for the device).  n == 0 does nothing.
 * SAS_ERR_INVALID for k outside 1..8, n < 0 or > 2^31 - 1, points or dist2_out NULL with n > 0.
 * The environment variable SAS_KNN_GRID=g (read when the context is created) forces g cells per axis in the place of the library's choice;
 * g = 1 is pure brute force.
 *
 * sas_knn_last_counts (blocking) reports what the last call decided on the device, up to n of: [0] points the grid search handed to the
 * brute-force kernel, [1..3] the grid's cells per axis, [4] 1 when there was no grid (the whole cloud went through the brute-force kernel),
 * [5], [6] the occupied cells of the 32^3 and 16^3 occupancy grids the choice was made from.  Zeros before the first call.
 */
int sas_knn_points(sas_ctx *ctx, int64_t n, const float *points, int k, float *dist2_out, int32_t *index_out_or_null, void *stream);
int sas_knn_last_counts(sas_ctx *ctx, int64_t *out, int n);

/*
 * Deformable splats ("Deformation"): an embedded deformation graph over the resident scene.  Every Gaussian is bound to up
 * to 8 of M control nodes with weights; the nodes move rigidly, the means follow by linear blend skinning and the orientations by a
 * blended quaternion.  Node transforms are expected to be RIGID: stretch and shear are not represented.
 *
 * sas_knn_cross -- for every point of points [n,3] its k (1..8) nearest NODES of nodes [m,3], 1 <= m <= 65536, exactly: sas_knn_points'
 * contract (d2 = (dx dx + dy dy) + dz dz in binary32 with d = node - point, keys bits(d2) << 32 | node index, the k smallest ascending, a
 * NaN or +inf d2 never counts, missing neighbours read +inf / -1) with two differences: nothing is left out by index, and a node with
 * d2 > max_distance^2 (binary32, the square formed once on the host; INFINITY: no cut) never counts.  m < k is allowed.  points, nodes,
 * dist2_out [n,k] float32 and index_out_or_null [n,k] int32 are DEVICE arrays.  Needs no scene and no scratch; it only ENQUEUES, on `stream`.
 * SAS_ERR_INVALID for k outside 1..8, n < 0 or > 2^31 - 1, m outside 1..65536, a negative or NaN max_distance, a missing array with n > 0.
 *
 * sas_scene_skin -- bind a skin to the resident scene: indices [N,k] int32 and weights [N,k] float32, 1 <= k <= 8, DEVICE arrays in the
 * caller's order.  The first bind snapshots the means, orientations and scales (or covariances) as the REST pose; a bind over a skin
 * replaces the entries and keeps the rest pose.  k == 0 (indices and weights ignored) clears the skin: the rest pose returns bit for
 * bit (as sas_scene_adam_step_rest has stepped it, if it has).  While a skin is bound sas_scene_adam_step, sas_scene_densify, sas_scene_mcmc_refine, sas_scene_mcmc_noise and
 * sas_scene_reset_opacity are SAS_ERR_INVALID ("scene is skinned") and change nothing; everything that reads the scene sees the deformed
 * Gaussians; sas_scene_upload drops the skin.  Enqueued on `stream`; frames in flight are completed first.
 * sas_scene_skin_read -- the entries back in the caller's order, [N,k] each with the k of the bind, HOST or DEVICE.  Blocking.
 * SAS_ERR_INVALID without a skin.
 *
 * sas_scene_deform -- node_Rt [m,3,4] float32 DEVICE, rows [R | t] that map REST to CURRENT in the frame the scene was uploaded in (in
 * front of the group poses), 1 <= m <= 65536.  An entry is LIVE when 0 <= index < m and weight > 0; every other entry is ignored.  Per
 * Gaussian with live entries j, in entry order and binary32, nothing fused:
 *   mean'  = mean + (sum_j w_j ((R_j mean + t_j) - mean)) / sum_j w_j
 *   q_b    = normalize(sum_j s_j w_j q_j), q_j the unit quaternion of R_j, s_j = -1 where dot(q_j, q_first) < 0
 *   quat'  = q_b (x) quat (scales untouched), or Sigma' = R(q_b) Sigma R(q_b)^T for a scene uploaded as covariances
 * A Gaussian without a live entry keeps the rest pose's bits.  Opacities, colours, groups, the storage order and N are never written.
 * The state is always rest -> current, never accumulated.  Two launches on `stream`, nothing is waited for but frames in flight; the last
 * frame is invalidated as sas_scene_adam_step does.  SAS_ERR_INVALID without a skin, for m out of range or node_Rt NULL.
 * The environment variable SAS_SKIN_LDS=bytes (read when the context is created; 0..16384, the default) is the size up to which the node
 * records (64 B each) are staged in LDS; no result depends on it.
 *
 * sas_scene_deform_backward -- the adjoint of the LAST sas_scene_deform on the bound skin: from the gradients of the deformed arrays, as
 * sas_render_backward writes them on a skinned scene (d_means [N,3], and d_quats [N,4] for a quaternion scene or d_cov6 [N,6] for a
 * covariance scene; float32 DEVICE, the caller's order), to d_node_Rt [m,3,4] float32 DEVICE, WRITTEN: the gradient with respect to the
 * twelve entries of every node's [R | t], each an independent variable, exactly as d_viewmat and d_group_poses treat theirs.  m is the
 * last deform's.  The orientation gradient that does not match the scene's form must be NULL; d_means or the orientation gradient may be
 * NULL, not both; with the orientation gradient NULL the rotation path is skipped entirely.  The function differentiated is the one
 * sas_scene_deform evaluates with every decision a constant: which entries are live, the branch of the matrix-to-quaternion conversion,
 * the signs s_j, and the fallback to q_first.  The node records the deform left on the device are the saved state: node_Rt may have
 * changed since.  A node no live entry names gets an exact zero row; zero upstream gives exact zeros.  Otherwise the sums are float
 * atomics and vary in their last bits from run to run.  The adjoint is linear in its inputs: sum the views' gradients, call once.
 * It only ENQUEUES on `stream` (behind the deform, and behind its own previous call, whose accumulator it shares); no host
 * synchronisation.  SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID without a skin, without a sas_scene_deform since the skin was
 * bound (a rebind or a clear resets that), for all three gradients NULL, an orientation gradient of the wrong form, d_node_Rt NULL.
 * SAS_SKIN_GRAD_LDS=bytes (0..131072, the default) is the size up to which the per-node sums (64 B each) are kept in LDS by every
 * workgroup; SAS_SKIN_GRAD_STAGED=0/1 forces the form of the adds.  Both change the order of the sums only.
 *
 * sas_scene_deform_backward_rest -- the adjoint of the LAST sas_scene_deform to the REST arrays, the Gaussians that are stored: the same
 * inputs as sas_scene_deform_backward, under the same form rule, to d_rest_means [N,3] and d_rest_quats [N,4] or d_rest_cov6 [N,6], float32
 * DEVICE arrays in the caller's order.  The call ACCUMULATES: out[i] += the gradient, so that the sum over time steps, each with its own
 * deformation, is taken here; zero the arrays before the first.  An output is given exactly where its input is (d_rest_means with
 * d_means, and so on); no output may overlap an input or another output.  With the forward's decisions as constants:
 *   d_mean   = g + (sum_j w_j ((R_j^T g) - g)) / sum_j w_j, over the live entries in entry order
 *   d_quat   = conj(q_b) (x) h (the transpose of the left product by q_b), or dSigma = R(q_b)^T G R(q_b) for a covariance scene, G the
 *              symmetric matrix of d_cov6 in sas_render_backward's convention, written back in that convention
 * A Gaussian without a live entry has its gradient passed through bit for bit; with flags & SAS_DEFORM_REST_BOUND_ONLY it adds nothing
 * (for skins bound to one group: the static rest of the scene then gets no step from a fit of the deformable group).  Every output depends
 * on its own input alone, and an all-zero gradient adds exact zeros: SAS_ADAM_VISIBLE_ONLY keeps its meaning.  No atomics: the same inputs
 * give the same bits on every run and under every SAS_SKIN_LDS.  Opacity, colour and scale gradients are untouched by a deformation: they
 * are the rest scene's as sas_render_backward wrote them.  It only ENQUEUES on `stream`, behind the deform; no host synchronisation.
 * SAS_ERR_NO_SCENE before an upload; SAS_ERR_INVALID without a skin, without a sas_scene_deform since the skin was bound, for unknown
 * flags, all three gradients NULL, an orientation gradient of the wrong form, an output without its input or an input without its
 * output, or overlapping arrays.
 *
 * sas_scene_adam_step_rest -- sas_scene_adam_step on the REST scene of a bound skin: the same arguments, kernel, variables and optimiser
 * state (a group stepped here for the first time starts as it would there; the moments survive clearing the skin), with gradients with
 * respect to the rest arrays (sas_scene_deform_backward_rest's sums, and sas_render_backward's opacity, colour and scale gradients as
 * they are).  The rest planes are stepped; colours are no part of the rest snapshot and step where they live.  Then the last deformation is
 * applied again from the node records on the device -- without a sas_scene_deform since the bind the rest planes are copied -- so every
 * reader sees the stepped scene in its current bend, and clearing the skin returns the STEPPED rest scene.  The last frame is invalidated
 * as sas_scene_deform does.  SAS_ERR_INVALID without a skin; sas_scene_adam_step itself stays refused under one.
 */
#define SAS_DEFORM_REST_BOUND_ONLY 1u
int sas_knn_cross(sas_ctx *ctx, int64_t n, const float *points, int64_t m, const float *nodes, int k, float max_distance,
                  float *dist2_out, int32_t *index_out_or_null, void *stream);
int sas_scene_skin(sas_ctx *ctx, int k, const int32_t *indices, const float *weights, void *stream);
int sas_scene_skin_read(sas_ctx *ctx, int32_t *indices_out, float *weights_out);
int sas_scene_deform(sas_ctx *ctx, int m, const float *node_Rt, void *stream);
int sas_scene_deform_backward(sas_ctx *ctx, const float *d_means, const float *d_quats, const float *d_cov6, float *d_node_Rt, void *stream);
int sas_scene_deform_backward_rest(sas_ctx *ctx, const float *d_means, const float *d_quats, const float *d_cov6, float *d_rest_means,
                                   float *d_rest_quats, float *d_rest_cov6, unsigned flags, void *stream);
int sas_scene_adam_step_rest(sas_ctx *ctx, const sas_adam_config *cfg, const float *d_means, const float *d_opacities, const float *d_sh,
                             const float *d_quats, const float *d_scales, void *stream);

/*
 * The node optimiser on the device ("Deformation": the node optimiser): what fits the node transforms of a skin from the
 * gradients sas_scene_deform_backward writes, without the host in the loop.  Both calls are scene-free, take DEVICE arrays, only ENQUEUE on
 * `stream`, require 1 <= m <= 65536 and use no atomics: the same inputs give the same bits on every run.  The STATE -- the rows [R | t], the
 * Adam moments, the rigidity gradient -- is BINARY64 (double): a rotation left-multiplied hundreds of times in binary32 drifts away from
 * R^T R = I, and sas_scene_deform does not check device arrays.  The float32 rows sas_scene_deform takes are the state rounded once.
 *
 * sas_nodes_rigidity -- the embedded-deformation consistency term and its gradient:
 *   value = sum_i sum_{j in N(i)} |T_i(g_j) - T_j(g_j)|^2 / (m kn),   T(x) = R x + t the rows Rt64 [m,3,4], g = nodes [m,3] float32,
 * N(i) the kn (0..8) entries nb [m,kn] int32 of node i; an entry outside [0, m) is ignored.  d_Rt64_out [m,3,4] double, WRITTEN: the
 * gradient with respect to the twelve entries of every node, each an independent variable.  value_out [1] double, written.
 * rev_start [m + 1] / rev_edge is the REVERSE table: rev_edge[rev_start[j] .. rev_start[j + 1]) lists the edge numbers i kn + slot with
 * nb[i][slot] == j in ascending order; rev_start[m] <= m kn entries are read (ranges are clipped to that, edge numbers out of range are
 * ignored).  One lane per node: lane i sums its own kn edges in slot order, then its incoming edges in table order, every residual
 * recomputed from the two transforms -- the order of every sum is fixed, and a node with in-degree m - 1 is correct (and slow).  The value
 * is one partial sum per workgroup, then one fixed-order reduction; the partials (2 KiB) belong to the context and are allocated by its
 * first call: no later call allocates.  kn == 0 writes exact zeros and a value of 0 (nb and the reverse table may then be NULL).
 * SAS_ERR_INVALID for m or kn out of range, or a missing array.
 *
 * sas_nodes_twist_step -- one Adam step of every node's se(3) twist, left-multiplied about the node's CURRENT position p = R g + t.  The
 * gradient is G = double(d_Rt32) + weight64 * d_Rt64 ([m,3,4] each; either may be NULL, not both).  Per node, in binary64:
 *   tw   = (sum_c A[:,c] x G[:,c] over the four columns of A = [R | t], + G[:,3] x p;  G[:,3])          (the twist gradient about p)
 *   m1   = beta1 m1 + gain1 tw,   m2 = beta2 m2 + gain2 tw tw                                            ([m,6] each, in place)
 *   hat  = (m1 / c1) / (sqrt(m2 / c2) + eps)
 *   E    = exp(-(lr_rot hat[0:3], lr_trans hat[3:6]))      (Rodrigues; below |omega| = 1e-8 the series 1 - th^2/6, 1/2 - th^2/24, 1/6 - th^2/120)
 *   R   <- E_R R,   t <- (E_R (t - p) + E_t) + p                                                         (Rt64, in place)
 * and Rt32_out [m,3,4] float32 = Rt64 rounded once (its bits are float(Rt64)).  gain1 / gain2 are the weights of the new gradient in the
 * moments, 1 - beta in exact arithmetic; they are given beside the betas because 1 - 0.999 in binary64 is not the binary64 0.001 a host
 * optimiser writes (they are 4 units in the last place apart).  The bias corrections c1 = 1 - beta1^step, c2 = 1 - beta2^step and the
 * decayed rates are formed on the host.  One launch, no scratch.
 * SAS_ERR_INVALID for m out of range, non-finite or negative rates, eps or weight64, betas outside [0,1), gains outside (0,1], c1 or
 * c2 <= 0, both gradients NULL, or a missing array.
 */
typedef struct sas_node_step_config {
    double lr_rot, lr_trans;   /* radians, scene units */
    double beta1, beta2;       /* 0.9, 0.999 */
    double c1, c2;             /* 1 - beta1^(it + 1), 1 - beta2^(it + 1) */
    double eps;                /* 1e-12 */
    double gain1, gain2;       /* 0.1, 0.001 */
} sas_node_step_config;
int sas_nodes_rigidity(sas_ctx *ctx, int64_t m, const float *nodes, const double *Rt64, int kn, const int32_t *nb, const int32_t *rev_start,
                       const int32_t *rev_edge, double *d_Rt64_out, double *value_out, void *stream);
int sas_nodes_twist_step(sas_ctx *ctx, int64_t m, const float *nodes, const float *d_Rt32_or_null, const double *d_Rt64_or_null,
                         double weight64, double *Rt64, double *m1, double *m2, float *Rt32_out, const sas_node_step_config *cfg,
                         void *stream);

/*
 * The node driver on the device ("Deformation": the node driver): the rigid rows [R | t] of every node from the node POSITIONS a
 * physics engine publishes -- what deform.transforms_from_positions computes on the host -- so that positions -> transforms -> sas_scene_deform
 * -> frame stays on the device.  Scene-free, DEVICE arrays, only ENQUEUES on `stream`, no atomics, no scratch: the same inputs give the same bits.
 *
 * sas_nodes_fit_rigid -- nodes [m,3] float32 the rest positions, moved [steps,m,3] float32 their positions in `steps` >= 1 time steps (a
 * recorded trajectory is one launch), nb [m,kn] int32 (kn 0..8) sas_knn_points' table of the rest nodes.  One lane per (step, node), binary64,
 * only + - * / and sqrt, every loop of a fixed length (a poisoned input costs what a clean one costs):
 *   members  node i itself, then nb[i] in slot order; an entry outside [0, m) is ignored, and so is a member whose moved position has a
 *            non-finite coordinate.  If node i's OWN moved position is not finite the lane writes [I | 0].
 *   S        = sum (a - ca)(b - cb)^T over the members in that order, ca / cb the centroids of their rest / moved positions
 *   N        Horn's symmetric 4x4 matrix of S; all four eigenpairs by 14 cyclic Jacobi sweeps (a fixed count: csrc/sas_internal.h)
 *   q        (1,0,0,0) projected onto the span of the eigenvectors whose eigenvalue is within 1e-9 (times the largest |eigenvalue|) of the
 *            top one, normalised.  One rule for every case: the top eigenvector with q_w >= 0 for a neighbourhood of full rank; of all
 *            optimal rotations the one of LEAST angle for a collinear one (two nodes, a rope); the identity for S = 0 (kn = 0, one node, all
 *            members coincident).  A projection with a squared norm below 1e-12 is an exact half turn: the top eigenvector as it is.
 *   R, t     R of the unit quaternion -- always a proper rotation, there is no determinant to correct -- and t = moved_i - R rest_i: the
 *            node lands on its moved position.
 * Rt64_out_or_null [steps,m,3,4] double and Rt32_out [steps,m,3,4] float32 = the double rounded once, both WRITTEN.  Not represented: member
 * weights, pinned nodes, stretch and shear.
 * SAS_ERR_INVALID for m outside 1..65536, steps < 1 or steps * m > 2^30, kn out of range, or a missing array (nb may be NULL with kn == 0).
 */
int sas_nodes_fit_rigid(sas_ctx *ctx, int steps, int64_t m, const float *nodes, const float *moved, int kn, const int32_t *nb,
                        double *Rt64_out_or_null, float *Rt32_out, void *stream);

/* sas_render_batch_host from camera POSES: n_views camera-to-world poses (wxyz [n,4], position [n,3], float64, OpenCV
 * axes: what client.get_render(height, width, wxyz, position) takes, splat_env_wrapper.py:148-157) and one vertical
 * field of view; the view matrices and intrinsics are those of sas_camera_matrices. */
int sas_render_cameras_host(sas_ctx *ctx, int n_views, const double *wxyz, const double *position, double fov, int width,
                            int height, const float *background, unsigned flags, uint8_t *rgb8_host, void *stream);

/* Complete every SAS_ASYNC frame in flight: synchronise with each, and where its intersection buffer
 * overflowed grow it and render the frame again. */
int sas_wait(sas_ctx *ctx);

/* Frames submitted / completed (see SAS_ASYNC) since sas_create; either pointer may be NULL.  Frames
 * 0 .. *completed-1 (in submission order) are final and `stream` is ordered behind them. */
int sas_frames_completed(sas_ctx *ctx, int64_t *submitted, int64_t *completed);

const char *sas_last_error(sas_ctx *ctx);
int sas_stage_times(sas_ctx *ctx, float *ms, int n);
/* Mean stage times over the frames completed with SAS_TIMING / SAS_TIME_TILES since the last reset
 * (slots without events read 0); *frames receives the number of frames averaged. */
int sas_stage_time_means(sas_ctx *ctx, float *ms, int n, int64_t *frames, int reset);
int sas_frame_stats(sas_ctx *ctx, int64_t *stats, int n);

/* Parity hooks (HOST output pointers, any may be NULL): per-Gaussian projection results and the
 * per-tile sorted lists of the last completed frame, in the layout of gsplat's intermediate
 * tensors (radii [n,2] i32, means2d [n,2], depths [n], conics [n,3], colors [n,3];
 * tile_offsets [tiles+1] i32, sorted_ids [<=cap] i32).  sorted_ids is complete only for a frame
 * rendered with SAS_FULL_SORT (the default path orders lists lazily, front chunk by front chunk).
 * sas_read_projection: the product path does not keep the rectangles and radii of a frame (nothing on the device reads
 * them); the hook projects the last frame once more to obtain them -- same camera, same pose snapshot -- before it
 * reads back: a test facility, not a per-frame call. */
int sas_read_projection(sas_ctx *ctx, int32_t *radii, float *means2d, float *depths, float *conics,
                        float *colors);
int sas_read_tile_lists(sas_ctx *ctx, int32_t *tile_offsets, int32_t *sorted_ids, int64_t cap);

const char *sas_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SIM_A_SPLAT_AMD_H */
