// sas_api.cpp -- context management and the C ABI declared in include/sim_a_splat_amd.h.
// Compiled by hipcc together with sas_kernels.hip into libsas_hip.so.  Host float arithmetic
// that feeds the kernels (camera constants) follows the arithmetic contract: built with
// -ffp-contract=off, fused only where fmaf() is written.
#include "../../include/sim_a_splat_amd.h"
#include "sas_internal.h"

#include <cmath>
#include <functional>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace {

// OWNERS.  What the context holds of the runtime (device memory, pinned blocks, streams, events) belongs to a move-only member that
// gives it back in its destructor; a staging buffer is a local.  The four calls that give something back are written once, in these.
template <class T, auto Free>
struct Owned {
    T h{};
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = T{}; }
    Owned &operator=(Owned &&o) noexcept { std::swap(h, o.h); return *this; }
    ~Owned() { if (h) (void)Free(h); }
    T *put() { return &h; }   // (of an empty owner: for the runtime's create calls)
    operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
template <class T> using Pinned = Owned<T *, hipHostFree>;

// Device memory that only ever grows (ensure) unless it is given back on purpose (release).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { (void)release(); }
    int release(sas_ctx *c = nullptr);   // (behind HIP_TRY; c: where a failure is reported)
};

// Where one view's images go: device buffers of the caller, except rgb8_host.  A view carries them from the C ABI to
// its slot as a whole (ViewCall -> RenderArgs); only the kernels' argument segment has a layout of its own (SasOutputs).
struct ViewOut {
    float *rgb = nullptr, *alpha = nullptr, *depth = nullptr;
    uint8_t *rgb8 = nullptr;
    float *points = nullptr;   // RGB-D tail (sas_render_rgbd)
    uint8_t *mask = nullptr;
    uint8_t *rgb8_host = nullptr;   // sas_render_batch_host: host copy of rgb8, made on the frame's stream
    float *features = nullptr;      // sas_render_features: [H,W,feat_c] (device), composited behind the frame's k_blend
    uint8_t *labels = nullptr;      // sas_render_batch_labels: [H,W] (device), the argmax of the one-hot stores' channels
    // The frame's list reader: what walks its complete lists once more behind k_blend and ADDS to buffers of the caller's, with its
    // arguments as the record its kernel takes.  At most one per frame, so the records share their bytes.
    enum Reader : uint8_t { NO_READER, LIFT_LABELS, LIFT_FEATURES, BACKWARD } reader = NO_READER;
    // sas_render_backward_screen: k_grad_tiles' record; sas_render_backward: k_grad_project's behind it (proj.s_means2d nullptr: no
    // chain), whose s_* are tiles' d_*; sas_render_backward_poses: the selected groups as well (poses.n_sel 0: none)
    struct Backward { SasGrad tiles; SasGradProj proj; SasPoseSel poses; };
    union {
        SasLift lift;                    // sas_lift_labels
        SasLiftFeatures lift_features;   // sas_lift_features
        Backward back{};
    };
    bool chained() const { return reader == BACKWARD && back.proj.s_means2d; }   // (k_grad_project reads the group poses on the device)
};
static_assert(sizeof(ViewOut) <= 344, "ViewOut is copied per view into RenderArgs on the render path: it was 344 bytes with the readers' arguments field by field");

struct RenderArgs {
    float viewmat[16], K[9], bg[3];
    int W = 0, H = 0;
    unsigned flags = 0;
    ViewOut out;
    float max_depth = 0.0f;
    bool use_max_depth = false;
    hipStream_t stream = nullptr;
    bool order_caller = true;  // the frame writes device buffers of the caller: it runs behind what the caller's stream holds, and the
                               // caller's stream is ordered behind it (false: frames delivered to host memory, sas_render_batch_host)
    bool solo = false;         // a blocking call for this one view with nothing else in flight: the caller waits for the frame's chain
    int feat_c = 0;            // channels of out.features
    float fbg[SAS_MAX_FEATURES];   // feature background, [feat_c]
    float min_alpha = 0.0f;        // of out.labels
};

// The resident scene's planes (k_relayout's layout) and its storage order; sas_scene_densify builds a second record and swaps it in.
struct Planes {
    DevBuf g0, g1, g2, col, gid8, perm;
    std::vector<int> perm_host;   // perm's host copy (slot -> caller's index), made on demand: host_perm() fills it, forget_host_perm() drops it
    bool perm_host_valid = false;
    int64_t n = 0, n_pad = 0;
    int alloc(sas_ctx *c, int64_t count, int colour_planes);   // (the device buffers alone)
    int host_perm(sas_ctx *c, const int **out);   // the host copy, read back from `perm` when it is not there (blocking)
    void forget_host_perm() { perm_host.clear(); perm_host_valid = false; }   // wherever the device `perm` changes
    void bind(SasScene &s) const
    {
        s.g0 = (const float4 *)g0.p; s.g1 = (const float4 *)g1.p; s.g2 = (const float4 *)g2.p; s.col = (const float4 *)col.p;
        s.gid8 = (const uint8_t *)gid8.p; s.perm = (const int *)perm.p;
        s.n = n; s.n_pad = n_pad;
    }
};

// Optimiser state (sas_scene_adam_step), slot order; a group's buffers exist from its first step to the next upload or reset.  `rows` is
// THE description of the state: which group a buffer belongs to (its flag in `on` guards it), whether it spans the colour planes, and
// whether a first step finds it zeroed or filled by k_adam_init.  Everything else here is derived from it.
struct Adam {
    enum Group { MEANS, QUATS, SH, OPACITIES, SCALES, GROUPS };   // (in the order a first step allocates them)
    struct Row { float4 *SasAdamState::*field; Group group; bool colour, zeroed; };
    static constexpr int kRows = 10;
    static constexpr Row rows[kRows] = {
        {&SasAdamState::means_m, MEANS, false, true},   {&SasAdamState::means_v, MEANS, false, true},
        {&SasAdamState::opac, OPACITIES, false, false},
        {&SasAdamState::quats_m, QUATS, false, true},   {&SasAdamState::quats_v, QUATS, false, true},
        {&SasAdamState::scales_m, SCALES, false, true}, {&SasAdamState::scales_v, SCALES, false, true}, {&SasAdamState::scales_raw, SCALES, false, false},
        {&SasAdamState::sh_m, SH, true, true},          {&SasAdamState::sh_v, SH, true, true}};
    DevBuf buf[kRows];
    bool on[GROUPS] = {false, false, false, false, false};
    int drop(sas_ctx *c);
    int alloc(sas_ctx *c, int row, int64_t n_pad, int colour_planes, hipStream_t st, bool zero);   // buf[row] for n_pad slots, zeroed on st
    SasAdamState view(const bool *which = nullptr) const   // (which: the buffers of those groups alone, nullptr for the others)
    {
        SasAdamState s{};
        for (int k = 0; k < kRows; ++k)
            if (!which || which[rows[k].group]) s.*rows[k].field = (float4 *)buf[k].p;
        return s;
    }
};

// The skin of the resident scene (sas_scene_skin; DESIGN.md 3, "Deformation"), slot order: the rest snapshot of g0 / g1 / g2 taken at the
// first bind, the entries' planes, and the node records of the last sas_scene_deform.  k == 0: no skin is bound.  Clearing a skin gives no
// memory back (hipFree would wait for the whole device in front of frames in flight): the buffers serve the next bind, and go where the
// optimiser state goes, at the next upload or with the context.  m: the node count of the last sas_scene_deform since the bind, whose records
// `nodes` holds (0: none -- sas_scene_deform_backward has nothing to differentiate); grad_acc: that call's accumulator [m,16].
struct Skin {
    DevBuf rest0, rest1, rest2, idx, w, nodes, grad_acc;
    int k = 0;
    int m = 0;
    bool bound() const { return k > 0; }
    int kp() const { return k <= 4 ? 4 : SAS_SKIN_MAX_K; }
    int drop(sas_ctx *c);
};

}  // namespace

// Per-frame scratch.  Every slot owns one, so several frames can be on the GPU at the same time.
struct Scratch {
    DevBuf rec, col, info, tilebuf, keys, ids, counters, wgvis, wgbase, tilemax;
    long long cap = 0;
    long long seg = 0;            // single-pass binning: keys per tile segment (grown when a tile outgrows it)
    bool seg_too_big = false;     // ... segments for this slot's frames would exceed the memory budget: two-pass binning instead
    int seg_tiles = -1;           // the tile count and scene size `seg` / `seg_too_big` were established for: another frame size or scene
    int64_t seg_n = -1;           // sizes the segments afresh (a slot that once met a pathological frame does not stay two-pass for good)
    // what the slot has learned about other (tile count, scene size) pairs it has rendered: a slot that alternates between two
    // camera sizes neither carries one size's segment length over to the other nor guesses (and overflows) anew at every change
    struct SegMemo { int tiles; int64_t n; long long seg; };
    SegMemo seg_memo[4] = {{-1, -1, 0}, {-1, -1, 0}, {-1, -1, 0}, {-1, -1, 0}};
    int seg_memo_next = 0;
    bool counters_zero = false;   // the counter block is known to be all zero (SasFrame invariant)
};

// Mesh scratch of a slot's frame (SasMeshFrame), when the context holds meshes.
struct MeshScratch {
    DevBuf rec, rect, tiles, list;   // records, rectangles, [count | offset | cursor], lists
    DevBuf planes;                   // frames of meshes with vertex attributes: the records' attribute planes (SAS_MESH_PLANE_STRIDE float4 each)
    DevBuf win;                      // feature frames: every pixel's triangle as k_blend_mesh_scene resolved it (SasMeshExtra::win)
    long long cap = 0;               // entries `list` holds (grown like the splat keys when a frame outgrows it)
    Pinned<unsigned> status_host;    // [2], written by k_mesh_scan
};

// One in-flight frame.  Each slot has its own internal stream (plus two side streams for the
// concurrent sort classes) and its own scratch: the stages of a frame are each too short on
// parallelism to fill 256 CUs (a few thousand tiles), so consecutive frames overlap on the chip.
// A frame writes its output buffers only after everything the caller had enqueued on `stream` at the
// time of sas_render (its projection and binning, which touch only the scene and the slot's scratch,
// do not wait for the caller); the caller's stream is made to wait for frame i when it is complete.
// Frames reach the GPU through enqueue_launch alone, as a single view, a view pair (two slots, two streams, one
// two-view projection) or a launch group (up to SAS_MAX_GROUP slots, every launch shared, the leader's stream).
// A frame is: [group poses: one small upload kernel] projection (+ key emit, scan and tile order in its tail) [-> scatter: two-pass binning only] -> tile kernel
// [-> depth tail] [-> host copy] (enqueue_chain).  Parameters travel in the kernels' argument segments, the counters are left
// zeroed by the tile kernel, the statistics reach the host through pinned words the projection's tail writes:
// no memset, no upload and no read-back copy around a frame.
struct Slot {
    RenderArgs args;
    Stream fs, side[2];              // the frame's stream; the side streams of the concurrent sort classes
    Event fork, join[2];             // ... and their events: sort_streams names all five for sas_launch_sort
    SasSortStreams sort_streams{};
    Event start, done, pair_ev;      // pair_ev: leader of a view pair: both projections are done
    Event ev[SAS_T_COUNT + 1];
    Pinned<unsigned> stats_host;     // 8 words, written by the projection's tail (SasFrame::stats_host)
    Pinned<float> poses_host;        // [256 * 12]: the group poses this slot's frame was submitted with
    DevBuf poses_dev;                // ... and their device copy, uploaded in front of the projection
    Scratch scr;
    MeshScratch msc;
    SasCam cam{};
    SasParams params{};
    bool busy = false, timed = false, timed_tiles = false;
    bool quad = false;   // the frame runs in the quad layout: projected, binned and composited in 8-pixel tiles (prepare_frame)
    bool mesh = false;   // the frame composites the context's meshes (enqueue_chain): msc.status_host tells whether its lists fit
    bool direct = false; // single-pass binning (SasFrame::seg > 0): the projection emits the keys, no scatter launch (choose_binning)
    bool host_direct = false;   // the tile kernel delivers the uint8 frame to pinned host memory itself (host_direct_ok)
    bool info_kept = false;     // the frame's projection wrote info[] (SasFrame::keep_info): sas_read_projection need not project again
    int group = 1;   // slots of the launch group this slot LEADS (enqueue_chain); 0: member of the group led by an earlier slot
    // The slot's streams, events and pinned words (zeroed).  On failure the slot keeps what it got: its destructor gives it back.
    // (The order of creation is the one this code always had; whether it matters is open: profiles/host_owners_ab.txt, call C.)
    hipError_t init()
    {
        hipError_t e = hipSuccess;
        auto pinned = [&](auto &b, size_t count) {
            if (e == hipSuccess) e = hipHostMalloc((void **)b.put(), count * sizeof(*b.h));
            if (e == hipSuccess) memset(b.h, 0, count * sizeof(*b.h));
        };
        auto stream = [&](Stream &s) { if (e == hipSuccess) e = hipStreamCreateWithFlags(s.put(), hipStreamNonBlocking); };
        auto event = [&](Event &v, bool timing) {
            if (e == hipSuccess) e = timing ? hipEventCreate(v.put()) : hipEventCreateWithFlags(v.put(), hipEventDisableTiming);
        };
        pinned(stats_host, 8);
        pinned(poses_host, 12 * 256);
        pinned(msc.status_host, 2);
        stream(fs);
        for (Event *v : {&start, &done, &pair_ev}) event(*v, false);
        for (Event &v : ev) event(v, true);
        for (Stream &s : side) stream(s);
        for (Event *v : {&fork, &join[0], &join[1]}) event(*v, false);
        sort_streams = SasSortStreams{{side[0], side[1]}, fork, {join[0], join[1]}};
        return e;
    }
};

constexpr int kMaxSlots = 8;

// Constants of the per-link pose algebra (sas_set_link_constants), float64.
struct LinkConsts {
    int n = 0;
    double scale = 1.0, Ri[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ti[3] = {0, 0, 0}, weld[3] = {0, 0, 0};
    std::vector<double> Rfk, tfk;   // [n,9], [n,3]
    std::vector<int> group;         // [n] splat group driven by link k
};

// What the environment settles for a context, read once when it is created (from_env: the only getenv calls of this file).
struct Settings {
    int n_slots = 4;     // frames that may be enqueued (SAS_SLOTS=1..8; 6 and 8 are slower)
    // sas_render_batch projects two views per pass over the scene when that pass is long enough to pay
    // (measured: +5 % frames/s at 1 M Gaussians, +16 % at 5 M, -5 % at 0.3 M).  SAS_PAIR=0/1 forces it.
    int pair_views = -1;            // -1: by scene size
    // single-pass binning (fixed-stride tile segments, the projection emits the keys): -1 = whenever the segments fit
    // direct_budget bytes per CONTEXT (all its frame slots together: a slot's keys + ids may take direct_budget / n_slots), 0 =
    // never (SAS_DIRECT=0: the two-pass path of rounds 1-3).  24 GB: config 5's 6.4 GB per slot; of 288 GB of HBM
    int direct_mode = -1;
    long long direct_budget = 24ll << 30;
    // exact tile culling on single-pass frames (sas_kernels.hip: tile_reached); SAS_CULL=0 bins whole rectangles as T3 does
    int cull_mode = 1;
    int seg_guess_factor = 16;    // first guess of a tile segment = this x the mean list of a frame with five intersections per Gaussian (SAS_SEG_FACTOR)
    // quad layout (the frame binned in 8-pixel tiles, one workgroup per 8x8 quadrant): -1 = for views of at most
    // quad_max_tiles 16-pixel tiles, 0 = never, 1 = always (SAS_QUAD, SAS_QUAD_TILES)
    int quad_mode = -1;
    int quad_max_tiles = 640;        // views of frames that share the chip (SAS_ASYNC, batches): beyond, the layout's 4 x workgroups lose
    int quad_max_tiles_solo = 960;   // one blocking view alone on the GPU: its heaviest tile's chain is the frame (tools/quad_threshold.py)
    // sas_render_batch renders the views of a SMALL scene (< kPairMinGaussians: launch-bound frames, the Gym
    // cameras) in groups that share one set of launches (grid.y = view).  SAS_GROUP=1 disables, 2..4 sets the size.
    int group_views = -1;           // -1: half of the slots (two groups can be in flight)
    // nothing in flight: the ring restarts at slot 0, so that a sequence of frames always meets the slots in the same order
    // (SAS_RING_RESTART=0: the ring goes on where it stood -- bench passes of 25 steps then start on alternating slot pairs)
    bool ring_restart = true;
    // the storage order of a scene (upload, densify, mcmc_refine) is computed on the device (sas_order.hip); SAS_ORDER=0: by storage_order()
    // on the host, from read-back means and group ids -- the reference the device path equals bit for bit, kept for A/B runs
    // (tools/order_probe.py, profiles/storage_order.txt)
    bool order_on_device = true;
    // sas_knn_points chooses its grid on the device (sas_knn.hip: the grid rule); SAS_KNN_GRID=g forces g cells per axis, 1: no grid, every
    // point through the brute-force kernel.  No result depends on it: the knob is there so that tests and tools/knn_probe.py compare the paths
    int knn_grid = 0;
    // sas_scene_deform stages the node records in LDS while m * 64 B fits this budget (SAS_SKIN_LDS=bytes, 0: never; SAS_SKIN_LDS_BYTES at
    // most, which is what the kernel reserves).  No result depends on it: the knob is there so that tests and tools/deform_probe.py compare the paths
    int skin_lds = SAS_SKIN_LDS_BYTES;
    // sas_scene_deform_backward sums its accumulator rows in LDS while m * 64 B fits this budget (SAS_SKIN_GRAD_LDS=bytes, 0: never;
    // SAS_SKIN_GRAD_LDS_MAX at most), and above it adds to global memory.  skin_grad_staged: rows pass through LDS and are added 16 lanes per row
    // (1) or every lane adds its own row (0); -1: the faster form (profiles/deform_grad.txt): staged on the global path, and on the LDS path while the
    // accumulator is within SAS_SKIN_GRAD_STAGED_LDS_BYTES (beyond it the stage costs workgroups per CU).  SAS_SKIN_GRAD_STAGED=0/1 forces one.
    // Results differ in their last bits only (the order of a float sum): the knobs are there so that tests and tools/deform_grad_probe.py compare
    int skin_grad_lds = SAS_SKIN_GRAD_LDS_BYTES;
    int skin_grad_staged = -1;
    static Settings from_env()
    {
        Settings s;
        auto num = [](const char *name, long long &v) { const char *e = getenv(name); if (e) v = atoll(e); return e != nullptr; };
        long long v = 0;
        if (num("SAS_SLOTS", v) && v >= 1 && v <= kMaxSlots) s.n_slots = (int)v;
        if (num("SAS_PAIR", v)) s.pair_views = v != 0 ? 1 : 0;
        if (num("SAS_GROUP", v) && v >= 1 && v <= SAS_MAX_GROUP) s.group_views = (int)v;
        if (num("SAS_QUAD", v)) s.quad_mode = v != 0 ? 1 : 0;
        if (num("SAS_DIRECT", v)) s.direct_mode = v != 0 ? -1 : 0;
        if (num("SAS_CULL", v)) s.cull_mode = v != 0;
        if (num("SAS_SEG_FACTOR", v)) s.seg_guess_factor = (int)std::max(1ll, v);
        if (num("SAS_DIRECT_BUDGET_MB", v)) s.direct_budget = std::max(1ll, v) << 20;
        if (num("SAS_QUAD_TILES", v) && v >= 0) s.quad_max_tiles = s.quad_max_tiles_solo = (int)v;
        if (num("SAS_RING_RESTART", v)) s.ring_restart = v != 0;
        if (num("SAS_ORDER", v)) s.order_on_device = v != 0;
        if (num("SAS_KNN_GRID", v) && v >= 1 && v <= SAS_KNN_MAX_AXIS) s.knn_grid = (int)v;
        if (num("SAS_SKIN_LDS", v) && v >= 0) s.skin_lds = (int)std::min<long long>(v, SAS_SKIN_LDS_BYTES);
        if (num("SAS_SKIN_GRAD_LDS", v) && v >= 0) s.skin_grad_lds = (int)std::min<long long>(v, SAS_SKIN_GRAD_LDS_MAX);
        if (num("SAS_SKIN_GRAD_STAGED", v)) s.skin_grad_staged = v != 0 ? 1 : 0;
        return s;
    }
};

// What the context stores (sas_ctx::have).  Features and meshes sit beside a scene, mesh features beside both: forget() drops a
// store together with what sits beside it, and is the only place a bit is cleared; each store has one line that sets its bit.
// Vertex attributes (sas_scene_mesh_vertex_attributes) sit beside the meshes.
enum : unsigned { HAVE_SCENE = 1, HAVE_FEAT = 2, HAVE_MESH = 4, HAVE_MESH_FEAT = 8, HAVE_MESH_ATTR = 16 };

struct sas_ctx : Settings {
    int device = 0;
    std::string err;
    // scene
    Planes planes;
    DevBuf feat;        // feature store (sas_scene_features): [chunks][n_pad][SAS_FEAT_K], slot order
    int feat_c = 0;      // its channels
    bool feat_onehot = false, mesh_feat_onehot = false;   // the store / the triangles' rows are the one-hot of the groups (label frames)
    DevBuf mesh_vert, mesh_tri, mesh_col;   // meshes (sas_scene_meshes): float4 vertices, int4 (i0, i1, i2, group), float4 colours
    SasMeshScene mesh{};
    DevBuf mesh_nrm, mesh_vcol;   // vertex attributes (sas_scene_mesh_vertex_attributes): float4 normals, float4 colours, [mesh.nv] each
    bool mesh_has_vcol = false;   // ... colours were given
    DevBuf mesh_feat;        // per-triangle feature rows (sas_scene_mesh_features): [chunks][nt][SAS_FEAT_K], feat_c channels
    DevBuf query_pts, query_tri, query_mesh, query_list, query_count;   // scratch of sas_query_meshes (SasQuery)
    DevBuf match_src, match_tgt, match_keys, match_index, match_dist2, match_partial;   // scratch of sas_match_points (SasMatch)
    DevBuf cloud_par, cloud_grid, cloud_cand, cloud_blk, cloud_rows, cloud_dist, cloud_count;   // scratch of sas_sample_points (SasCloud)
    DevBuf fuse_par;   // per-view rows and keep table of sas_fuse_depth (SasFuse)
    Adam adam;            // optimiser state of the resident scene
    Event adam_done;      // recorded behind a step on the caller's stream: the slots' streams wait for it
    Skin skin;            // skin of the resident scene
    Event skin_done;      // recorded behind sas_scene_skin / sas_scene_deform on the caller's stream, as adam_done
    Event skin_grad_done; // recorded behind sas_scene_deform_backward's launches: the next call's stream waits for it before it zeroes the accumulator
    DevBuf grad_screen;   // sas_render_backward: [10 n] screen-space sums + [ceil(n / 256)][12] view-matrix rows (SasGradProj)
    int grad_frame = 0;   // the last frame is a backward frame: 1 of sas_render_backward_screen, 2 of sas_render_backward (grad_screen holds its sums); 0: none
    Event density_done;   // recorded behind sas_density_accumulate / sas_scene_reset_opacity / sas_scene_mcmc_noise on the caller's stream: the slots' streams wait for it
    DevBuf density_inv, density_cls, density_blk;   // scratch of sas_scene_densify (SasDensity); sas_scene_mcmc_refine shares inv and blk
    DevBuf mcmc_u32, mcmc_u64, mcmc_reloc;          // scratch of sas_scene_mcmc_refine (SasMcmc): weight | copies, prefix, reloc
    DevBuf order_key, order_idx, order_table, order_rec;   // scratch of device_order (SasOrder): keys x 2, indices x 2, histogram table, partials + record
    Event order_done;     // recorded behind device_order's launches: the next call's stream waits for it before it reuses the scratch
    DevBuf knn_pts, knn_table, knn_left, knn_keys, knn_rec;   // scratch of sas_knn_points (SasKnn): cell-ordered points, cell table + block sums, leftover list, slice keys, records
    Event knn_done;       // recorded behind sas_knn_points' launches, as order_done
    DevBuf nodes_partial; // scratch of sas_nodes_rigidity: SAS_NODES_MAX_PARTIALS doubles, allocated by a context's first call
    Event nodes_done;     // recorded behind sas_nodes_rigidity's launches, as knn_done
    // host clock of the last sas_scene_densify / sas_scene_mcmc_refine: classes, scatter, storage order, relayout + state + commit.  With the
    // order on the device (the default) laps 1 and 2 clock the ENQUEUE of the scatter and of the order; the kernels' time falls into lap 3,
    // whose wait is the first behind them.  SAS_ORDER=0: lap 1 ends behind the read-back, lap 2 is the host sort.
    float densify_ms[4] = {0, 0, 0, 0};
    DevBuf loss_scratch;  // sas_photometric_loss: [9 H W] partial planes + [tiles][4] workgroup sums + D (SasLoss)
    int match_cus = 0;   // compute units of the device, asked once (the slice count of sas_match_points)
    DevBuf host_stage;   // device staging of sas_render_batch_host's uint8 frames
    // answer of the pinned-memory query for the host buffer of the sas_render_batch_host call being served (cleared when
    // the call returns: nothing is remembered across calls)
    const uint8_t *host_query_base = nullptr, *host_query_end = nullptr;
    bool host_query_ok = false;
    SasScene scene{};
    unsigned have = 0;   // HAVE_*: the stores that are valid
    std::vector<float> group_host;    // [n_groups * 12] current poses: what a frame submitted now is rendered with
    LinkConsts links;
    // frames
    Slot slots[kMaxSlots];
    int head = 0;        // oldest busy slot
    int inflight = 0;
    int last_slot = 0;   // most recently enqueued (parity hooks)
    hipStream_t stream = nullptr;   // caller's stream of the in-flight frames
    bool has_frame{};    // a frame of the scene as it stands has been rendered (cleared by scene_changed alone)
    static constexpr int64_t kPairMinGaussians = 500000;
    uint64_t scene_version = 0;
    int64_t frames_submitted = 0, frames_completed = 0;   // sas_frames_completed
    int64_t stats[SAS_S_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t regrows = 0;
    float stage_ms[SAS_T_COUNT] = {0, 0, 0, 0, 0, 0, 0};
    double stage_sum[SAS_T_COUNT] = {0, 0, 0, 0, 0, 0, 0};
    int64_t stage_frames = 0;
};

namespace {

int fail(sas_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

bool has(const sas_ctx *c, unsigned stores) { return (c->have & stores) == stores; }

// the prologue of every call that needs a scene in place
int need_scene(sas_ctx *c, const char *who)
{
    if (!c) return SAS_ERR_INVALID;
    return has(c, HAVE_SCENE) ? SAS_OK : fail(c, SAS_ERR_NO_SCENE, "%s before sas_scene_upload", who);
}

void forget(sas_ctx *c, unsigned stores)
{
    if (stores & HAVE_SCENE) stores |= HAVE_FEAT | HAVE_MESH;
    if (stores & (HAVE_FEAT | HAVE_MESH)) stores |= HAVE_MESH_FEAT;
    if (stores & HAVE_MESH) stores |= HAVE_MESH_ATTR;
    c->have &= ~stores;
}

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, e_ == hipErrorOutOfMemory ? SAS_ERR_OOM : SAS_ERR_HIP, "%s: %s", #expr, \
                        hipGetErrorString(e_));                                                    \
    } while (0)

// (a failure reads "<the call>(b.p): ..." and leaves the buffer as it was, as it always did in ensure)
int DevBuf::release(sas_ctx *c)
{
    DevBuf &b = *this;
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    return SAS_OK;
}

int ensure(sas_ctx *c, DevBuf &b, size_t bytes)
{
    if (bytes <= b.bytes && b.p) return SAS_OK;
    if (const int rc = b.release(c)) return rc;
    if (bytes == 0) bytes = 16;
    HIP_TRY(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return SAS_OK;
}

// ... and several buffers in the order given: the first failure is the call's.
struct Want { DevBuf &buf; size_t bytes; };
int ensure(sas_ctx *c, std::initializer_list<Want> wants)
{
    for (const Want &w : wants)
        if (const int rc = ensure(c, w.buf, w.bytes)) return rc;
    return SAS_OK;
}

// Behind the launches of a blocking call on `st`: what launching left behind, `ev` (optional) recorded behind them, the wait.
int finish_launches(sas_ctx *c, hipStream_t st, const char *what, hipEvent_t ev = nullptr)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && ev) e = hipEventRecord(ev, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(c, SAS_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SAS_OK;
}

// The optimiser state goes (a new scene, sas_scene_adam_reset): hipFree waits for the step that may still be using it.
int Adam::drop(sas_ctx *c)
{
    for (DevBuf &b : buf)
        if (const int rc = b.release(c)) return rc;
    for (bool &g : on) g = false;
    return SAS_OK;
}

int Adam::alloc(sas_ctx *c, int row, int64_t n_pad, int colour_planes, hipStream_t st, bool zero)
{
    const size_t bytes = sizeof(float4) * (size_t)n_pad * (rows[row].colour ? colour_planes : 1);
    if (const int rc = ensure(c, buf[row], bytes)) return rc;
    if (zero) HIP_TRY(c, hipMemsetAsync(buf[row].p, 0, bytes, st));
    return SAS_OK;
}

// The skin goes with its scene (sas_scene_upload): hipFree waits for the deformation that may still be using it.
int Skin::drop(sas_ctx *c)
{
    for (DevBuf *b : {&rest0, &rest1, &rest2, &idx, &w, &nodes, &grad_acc})
        if (const int rc = b->release(c)) return rc;
    k = m = 0;
    return SAS_OK;
}

// The prologue of the calls that change the scene's raw values or its count: neither has a meaning over deformed planes.
int need_unskinned(sas_ctx *c, const char *who)
{
    return c->skin.bound() ? fail(c, SAS_ERR_INVALID, "%s: scene is skinned: clear_skin() first", who) : SAS_OK;
}

// Room for `count` Gaussians: whole waves of 64 slots, and 64 slots for an empty scene.
int Planes::alloc(sas_ctx *c, int64_t count, int colour_planes)
{
    n = count;
    n_pad = (count + 63) & ~63ll;
    const size_t np = (size_t)(n_pad > 0 ? n_pad : 64), plane = sizeof(float4) * np;
    return ensure(c, {{g0, plane}, {g1, plane}, {g2, plane}, {col, plane * colour_planes}, {gid8, np}, {perm, sizeof(int) * np}});
}

// What of the resident scene a call has changed: the values in the planes; the count and the storage order too; or everything.
enum class Changed { Values, CountAndOrder, Everything };

// The one place where the context forgets what it derived from the scene as it was: the last frame and its backward status, every slot's
// kept projection records, and -- once more than values changed -- the intersection capacity and the stores that sit in storage order.
void scene_changed(sas_ctx *c, Changed what)
{
    c->has_frame = false;
    c->grad_frame = 0;
    for (Slot &sl : c->slots) {
        sl.info_kept = false;
        if (what != Changed::Values) sl.scr.cap = 0;   // re-derive the intersection capacity for the new scene
    }
    if (what != Changed::Values) forget(c, HAVE_FEAT);
    if (what == Changed::Everything) {
        c->group_host.clear();
        c->links = LinkConsts{};
    }
    c->scene_version++;
}

// 3-D Hilbert index (Skilling's transpose form), `bits` per axis.  Storage order of the scene:
// consecutive Gaussians are spatial neighbours, so a workgroup's tile window is compact.
uint32_t hilbert3(uint32_t x, uint32_t y, uint32_t z, int bits)
{
    uint32_t X[3] = {x, y, z};
    const uint32_t M = 1u << (bits - 1);
    for (uint32_t Q = M; Q > 1; Q >>= 1) {
        const uint32_t P = Q - 1;
        for (int i = 0; i < 3; ++i) {
            if (X[i] & Q) X[0] ^= P;
            else { const uint32_t t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    uint32_t t = 0;
    for (uint32_t Q = M; Q > 1; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1;
    for (int i = 0; i < 3; ++i) X[i] ^= t;
    uint32_t code = 0;
    for (int b = bits - 1; b >= 0; --b)
        for (int i = 0; i < 3; ++i) code = (code << 1) | ((X[i] >> b) & 1u);
    return code;
}

// perm[slot] = caller index, ordered by (group, Hilbert index of the mean, caller index).
void storage_order(int64_t n, const float *means, const uint8_t *gid, std::vector<int> &perm)
{
    perm.resize((size_t)n);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const float v = means[3 * i + k];
            if (std::isfinite(v)) { lo[k] = std::min(lo[k], v); hi[k] = std::max(hi[k], v); }
        }
    float inv[3];
    for (int k = 0; k < 3; ++k) inv[k] = (hi[k] > lo[k]) ? 1023.0f / (hi[k] - lo[k]) : 0.0f;
    std::vector<uint64_t> key((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        uint32_t q[3];
        for (int k = 0; k < 3; ++k) {
            const float v = means[3 * i + k];
            float u = std::isfinite(v) ? (v - lo[k]) * inv[k] : 0.0f;
            u = std::min(std::max(u, 0.0f), 1023.0f);
            q[k] = (uint32_t)u;
        }
        const uint64_t g = gid ? gid[i] : 0;
        key[(size_t)i] = (g << 32) | hilbert3(q[0], q[1], q[2], 10);
    }
    for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = (int)i;
    std::sort(perm.begin(), perm.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
}

// Host copies of a scene's means and group ids (host or device arrays; gid nullptr: no groups), and its storage order from them.  fetch
// copies with blocking calls, or on a stream it then waits for; what lies between the copies and order() is the caller's.
struct OrderInput {
    int64_t n = 0;
    std::vector<float> means;
    std::vector<uint8_t> gid;   // (empty: no groups)
    int fetch(sas_ctx *c, int64_t count, const float *src_means, const uint8_t *src_gid, bool on_stream, hipStream_t st)
    {
        n = count;
        means.resize((size_t)3 * n);
        gid.resize(src_gid ? (size_t)n : 0);
        auto copy = [&](void *dst, const void *src, size_t bytes) {
            return on_stream ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipMemcpy(dst, src, bytes, hipMemcpyDefault);
        };
        HIP_TRY(c, copy(means.data(), src_means, sizeof(float) * 3 * n));
        if (src_gid) HIP_TRY(c, copy(gid.data(), src_gid, (size_t)n));
        if (on_stream) HIP_TRY(c, hipStreamSynchronize(st));
        return SAS_OK;
    }
    void order(std::vector<int> &perm) const { storage_order(n, means.data(), gid.empty() ? nullptr : gid.data(), perm); }
};

// The same permutation on the device (sas_order.hip), from device arrays into d_perm_out: enqueued on `stream`, nothing is waited for.  The
// scratch is the context's and grows with the largest n; a call on another stream than the one before runs behind it (order_done).
// n_groups: ids at or above it are reported in the record order_record() reads (256: a byte cannot be).
int device_order(sas_ctx *c, int64_t n, const float *d_means, const uint8_t *d_gid_or_null, int *d_perm_out, hipStream_t stream, int n_groups = 256)
{
    if (n <= 0) return SAS_OK;
    SasOrder q{};
    q.means = d_means; q.gid = d_gid_or_null; q.perm = d_perm_out;
    q.n = n; q.n_tiles = (n + SAS_ORDER_TILE - 1) / SAS_ORDER_TILE;
    q.n_groups = n_groups;
    const size_t m = (size_t)n, tiles = (size_t)q.n_tiles;
    if (const int rc = ensure(c, {{c->order_key, sizeof(unsigned long long) * 2 * m}, {c->order_idx, sizeof(int) * 2 * m},
                                  {c->order_table, sizeof(unsigned) * 256 * tiles},
                                  {c->order_rec, sizeof(SasOrderRecord) + sizeof(int) * SAS_ORDER_PARTIAL * tiles}}))
        return rc;
    q.key[0] = (unsigned long long *)c->order_key.p; q.key[1] = q.key[0] + m;
    q.idx[0] = (int *)c->order_idx.p; q.idx[1] = q.idx[0] + m;
    q.table = (unsigned *)c->order_table.p;
    q.rec = (SasOrderRecord *)c->order_rec.p;
    q.partial = (int *)(q.rec + 1);
    if (!c->order_done.h) HIP_TRY(c, hipEventCreateWithFlags(c->order_done.put(), hipEventDisableTiming));
    else HIP_TRY(c, hipStreamWaitEvent(stream, c->order_done, 0));
    sas_launch_order(stream, q);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->order_done, stream));
    return SAS_OK;
}

// What the last device_order found of the group ids, once its stream has been waited for.
int order_record(sas_ctx *c, SasOrderRecord &rec)
{
    HIP_TRY(c, hipMemcpy(&rec, c->order_rec.p, sizeof(rec), hipMemcpyDeviceToHost));
    return SAS_OK;
}

int Planes::host_perm(sas_ctx *c, const int **out)
{
    if (!perm_host_valid) {
        perm_host.resize((size_t)n);
        if (n > 0) HIP_TRY(c, hipMemcpy(perm_host.data(), perm.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        perm_host_valid = true;
    }
    *out = perm_host.data();
    return SAS_OK;
}

// Camera constants in the oracle's operation order (oracle/sas_oracle.c cam_from, project_one).
void make_cam(const float *V, const float *K, int W, int H, int tile_px, SasCam &c)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) c.R[3 * i + j] = V[4 * i + j];
        c.t[i] = V[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i) {
        float d = fmaf(c.R[6 + i], c.t[2], fmaf(c.R[3 + i], c.t[1], c.R[0 + i] * c.t[0]));
        c.campos[i] = -d;
    }
    c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
    c.W = W; c.H = H;
    c.tile_px = tile_px;
    c.tw = (W + tile_px - 1) / tile_px;
    c.th = (H + tile_px - 1) / tile_px;
    c.Wf = (float)W; c.Hf = (float)H;
    const float tan_fovx = (0.5f * c.Wf) / c.fx;
    const float tan_fovy = (0.5f * c.Hf) / c.fy;
    c.lim_x_pos = fmaf(0.3f, tan_fovx, (c.Wf - c.cx) / c.fx);
    c.lim_x_neg = fmaf(0.3f, tan_fovx, c.cx / c.fx);
    c.lim_y_pos = fmaf(0.3f, tan_fovy, (c.Hf - c.cy) / c.fy);
    c.lim_y_neg = fmaf(0.3f, tan_fovy, c.cy / c.fy);
}

// (a multiple of four ints and four to spare: the projection's tail reads both arrays with 16-byte loads)
static size_t f_wg_stride(const sas_ctx *c) { return (((size_t)((c->scene.n + 255) / 256) + 3) & ~(size_t)3) + 4; }

// Tiles of the slot's frame, at the frame's own binning: 16-pixel tiles, or the 8-pixel ones of the quad layout.
int tiles_of(const Slot &sl) { return sl.cam.tw * sl.cam.th; }

// Keys the slot's frame may write: its tiles' segments (single-pass binning), else what the compact lists hold.
long long frame_cap(const Slot &sl) { return sl.direct ? (long long)tiles_of(sl) * sl.scr.seg : sl.scr.cap; }

// Entries of the slot's key and id buffers: never fewer than the compact lists need, so a launch group that goes
// two-pass as a whole (enqueue_launch) finds room in the buffers of its single-pass members.
size_t key_slots(const Slot &sl) { return (size_t)std::max(frame_cap(sl), sl.scr.cap); }

// What a buffer that a frame outgrew is grown to: the measured need + 25 % (`slack`: so that a tiny need does not
// regrow step by step).
long long grown(long long need, long long slack) { return need + need / 4 + slack; }

SasFrame frame_of(sas_ctx *c, Slot &sl, bool keep_info = false)
{
    Scratch &q = sl.scr;
    const int tiles = tiles_of(sl);
    SasFrame f{};
    f.rec = (float4 *)q.rec.p;
    f.col = (float4 *)q.col.p;
    f.info = (uint4 *)q.info.p;
    // counters block: [tickets][8 device counters, 16 class cursors][tile_count][tile_big]   (left zeroed by every frame)
    f.tickets = (unsigned *)q.counters.p;
    f.stats = (unsigned *)q.counters.p + SAS_TICKET_INTS;
    f.class_cursor = (int *)q.counters.p + SAS_TICKET_INTS + 8;
    f.stats_host = sl.stats_host;
    f.tile_count = (int *)q.counters.p + SAS_TICKET_INTS + 32;
    f.tile_big = f.tile_count + sas_count_stride(tiles);
    f.wg_base = (int *)q.wgbase.p;
    const size_t ts = sas_tile_stride(tiles);
    f.tile_offset = (int *)q.tilebuf.p;
    f.tile_cursor = (int *)q.tilebuf.p + ts;
    f.tile_order = (int *)q.tilebuf.p + 2 * ts;
    f.sort_class = (int *)q.tilebuf.p + 3 * ts;
    f.keys = (unsigned long long *)q.keys.p;
    f.sorted_ids = (int *)q.ids.p;
    f.seg = sl.direct ? (int)q.seg : 0;
    f.cap = frame_cap(sl);
    f.wg_vis = (int *)q.wgvis.p;
    f.cull = (sl.direct && c->cull_mode != 0) ? 1 : 0;
#ifdef SAS_TUNE_STATS
    keep_info = true;   // (the statistics build reads the radii in the tile kernel)
#endif
    f.keep_info = (keep_info || !sl.direct) ? 1 : 0;   // two-pass frames: k_scatter reads the rectangles
    f.group_fill = sl.args.solo ? 0 : 1;               // (measured: pair bench +1.1 % with it, the blocking frame -1.6 %: profiles/r05_ab_empty_tile_groups.txt)
    sl.info_kept = f.keep_info != 0;
    f.wg_isect16 = (sl.quad || f.cull) ? (int *)q.wgvis.p + f_wg_stride(c) : nullptr;   // the lists are not T3's: T3's count is kept beside them
    f.tile_max = (unsigned *)q.tilemax.p;
    f.group_Rt = c->scene.n_groups > 0 ? (const float *)sl.poses_dev.p : nullptr;
    f.group_host = c->scene.n_groups > 0 ? sl.poses_host.h : nullptr;
    f.n_wg = (int)std::max<int64_t>(1, (c->scene.n + 255) / 256);
    f.n_tiles = tiles;
    return f;
}

// A context that holds meshes renders SAS_FULL_SORT frames: the meshes are composited by the full path's k_blend_mesh
// (sas_scene_meshes), one view per frame.
unsigned frame_flags(const sas_ctx *c, unsigned flags) { return has(c, HAVE_MESH) ? flags | SAS_FULL_SORT : flags; }

// quad layout for views of `launch_tiles` tiles each?  By the view's own size: counting the frames in
// flight as well measured worse -- 32 Gym cameras per step in launch groups of two run 30 % faster in the quad
// layout than in the ordinary one even with four groups in flight (tools/vec_env_probe.py); what loses is a
// launch that fills the chip by itself (1 200 tiles of 640x480: docs/EXPERIMENTS.md 5.21).
bool use_quad(const sas_ctx *c, int launch_tiles, unsigned flags, bool solo)
{
    if ((flags & SAS_FULL_SORT) || !sas_tiles_lazy_quad_ok((flags & SAS_FAST_EXP) != 0)) return false;
    return c->quad_mode < 0 ? launch_tiles <= (solo ? c->quad_max_tiles_solo : c->quad_max_tiles) : c->quad_mode != 0;
}

// Can a kernel store to this host address (pinned / registered memory)?  Asked on every call: remembering the
// answer per address would be wrong the day a pinned block is freed and a pageable one takes its place.
bool kernel_can_write_host(sas_ctx *c, const void *p)
{
    // (within ONE sas_render_batch_host call the views' frames lie in one caller buffer: asked once, see host_query)
    if (c->host_query_base && p >= c->host_query_base && p < c->host_query_end) return c->host_query_ok;
    hipPointerAttribute_t at{};
    const bool ok = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();   // a pageable pointer makes the query fail: not an error of ours
    return ok;
}

// Does the tile kernel deliver this view's uint8 frame to `dst` itself?  Frame wanted in pinned host memory and every
// tile complete: it stores its rows there (no device staging frame, no copy kernel); SAS_FULL_SORT frames keep the
// staging path.  Asked per view; a batch needs its staging frames unless every view answers yes.
bool host_direct_ok(sas_ctx *c, const uint8_t *dst, int W, int H, unsigned flags)
{
    return dst && W % SAS_TILE == 0 && H % SAS_TILE == 0 && ((size_t)dst & 15) == 0 && !(flags & SAS_FULL_SORT) &&
           kernel_can_write_host(c, dst);
}

// Nothing pending on the caller's stream?
static bool stream_idle(hipStream_t s)
{
    const hipError_t e = hipStreamQuery(s);
    if (e != hipSuccess) (void)hipGetLastError();   // hipErrorNotReady is an answer, not an error of ours
    return e == hipSuccess;
}

// Group poses of the n frames (one launch): each slot's snapshot goes to its own device block, so frames in flight
// may carry different poses (vectorised envs, a pose update per Gym step) and nothing drains between them.
// `device_reader`: something besides the projection reads the block on the device, so it is uploaded even when the
// projection carries the poses itself.
void enqueue_poses(sas_ctx *c, Slot *const *sl, int n, hipStream_t st, bool device_reader = false)
{
    if (c->scene.n_groups <= 0) return;
    if (!device_reader && sas_poses_inline(c->scene.n_groups, n, n > 1)) return;   // small blocks ride in the projection's arguments
    SasPoseUpload u{};
    u.nv = n;
    for (int k = 0; k < n; ++k) {
        u.dst[k] = (float *)sl[k]->poses_dev.p;
        u.src_host[k] = sl[k]->poses_host;
        u.floats[k] = 12 * c->scene.n_groups;
    }
    sas_launch_pose_upload(st, u);
}

// Single-pass or two-pass binning for the slot's frame (sl.direct), and the length of a tile's segment (scr.seg).
// Single-pass binning: every tile owns a segment of q.seg keys.  First guess: 16 x the mean list of a frame with five
// intersections per Gaussian, a power of two (config 3: 16 384 keys = 1.6 GB of keys + ids per slot; its longest list
// is ~6 k); a frame whose longest list outgrows it is rendered again with larger segments (complete_oldest).
void choose_binning(sas_ctx *c, Slot &sl)
{
    Scratch &q = sl.scr;
    const int tiles = tiles_of(sl);
    const int64_t n = c->scene.n;
    if (q.seg_tiles != tiles || q.seg_n != n) {
        // another frame size or scene: remember what this one had learned, take up what the slot knows about the new one
        // (else 0: guessed below -- a segment length learned on a 300-tile frame says nothing about a 1 200-tile one)
        if (q.seg_tiles >= 0 && q.seg > 0) {
            int k = 0;
            while (k < 4 && !(q.seg_memo[k].tiles == q.seg_tiles && q.seg_memo[k].n == q.seg_n)) ++k;
            if (k == 4) { k = q.seg_memo_next; q.seg_memo_next = (q.seg_memo_next + 1) % 4; }
            q.seg_memo[k] = {q.seg_tiles, q.seg_n, q.seg};
        }
        q.seg = 0;
        for (const auto &m : q.seg_memo)
            if (m.tiles == tiles && m.n == n) q.seg = m.seg;
        q.seg_too_big = false;
        q.seg_tiles = tiles;
        q.seg_n = n;
    }
    sl.direct = c->direct_mode != 0 && !(sl.args.flags & SAS_FULL_SORT) && !q.seg_too_big;
    if (!sl.direct) return;
    if (q.seg == 0) {
        long long guess = c->seg_guess_factor * ((5 * n) / (tiles > 0 ? tiles : 1) + 1);
        long long s2 = 1024;
        while (s2 < guess) s2 <<= 1;
        q.seg = s2;
    }
    const long long slot_budget = c->direct_budget / std::max(1, c->n_slots);   // the budget is the context's: its slots share it
    if ((long long)tiles * q.seg * 12 > slot_budget || q.seg > (1ll << 30)) {
        sl.direct = false;          // pathological concentration (or a huge frame): the two-pass path has no such limit
        q.seg_too_big = true;
    }
}

// Key and id buffers for the binning choose_binning settled on; segments that do not fit the GPU's free memory turn
// the frame two-pass.
int ensure_keys(sas_ctx *c, Slot &sl)
{
    Scratch &q = sl.scr;
    // buffers sized for a much larger frame (or for segments the slot has since given up) go back to the allocator:
    // several contexts share a card (vectorised ranks, torch), and ensure() by itself only ever grows
    if (q.keys.bytes > 4 * sizeof(unsigned long long) * key_slots(sl) && q.keys.bytes > (256u << 20)) { (void)q.keys.release(); (void)q.ids.release(); }
    auto alloc = [&]() {
        const int rc = ensure(c, q.keys, sizeof(unsigned long long) * key_slots(sl));
        return rc ? rc : ensure(c, q.ids, sizeof(int) * key_slots(sl));
    };
    if (sl.direct && alloc()) {
        // the segments do not fit this GPU's free memory: not an error, the two-pass path needs 12 bytes per intersection only
        // (whatever of the segment-sized pair was allocated is released: the compact lists take a fraction of it)
        (void)hipGetLastError();
        c->err.clear();
        (void)q.keys.release();
        (void)q.ids.release();
        sl.direct = false;
        q.seg_too_big = true;
    }
    return alloc();
}

// The parameter block of the slot's frame (it travels in the argument segment of every kernel of the frame), and
// who delivers a frame wanted on the host.
void fill_params(sas_ctx *c, Slot &sl)
{
    const RenderArgs &a = sl.args;
    const ViewOut &o = a.out;
    sl.host_direct = host_direct_ok(c, o.rgb8_host, a.W, a.H, a.flags);
    SasParams &hp = sl.params;
    hp.cam = sl.cam;
    hp.out.rgb = o.rgb; hp.out.alpha = o.alpha; hp.out.depth = o.depth;
    hp.out.rgb8 = sl.host_direct ? nullptr : o.rgb8;
    hp.out.rgb8_host = sl.host_direct ? o.rgb8_host : nullptr;
    hp.out.bg[0] = a.bg[0]; hp.out.bg[1] = a.bg[1]; hp.out.bg[2] = a.bg[2];
    hp.out.points = o.points; hp.out.mask = o.mask;
    hp.out.max_depth = a.max_depth; hp.out.use_max_depth = a.use_max_depth ? 1 : 0;
    hp.out.n_pixels = (long long)a.W * a.H;
}

// Camera constants, scratch and the parameter block of the slot's frame.  `init_st`: the stream the frame's
// projection will run on (the slot's own, or its pair / group leader's): a new counter block is cleared there.
int prepare_frame(sas_ctx *c, Slot &sl, hipStream_t init_st)
{
    const RenderArgs &a = sl.args;
    // The layout is a property of the whole frame: in the quad layout the view is BINNED in 8-pixel tiles (every 8x8
    // quadrant has its own list), so the choice is made here, in front of the projection.
    const int tiles16 = ((a.W + SAS_TILE - 1) / SAS_TILE) * ((a.H + SAS_TILE - 1) / SAS_TILE);
    sl.quad = use_quad(c, tiles16, a.flags, a.solo) && a.W <= 65535 * (SAS_TILE / 2) && a.H <= 65535 * (SAS_TILE / 2);   // (tile coordinates are 16 bits in info)
    make_cam(a.viewmat, a.K, a.W, a.H, sl.quad ? SAS_TILE / 2 : SAS_TILE, sl.cam);
    const int tiles = tiles_of(sl);
    const int64_t n = c->scene.n;
    Scratch &q = sl.scr;
    int rc;
    if (q.cap == 0) {
        // 8 intersections per Gaussian to start with (trained scenes and the BASELINE configs need 4-5);
        // 12 bytes each: 96 MB per slot at 1 M Gaussians.  A frame that needs more is rendered again.
        long long want = 8 * (long long)n;
        if (want < (1ll << 20)) want = 1ll << 20;
        q.cap = want;
    }
    if ((rc = ensure(c, q.rec, sizeof(float4) * SAS_RS * (size_t)(n > 0 ? n : 1)))) return rc;
    if ((rc = ensure(c, q.col, sizeof(float4) * (size_t)(n > 0 ? n : 1)))) return rc;
    if ((rc = ensure(c, q.info, sizeof(uint4) * (size_t)(n > 0 ? n : 1)))) return rc;
    if ((rc = ensure(c, q.tilebuf, sizeof(int) * (3 * sas_tile_stride(tiles) + 16)))) return rc;
    {
        const size_t cb = sizeof(int) * sas_counter_ints(tiles);
        if (cb > q.counters.bytes || !q.counters.p) q.counters_zero = false;
        if ((rc = ensure(c, q.counters, cb))) return rc;
        if (!q.counters_zero) {   // new block, or a frame that failed half way: zero all of it once, on the slot's stream
            HIP_TRY(c, hipMemsetAsync(q.counters.p, 0, q.counters.bytes, init_st));
            q.counters_zero = true;
        }
    }
    if ((rc = ensure(c, q.wgvis, sizeof(int) * 2 * f_wg_stride(c)))) return rc;   // visible counts | 16-pixel intersections (quad layout)
    if ((rc = ensure(c, q.wgbase, sizeof(int) * SAS_WIN_BINS * (size_t)((n + 255) / 256 + 1)))) return rc;
    if ((rc = ensure(c, q.tilemax, sizeof(unsigned) * (size_t)tiles))) return rc;
    choose_binning(c, sl);
    if ((rc = ensure_keys(c, sl))) return rc;
    if (c->scene.n_groups > 0 && (rc = ensure(c, sl.poses_dev, sizeof(float) * 12 * 256))) return rc;
    fill_params(c, sl);
    return SAS_OK;
}

// Mesh scratch of the slot's frame: 2 records per triangle, the tile counts / offsets / cursors, the lists (first guess: four
// tiles per record; a frame whose lists outgrow it is rendered again with the measured need, as for the splat keys).
// The meshes as a frame's setup kernel takes them: with their vertex attributes while the context holds any.
SasMeshScene mesh_scene_of(const sas_ctx *c)
{
    SasMeshScene m = c->mesh;
    const bool attr = has(c, HAVE_MESH_ATTR);
    m.vnormal = attr ? (const float4 *)c->mesh_nrm.p : nullptr;
    m.vcolor = attr && c->mesh_has_vcol ? (const float4 *)c->mesh_vcol.p : nullptr;
    return m;
}

int prepare_mesh(sas_ctx *c, MeshScratch &m, int tiles, size_t feature_pixels)
{
    const size_t nrec = 2 * (size_t)c->mesh.nt;
    int rc;
    if (m.cap == 0) m.cap = std::max<long long>(1 << 16, 4 * (long long)nrec);
    if ((rc = ensure(c, m.rec, sizeof(float4) * 4 * nrec))) return rc;
    if ((rc = ensure(c, m.rect, sizeof(int4) * nrec))) return rc;
    if ((rc = ensure(c, m.tiles, sizeof(int) * (3 * sas_tile_stride(tiles) + 16)))) return rc;
    if (has(c, HAVE_MESH_ATTR) && (rc = ensure(c, m.planes, sizeof(float4) * SAS_MESH_PLANE_STRIDE * nrec))) return rc;
    if (feature_pixels && (rc = ensure(c, m.win, sizeof(unsigned long long) * feature_pixels))) return rc;
    return ensure(c, m.list, sizeof(int) * (size_t)m.cap);
}

SasMeshFrame mesh_frame_of(const sas_ctx *c, const MeshScratch &m, int tiles)
{
    const size_t ts = sas_tile_stride(tiles);
    SasMeshFrame mf{};
    mf.rec = (float4 *)m.rec.p;
    mf.rect = (int4 *)m.rect.p;
    mf.tile_count = (int *)m.tiles.p;
    mf.tile_offset = (int *)m.tiles.p + ts;
    mf.tile_cursor = (int *)m.tiles.p + 2 * ts;
    mf.list = (int *)m.list.p;
    mf.cap = m.cap;
    mf.n_rec = 2 * c->mesh.nt;
    mf.status_host = m.status_host;
    return mf;
}

SasFeatures features_of(const sas_ctx *c, const RenderArgs &a)
{
    SasFeatures F{};
    F.store = (const float *)c->feat.p;
    F.out = a.out.features;
    F.n_pad = c->scene.n_pad;
    F.C = a.feat_c;
    F.chunks = sas_feature_chunks(a.feat_c);
    memcpy(F.bg, a.fbg, sizeof(float) * (size_t)a.feat_c);
    return F;
}

SasLabels labels_of(const sas_ctx *c, const RenderArgs &a)
{
    SasLabels B{};
    B.store = (const float *)c->feat.p;
    B.n_pad = c->scene.n_pad;
    B.C = c->feat_c;
    B.chunks = sas_feature_chunks(c->feat_c);
    B.out = a.out.labels;
    B.min_alpha = a.min_alpha;
    B.surface = (a.flags & SAS_MESH_SURFACE) != 0;
    return B;
}

// Frames wanted on the host (sas_render_batch_host) and not delivered by the tile kernel: one copy kernel for the
// chain's views when the destination is pinned (no copy-engine hop), else a runtime copy per view.
int deliver_to_host(sas_ctx *c, Slot *const *sl, int nv, hipStream_t st)
{
    SasHostCopy h{};
    h.nv = nv;
    h.bytes = 3 * (size_t)sl[0]->args.W * (size_t)sl[0]->args.H;
    const uint8_t *first = nullptr;
    for (int k = 0; k < nv; ++k) {
        const ViewOut &o = sl[k]->args.out;
        h.src[k] = (o.rgb8_host && !sl[k]->host_direct) ? o.rgb8 : nullptr;
        h.dst[k] = o.rgb8_host;
        if (h.src[k] && !first) first = o.rgb8_host;
    }
    if (!first) return SAS_OK;
    if (kernel_can_write_host(c, first)) sas_launch_host_copy(st, h);
    else
        for (int k = 0; k < nv; ++k)
            if (h.src[k]) HIP_TRY(c, hipMemcpyAsync(h.dst[k], h.src[k], h.bytes, hipMemcpyDeviceToHost, st));
    return SAS_OK;
}

// The frames of nv prepared views as ONE chain of launches on the first view's stream (the slots must be idle on the
// GPU).  nv > 1 is a launch group: same-sized views that share every launch (grid.y = view) -- a Gym step's cameras on a
// small scene are launch-bound, and the group's kernels also fill more of the chip.  The two chains of a view pair
// (sas_render_batch) share one projection: the leader's chain (`follower` set) runs one two-view pass over the scene,
// whose tail scans both views' counts; the follower's chain (`leader` set) waits for it and continues with its own
// binning and tiles.
int enqueue_chain(sas_ctx *c, Slot *const *sl, int nv, Slot *follower = nullptr, Slot *leader = nullptr)
{
    Slot &ld = *sl[0];
    const RenderArgs &a = ld.args;   // (size and flags are the same for all views of a group)
    hipStream_t st = ld.fs;
    const int tiles = tiles_of(ld);
    const bool timing = (a.flags & SAS_TIMING) != 0;   // timed and full-sort frames are one view per chain (render_batch_impl)
    const bool full = (a.flags & SAS_FULL_SORT) != 0;
    const bool ttiles = (a.flags & SAS_TIME_TILES) != 0 && !timing && !full;
    const bool fast_exp = (a.flags & SAS_FAST_EXP) != 0;
    int rc;
    SasFrame fr[SAS_MAX_GROUP];
    bool writes_caller = false, any_fill = false;
    for (int k = 0; k < nv; ++k) {
        fr[k] = frame_of(c, *sl[k]);
        writes_caller = writes_caller || sl[k]->args.order_caller;
        any_fill = any_fill || (sl[k]->args.out.depth && (a.flags & SAS_DEPTH_FILL_MAX));
        sl[k]->mesh = full && has(c, HAVE_MESH) && c->mesh.nt > 0;   // a frame with meshes: always SAS_FULL_SORT, a view of its own
    }
    const SasFrame &f = fr[0];
    const SasParams &P = ld.params;
    SasMulti mf;   // a launch group's views as its launches take them (3 KB by value: not built for a single view)
    if (nv > 1) {
        mf = SasMulti{};
        mf.nv = nv;
        for (int k = 0; k < nv; ++k) { mf.f[k] = fr[k]; mf.P[k] = sl[k]->params; }
    }

    // ORDER.  The chain runs after whatever the caller has enqueued on its stream so far: `start` is recorded there
    // and waited for -- by timed frames as a whole, by the others in front of the first launch that writes an output
    // buffer (the tile / blend kernel, or the sort of a full-sort frame; everything before touches only the scene and
    // the slots' scratch).
    // (a blocking single frame whose caller's stream has nothing pending needs no ordering: one query instead of an event
    // record, a stream wait and the wait packet between the scatter and the tile kernel -- +2.4 % on the blocking
    // config-3 frame; pipelined frames keep the event: no gain measured there)
    const bool order = timing || (writes_caller && !(a.solo && stream_idle(a.stream)));
    if (order) HIP_TRY(c, hipEventRecord(ld.start, a.stream));
    if (timing) HIP_TRY(c, hipStreamWaitEvent(st, ld.start, 0));

    const bool per_pixel_win = a.out.features || a.out.labels;   // the feature / label kernels take every pixel's triangle from the blend
    if (ld.mesh && (rc = prepare_mesh(c, ld.msc, tiles, per_pixel_win ? (size_t)a.W * (size_t)a.H : 0))) return rc;
    if (leader) {
        HIP_TRY(c, hipStreamWaitEvent(st, leader->pair_ev, 0));   // projected by the leader's pass
    } else {
        // (a pair shares its poses: the leader's block serves both views; the triangle setup of a mesh frame reads the
        // slot's poses on the device)
        enqueue_poses(c, sl, nv, st, ld.mesh || a.out.chained());   // (k_grad_project reads the poses on the device)
        if (timing) HIP_TRY(c, hipEventRecord(ld.ev[0], st));
        if (follower) {
            sas_launch_project2(st, c->scene, P, f, follower->params, frame_of(c, *follower));
            HIP_TRY(c, hipEventRecord(ld.pair_ev, st));
        } else if (nv > 1) {
            sas_launch_project_multi(st, c->scene, mf);
        } else {
            sas_launch_project(st, c->scene, P, f);
        }
    }
    if (timing) {
        HIP_TRY(c, hipEventRecord(ld.ev[1], st));
        HIP_TRY(c, hipEventRecord(ld.ev[2], st));   // SAS_T_SCAN: the scan is the projection's tail
    }
    if (!ld.direct) {   // (single-pass binning: keys and tile order are in place when the projection ends)
        if (nv > 1) sas_launch_scatter_multi(st, c->scene, ld.cam.tw, mf);
        else sas_launch_scatter(st, c->scene, ld.cam.tw, f);
    }
    if (timing) HIP_TRY(c, hipEventRecord(ld.ev[3], st));
    if (order && !timing) HIP_TRY(c, hipStreamWaitEvent(st, ld.start, 0));
    if (full) sas_launch_sort(st, c->scene, tiles, f, ld.sort_streams);
    if (timing) HIP_TRY(c, hipEventRecord(ld.ev[4], st));
    hipEvent_t tile_ev[2] = {ttiles ? ld.ev[4] : nullptr, ttiles ? ld.ev[5] : nullptr};
    if (ld.mesh) {
        const SasMeshFrame mesh = mesh_frame_of(c, ld.msc, tiles);
        float4 *planes = has(c, HAVE_MESH_ATTR) ? (float4 *)ld.msc.planes.p : nullptr;
        sas_launch_mesh_bin(st, mesh_scene_of(c), P, f, mesh, planes);
        const SasMeshExtra extra{per_pixel_win ? (unsigned long long *)ld.msc.win.p : nullptr, (a.flags & SAS_MESH_SURFACE) != 0};
        sas_launch_blend_mesh(st, c->scene, tiles, P, f, mesh, extra, planes, fast_exp, any_fill);
        if (a.out.features) {   // ... in front of the triangles the blend kernel has just resolved (extra.win)
            const SasMeshFeatures MF{extra.win, (const float *)c->mesh_feat.p, c->mesh.nt};
            sas_launch_blend_features(st, c->scene, tiles, P, f, features_of(c, a), fast_exp, &MF);
        }
        if (a.out.labels) {
            const SasMeshFeatures MF{extra.win, (const float *)c->mesh_feat.p, c->mesh.nt};
            sas_launch_blend_labels(st, c->scene, tiles, P, f, labels_of(c, a), fast_exp, &MF);
        }
    } else if (full) {
        sas_launch_blend(st, c->scene, tiles, P, f, fast_exp, any_fill);
        // a feature frame (sas_render_features): the same lists and records once more, per chunk of channels
        if (a.out.features) sas_launch_blend_features(st, c->scene, tiles, P, f, features_of(c, a), fast_exp, nullptr);
        if (a.out.labels) sas_launch_blend_labels(st, c->scene, tiles, P, f, labels_of(c, a), fast_exp, nullptr);   // a label frame: likewise
        switch (a.out.reader) {
        case ViewOut::NO_READER: break;
        case ViewOut::LIFT_LABELS:   // a lift frame: the same lists, the weights handed back to their Gaussians
            sas_launch_lift_labels(st, c->scene, tiles, P, f, a.out.lift, fast_exp);
            break;
        case ViewOut::LIFT_FEATURES:   // ... or, channel by channel, the pixels' features weighted by them
            sas_launch_lift_features(st, c->scene, tiles, P, f, a.out.lift_features, fast_exp);
            break;
        case ViewOut::BACKWARD:   // a backward frame: the same lists walked there and back (sas_grad.hip)
            sas_launch_grad_tiles(st, c->scene, tiles, P, f, a.out.back.tiles, fast_exp);
            if (a.out.chained()) sas_launch_grad_project(st, c->scene, P, f, a.out.back.proj, a.out.back.poses);
            break;
        }
    } else if (nv > 1) {
        // (quad: by the size of one view (prepare_frame): groups of four 300-tile views still gain (vec_env_probe))
        sas_launch_tiles_lazy_multi(st, c->scene, tiles, mf, fast_exp, any_fill, ld.quad, tile_ev[0], tile_ev[1]);
    } else {
        sas_launch_tiles_lazy(st, c->scene, tiles, P, f, fast_exp, any_fill, ld.quad, tile_ev[0], tile_ev[1]);
    }
    if (timing) HIP_TRY(c, hipEventRecord(ld.ev[5], st));
    for (int k = 0; k < nv; ++k) {
        const ViewOut &o = sl[k]->args.out;
        const bool fill = o.depth && (a.flags & SAS_DEPTH_FILL_MAX);
        const bool pts = o.depth && (o.points || o.mask);
        if (fill || pts) sas_launch_depth_tail(st, tiles, sl[k]->params, fr[k], fill, pts);
    }
    if (timing) HIP_TRY(c, hipEventRecord(ld.ev[6], st));
    if ((rc = deliver_to_host(c, sl, nv, st))) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ld.done, st));   // the chain completes as a whole
    for (int k = 0; k < nv; ++k) {
        sl[k]->busy = true;
        sl[k]->timed = k == 0 && timing;
        sl[k]->timed_tiles = k == 0 && ttiles;
        sl[k]->group = k == 0 ? nv : 0;
    }
    c->has_frame = true;
    c->grad_frame = 0;   // (the backward calls set it once their frame is complete)
    return SAS_OK;
}

// Enqueue the views of the consecutive idle slots sl[0..n-1] (args and pose snapshots filled): one view, a launch
// group of n, or -- `pair` -- two views that share one pass over the scene.  The only way frames reach the GPU.
int enqueue_launch(sas_ctx *c, Slot *const *sl, int n, bool pair = false)
{
    int rc;
    for (int k = 0; k < n; ++k)   // counters are cleared on the stream that runs the projection: the leader's
        if ((rc = prepare_frame(c, *sl[k], sl[0]->fs))) return rc;
    if (pair) {
        if ((rc = enqueue_chain(c, sl, 1, sl[1], nullptr))) return rc;
        return enqueue_chain(c, sl + 1, 1, nullptr, sl[0]);
    }
    // one launch, one binning scheme: single-pass only when every view of the group has its segments
    bool all_direct = true;
    for (int k = 0; k < n; ++k) all_direct = all_direct && sl[k]->direct;
    for (int k = 0; k < n; ++k) sl[k]->direct = all_direct;
    return enqueue_chain(c, sl, n);
}

// After a failure somewhere inside a frame's enqueue the counters can no longer be assumed zero.
void mark_dirty(sas_ctx *c)
{
    (void)hipDeviceSynchronize();
    for (Slot &sl : c->slots) sl.scr.counters_zero = false;
}

// What the g frames of a finished launch report (sas_frame_stats: the last one stays).  Did one outgrow a buffer?
bool read_stats(sas_ctx *c, Slot *const *mem, int g)
{
    bool overflow = false;
    for (int k = 0; k < g; ++k) {
        const volatile unsigned *s = mem[k]->stats_host;   // written by the projection's tail (+ the tile kernel's [6])
        c->stats[SAS_S_NVISIBLE] = s[0];
        c->stats[SAS_S_NISECT] = s[3];   // intersections with the contract's 16-pixel tiles ([1]: keys written, at the frame's own binning)
        c->stats[SAS_S_NKEYS] = s[1];
        c->stats[SAS_S_MAX_TILE_LEN] = s[4];
        c->stats[SAS_S_CAPACITY] = frame_cap(*mem[k]);
        c->stats[SAS_S_REGROWS] = c->regrows;
        c->stats[SAS_S_WINDOW_MISSES] = s[5];
        c->stats[SAS_S_FALLBACK_TILES] = s[6];
        c->stats[SAS_S_QUAD_LAYOUT] = mem[k]->quad ? 1 : 0;
        c->stats[SAS_S_LAUNCH_VIEWS] = g;
        overflow = overflow || s[2] != 0 || (mem[k]->mesh && mem[k]->msc.status_host[1] != 0);
    }
    return overflow;
}

void read_stage_times(sas_ctx *c, const Slot &sl)
{
    if (sl.timed) {
        for (int k = 0; k < 6; ++k) (void)hipEventElapsedTime(&c->stage_ms[k], sl.ev[k], sl.ev[k + 1]);
        (void)hipEventElapsedTime(&c->stage_ms[SAS_T_TOTAL], sl.ev[0], sl.ev[6]);
        for (int k = 0; k < SAS_T_COUNT; ++k) c->stage_sum[k] += c->stage_ms[k];
        c->stage_frames++;
    } else if (sl.timed_tiles) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sl.ev[4], sl.ev[5]) == hipSuccess) {
            c->stage_ms[SAS_T_BLEND] = ms;
            c->stage_sum[SAS_T_BLEND] += ms;
            c->stage_frames++;
        }
    }
}

// A launch outgrew its intersection buffers (or a mesh frame its triangle lists): grow them to the measured need.
void grow_scratch(sas_ctx *c, Slot *const *mem, int g)
{
    long long want = 0, want_seg = 0;
    for (int k = 0; k < g; ++k) {
        MeshScratch &m = mem[k]->msc;
        if (mem[k]->mesh && m.status_host[1] != 0) m.cap = std::max(m.cap, grown((long long)m.status_host[0], 1024));
        want = std::max(want, grown((long long)mem[k]->stats_host[1], 1024));
        if (mem[k]->direct) {   // single-pass binning: the longest list, as a power of two
            long long s2 = mem[k]->scr.seg;
            while (s2 < grown((long long)mem[k]->stats_host[4], 0)) s2 <<= 1;
            want_seg = std::max(want_seg, s2);
        }
    }
    for (int k = 0; k < g; ++k) {
        if (mem[k]->direct) { if (want_seg > mem[k]->scr.seg) mem[k]->scr.seg = want_seg; }
        else if (want > mem[k]->scr.cap) mem[k]->scr.cap = want;
    }
    const Scratch &q = mem[0]->scr;
    for (Slot &o : c->slots) {   // the other slots will need it too (those set up for the same frame size and scene)
        if (o.busy) continue;
        if (want_seg && o.scr.seg && o.scr.seg < want_seg && o.scr.seg_tiles == q.seg_tiles && o.scr.seg_n == q.seg_n) o.scr.seg = want_seg;
        if (!want_seg && o.scr.cap && o.scr.cap < want) o.scr.cap = want;
    }
}

// Verify the oldest in-flight launch; on overflow grow its buffers and render it again.
int complete_oldest(sas_ctx *c)
{
    if (c->inflight <= 0) return SAS_OK;
    Slot &sl = c->slots[c->head];
    const int g = sl.group > 1 ? sl.group : 1;   // a launch group completes as a whole (one stream, one done event)
    Slot *mem[SAS_MAX_GROUP];
    for (int k = 0; k < g; ++k) mem[k] = &c->slots[(c->head + k) % c->n_slots];
    for (int attempt = 0; attempt < 4; ++attempt) {
        HIP_TRY(c, hipEventSynchronize(sl.done));
        const bool overflow = read_stats(c, mem, g);
        read_stage_times(c, sl);
        if (!overflow) {
            // Only now -- the host has seen the frame finished AND that it did not overflow its intersection buffer -- may
            // the frame be consumed.  Whatever the caller puts on its stream from here on starts after the frame in real
            // time: the frame's done event has been waited for by the host (above), so a stream wait on it would be a
            // no-op on the GPU and one more runtime call and barrier packet per frame (it was issued until round 3).
            for (int k = 0; k < g; ++k) {
                mem[k]->busy = false;
                mem[k]->group = 1;
            }
            c->head = (c->head + g) % c->n_slots;
            c->inflight -= g;
            c->frames_completed += g;
            return SAS_OK;
        }
        // render the launch again, with the poses it was submitted with (the slots' snapshots): a group as a group, a
        // single view or a member of a view pair as a single view
        grow_scratch(c, mem, g);
        c->regrows++;
        const int rc = enqueue_launch(c, mem, g);
        if (rc) { mark_dirty(c); return rc; }
    }
    return fail(c, SAS_ERR_HIP, "intersection buffer kept overflowing");
}

int complete_all(sas_ctx *c)
{
    while (c->inflight > 0)
        if (const int rc = complete_oldest(c)) return rc;
    return SAS_OK;
}

// A caller's `count` floats where a kernel can read them: in place when device memory of this context's device, else copied into `stage`.
int device_floats(sas_ctx *c, const float *p, size_t count, DevBuf &stage, const float **out)
{
    hipPointerAttribute_t at{};
    const bool on_device = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == c->device;
    (void)hipGetLastError();   // (a plain host pointer leaves an error behind on some runtimes)
    *out = p;
    if (on_device) return SAS_OK;
    if (const int rc = ensure(c, stage, sizeof(float) * count)) return rc;
    const hipError_t e = hipMemcpy(stage.p, p, sizeof(float) * count, hipMemcpyDefault);
    if (e != hipSuccess) return fail(c, SAS_ERR_HIP, "feature copy: %s", hipGetErrorString(e));
    *out = (const float *)stage.p;
    return SAS_OK;
}

// sas_scene_features / sas_scene_mesh_features once validated and with no frame in flight: size the store ([chunks][stride][SAS_FEAT_K]),
// bring the caller's rows to the device (nullptr: one-hot), launch on the context's own, idle stream (slot 0's) and wait for it alone.
template <class Launch>
int fill_feature_store(sas_ctx *c, DevBuf &store, size_t stride, int channels, const float *rows, size_t n_rows, const char *what,
                       Launch launch)
{
    int rc;
    if ((rc = ensure(c, store, sizeof(float) * SAS_FEAT_K * (size_t)sas_feature_chunks(channels) * stride))) return rc;
    const float *src = nullptr;
    DevBuf stage;
    if (rows && n_rows > 0 && (rc = device_floats(c, rows, n_rows * (size_t)channels, stage, &src))) return rc;
    hipStream_t st = c->slots[0].fs;
    launch(st, src, (float *)store.p);
    return finish_launches(c, st, what);
}

}  // namespace

extern "C" {

const char *sas_version(void) { return "sim_a_splat_amd 0.1 (gfx950)"; }

int sas_create(int device, sas_ctx **out)
{
    if (!out) return SAS_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SAS_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return SAS_ERR_INVALID;
    sas_ctx *c = new (std::nothrow) sas_ctx();
    if (!c) return SAS_ERR_OOM;
    c->device = device;
    static_cast<Settings &>(*c) = Settings::from_env();
    bool ok = hipSetDevice(device) == hipSuccess;
    for (Slot &sl : c->slots) ok = ok && sl.init() == hipSuccess;
    if (!ok) {
        delete c;
        return SAS_ERR_HIP;
    }
    *out = c;
    return SAS_OK;
}

int sas_destroy(sas_ctx *c)
{
    if (!c) return SAS_ERR_INVALID;
    (void)hipSetDevice(c->device);
    for (Slot &sl : c->slots)   // frames may still be in flight: nothing is given back under them
        for (hipStream_t st : {(hipStream_t)sl.fs, (hipStream_t)sl.side[0], (hipStream_t)sl.side[1]})
            if (st) (void)hipStreamSynchronize(st);
    delete c;
    return SAS_OK;
}

const char *sas_last_error(sas_ctx *c) { return c ? c->err.c_str() : "null context"; }

int sas_scene_upload(sas_ctx *c, int64_t n, const float *means, const float *quats, const float *scales,
                     const float *cov6, const float *opacities, const float *colors, int sh_degree,
                     const uint8_t *group_id, int n_groups)
{
    if (!c) return SAS_ERR_INVALID;
    if (n < 0 || n > 0x7fffffffll) return fail(c, SAS_ERR_INVALID, "n=%lld out of range", (long long)n);
    if (sh_degree > 3) return fail(c, SAS_ERR_INVALID, "sh_degree %d > 3", sh_degree);
    if (n > 0 && (!means || !opacities || !colors)) return fail(c, SAS_ERR_INVALID, "means/opacities/colors required");
    const bool quat_mode = quats && scales;
    if (n > 0 && !quat_mode && !cov6) return fail(c, SAS_ERR_INVALID, "need quats+scales or cov6");
    if (n_groups < 0 || n_groups > 256) return fail(c, SAS_ERR_INVALID, "n_groups %d out of [0,256]", n_groups);
    if (group_id && n_groups <= 0) return fail(c, SAS_ERR_INVALID, "group_id given but n_groups == 0");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    forget(c, HAVE_SCENE);
    if (const int rc = c->adam.drop(c)) return rc;   // (hipFree waits for the step that may still be using the state)
    if (const int rc = c->skin.drop(c)) return rc;   // (the scene is new)

    const int deg = sh_degree < 0 ? -1 : sh_degree;
    const int coeff_floats = sas_coeff_floats(deg), planes = sas_colour_planes(deg);
    Planes &pl = c->planes;
    int rc;
    if ((rc = pl.alloc(c, n, planes))) return rc;
    pl.forget_host_perm();
    if (n > 0) {
        if (!c->order_on_device) {
            // SAS_ORDER=0: storage order from host copies of the means / group ids
            OrderInput in;
            if ((rc = in.fetch(c, n, means, group_id, false, nullptr))) return rc;
            for (int64_t i = 0; i < n && group_id; ++i)
                if (in.gid[(size_t)i] >= n_groups) return fail(c, SAS_ERR_INVALID, "group_id[%lld]=%d >= n_groups=%d", (long long)i, (int)in.gid[(size_t)i], n_groups);
            in.order(pl.perm_host);
            pl.perm_host_valid = true;
            HIP_TRY(c, hipMemcpy(pl.perm.p, pl.perm_host.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        }

        // stage the caller's arrays (host or device) and re-lay them out on the device
        DevBuf s_means, s_q, s_s, s_cov, s_op, s_col, s_gid;
        auto stage = [&](DevBuf &b, const void *src, size_t bytes) -> int {
            if (const int rc = ensure(c, b, bytes)) return rc;
            HIP_TRY(c, hipMemcpy(b.p, src, bytes, hipMemcpyDefault));
            return SAS_OK;
        };
        rc = stage(s_means, means, sizeof(float) * 3 * n);
        if (!rc && quat_mode) rc = stage(s_q, quats, sizeof(float) * 4 * n);
        if (!rc && quat_mode) rc = stage(s_s, scales, sizeof(float) * 3 * n);
        if (!rc && !quat_mode) rc = stage(s_cov, cov6, sizeof(float) * 6 * n);
        if (!rc) rc = stage(s_op, opacities, sizeof(float) * n);
        if (!rc) rc = stage(s_col, colors, sizeof(float) * (size_t)coeff_floats * n);
        if (!rc && group_id) rc = stage(s_gid, group_id, (size_t)n);
        if (!rc && c->order_on_device) {
            // storage order from the staged means / group ids, where they are; only the record of the group ids' check comes back
            SasOrderRecord rec{};
            rc = device_order(c, n, (const float *)s_means.p, group_id ? (const uint8_t *)s_gid.p : nullptr, (int *)pl.perm.p, nullptr, n_groups);
            if (!rc && group_id) {
                hipError_t e = hipStreamSynchronize(nullptr);
                if (e != hipSuccess) rc = fail(c, SAS_ERR_HIP, "storage order: %s", hipGetErrorString(e));
                if (!rc) rc = order_record(c, rec);
                if (!rc && rec.bad_index >= 0) rc = fail(c, SAS_ERR_INVALID, "group_id[%lld]=%d >= n_groups=%d", (long long)rec.bad_index, rec.bad_id, n_groups);
            }
        }
        if (!rc) {
            sas_launch_relayout(nullptr, n, pl.n_pad, (const int *)pl.perm.p, (const float *)s_means.p,
                                (const float *)s_q.p, (const float *)s_s.p, (const float *)s_cov.p,
                                (const float *)s_op.p, (const float *)s_col.p, coeff_floats, planes,
                                (const uint8_t *)s_gid.p, (float4 *)pl.g0.p, (float4 *)pl.g1.p, (float4 *)pl.g2.p,
                                (float4 *)pl.col.p, (uint8_t *)pl.gid8.p);
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) rc = fail(c, SAS_ERR_HIP, "relayout: %s", hipGetErrorString(e));
        }
        if (rc) return rc;
    }

    c->scene = SasScene{};
    pl.bind(c->scene);
    c->scene.sh_degree = deg;
    c->scene.cov_mode = quat_mode ? 0 : 1;
    c->scene.n_groups = group_id ? n_groups : 0;
    scene_changed(c, Changed::Everything);
    if (group_id) {   // poses start as identity
        c->group_host.assign((size_t)12 * n_groups, 0.0f);
        for (int g = 0; g < n_groups; ++g) c->group_host[12 * g + 0] = c->group_host[12 * g + 5] = c->group_host[12 * g + 10] = 1.0f;
    }
    c->have |= HAVE_SCENE;
    return SAS_OK;
}

int sas_set_group_poses(sas_ctx *c, int n_groups, const float *Rt)
{
    if (!c || !Rt) return SAS_ERR_INVALID;
    if (!has(c, HAVE_SCENE)) return fail(c, SAS_ERR_NO_SCENE, "no scene uploaded");
    if (n_groups != c->scene.n_groups) return fail(c, SAS_ERR_INVALID, "scene has %d groups, got %d", c->scene.n_groups, n_groups);
    // Every frame carries a snapshot of the poses it was submitted with (its slot's block, uploaded in front of its
    // projection; kept for the case that it has to be rendered again), so frames in flight are not disturbed and
    // nothing is drained here: the new poses apply to the frames submitted from now on.
    c->group_host.assign(Rt, Rt + (size_t)12 * n_groups);
    return SAS_OK;
}

// ---- per-link pose algebra (rows a8 of SURVEY.md 8a; reference: splat_handler.py:239-288) -----------------------
// float64, the same expressions in the same order as sim_a_splat_amd/poses.py (quats_wxyz_to_matrices,
// link_splat_poses, matrices_to_quats_wxyz) and SplatScene._sync (quaternion -> matrix -> float32): the handle of a
// splat group stores a quaternion in the reference (handle.wxyz = ...), so the rotation goes matrix -> quaternion ->
// matrix here as well.  Built with -ffp-contract=off like everything else: no fused multiply-adds.
namespace {

void quat_to_matrix(const double *qin, double *R)
{
    const double n = std::sqrt(qin[0] * qin[0] + qin[1] * qin[1] + qin[2] * qin[2] + qin[3] * qin[3]);
    const double q[4] = {qin[0] / n, qin[1] / n, qin[2] / n, qin[3] / n};
    double qq[4][4];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) qq[a][b] = q[a] * q[b];
    R[0] = 1 - 2 * (qq[2][2] + qq[3][3]); R[1] = 2 * (qq[1][2] - qq[0][3]); R[2] = 2 * (qq[1][3] + qq[0][2]);
    R[3] = 2 * (qq[1][2] + qq[0][3]); R[4] = 1 - 2 * (qq[1][1] + qq[3][3]); R[5] = 2 * (qq[2][3] - qq[0][1]);
    R[6] = 2 * (qq[1][3] - qq[0][2]); R[7] = 2 * (qq[2][3] + qq[0][1]); R[8] = 1 - 2 * (qq[1][1] + qq[2][2]);
}

void matrix_to_quat(const double *R, double *q)
{
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        const double s = std::sqrt(tr + 1.0) * 2;
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double s = std::sqrt(1.0 + R[4 * i] - R[4 * j] - R[4 * k]) * 2;
        q[0] = (R[3 * k + j] - R[3 * j + k]) / s;
        q[1 + i] = 0.25 * s;
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) / s;
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) / s;
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int a = 0; a < 4; ++a) q[a] /= n;
}

// C = A B (3x3, row-major); tb: B transposed.  Sums left to right, as a plain triple loop does.
void mul33(const double *A, const double *B, bool tb, double *C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += A[3 * r + k] * (tb ? B[3 * c + k] : B[3 * k + c]);
            C[3 * r + c] = acc;
        }
}

}  // namespace

int sas_set_link_constants(sas_ctx *c, int n_links, double scale, const double *Ri, const double *ti, const double *Rfk,
                           const double *tfk, const double *weld, const int *group)
{
    if (!c) return SAS_ERR_INVALID;
    if (!has(c, HAVE_SCENE)) return fail(c, SAS_ERR_NO_SCENE, "no scene uploaded");
    if (n_links < 0 || n_links > c->scene.n_groups) return fail(c, SAS_ERR_INVALID, "n_links %d out of [0, %d groups]", n_links, c->scene.n_groups);
    if (n_links > 0 && (!Ri || !ti || !Rfk || !tfk)) return fail(c, SAS_ERR_INVALID, "Ri, ti, Rfk, tfk are required");
    LinkConsts L;
    L.n = n_links;
    L.scale = scale;
    if (n_links > 0) {
        memcpy(L.Ri, Ri, sizeof(L.Ri));
        memcpy(L.ti, ti, sizeof(L.ti));
        if (weld) memcpy(L.weld, weld, sizeof(L.weld));
        L.Rfk.assign(Rfk, Rfk + 9 * (size_t)n_links);
        L.tfk.assign(tfk, tfk + 3 * (size_t)n_links);
        L.group.resize((size_t)n_links);
        for (int k = 0; k < n_links; ++k) {
            const int g = group ? group[k] : k;
            if (g < 0 || g >= c->scene.n_groups) return fail(c, SAS_ERR_INVALID, "group[%d]=%d out of [0,%d)", k, g, c->scene.n_groups);
            L.group[(size_t)k] = g;
        }
    }
    c->links = L;
    return SAS_OK;
}

// ---- pure host functions (no context, no GPU): the float64 pose / camera algebra, testable on any machine ----------
int sas_link_group_poses(int k_links, double scale, const double *Ri, const double *ti, const double *Rfk, const double *tfk,
                         const double *weld, const double *q_msg, const double *p_msg, float *Rt_out)
{
    if (k_links < 0 || (k_links > 0 && (!Ri || !ti || !Rfk || !tfk || !q_msg || !p_msg || !Rt_out))) return SAS_ERR_INVALID;
    const double w0[3] = {0, 0, 0};
    const double *wd = weld ? weld : w0;
    for (int k = 0; k < k_links; ++k) {
        double Rm[9], RmF[9], T1[9], R[9], q[4], Rq[9];
        quat_to_matrix(q_msg + 4 * k, Rm);
        const double tm[3] = {p_msg[3 * k] + wd[0], p_msg[3 * k + 1] + wd[1], p_msg[3 * k + 2] + wd[2]};
        mul33(Rm, Rfk + 9 * (size_t)k, true, RmF);    // Rm Rfk^T
        mul33(Ri, RmF, false, T1);
        mul33(T1, Ri, true, R);                        // R = Ri Rm Rfk^T Ri^T
        // t = ti - R ti + s (tm - RmF tfk) Ri^T
        double u[3], t[3];
        for (int r = 0; r < 3; ++r) {
            double acc = 0.0;
            for (int j = 0; j < 3; ++j) acc += RmF[3 * r + j] * tfk[3 * (size_t)k + j];
            u[r] = scale * (tm[r] - acc);
        }
        for (int r = 0; r < 3; ++r) {
            double rti = 0.0, uri = 0.0;
            for (int j = 0; j < 3; ++j) rti += R[3 * r + j] * ti[j];
            for (int j = 0; j < 3; ++j) uri += u[j] * Ri[3 * r + j];
            t[r] = (ti[r] - rti) + uri;
        }
        matrix_to_quat(R, q);        // what the handle stores ...
        quat_to_matrix(q, Rq);       // ... and what the scene uploads
        float *dst = Rt_out + 12 * (size_t)k;
        for (int r = 0; r < 3; ++r) {
            for (int j = 0; j < 3; ++j) dst[4 * r + j] = (float)Rq[3 * r + j];
            dst[4 * r + 3] = (float)t[r];
        }
    }
    return SAS_OK;
}

int sas_attached_frame(double scale, const double *Ri, const double *ti, const double *q_link, const double *p_link,
                       const double *local_xyz, double *wxyz_out, double *xyz_out)
{
    if (!Ri || !ti || !q_link || !p_link || !local_xyz || !wxyz_out || !xyz_out) return SAS_ERR_INVALID;
    double Rl[9], R[9];
    quat_to_matrix(q_link, Rl);
    mul33(Ri, Rl, false, R);
    const double p[3] = {(p_link[0] + local_xyz[0]) * scale, (p_link[1] + local_xyz[1]) * scale, (p_link[2] + local_xyz[2]) * scale};
    for (int r = 0; r < 3; ++r) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += Ri[3 * r + j] * p[j];
        xyz_out[r] = acc + ti[r];
    }
    matrix_to_quat(R, wxyz_out);
    return SAS_OK;
}

int sas_camera_matrices(int n, const double *wxyz, const double *position, double fov, int width, int height, float *viewmats,
                        float *Ks)
{
    if (n < 0 || (n > 0 && (!wxyz || !position || !viewmats || !Ks))) return SAS_ERR_INVALID;
    const double f = 0.5 * height / std::tan(0.5 * fov);      // vertical FOV, square pixels
    for (int c = 0; c < n; ++c) {
        double R[9];
        quat_to_matrix(wxyz + 4 * c, R);                        // camera-to-world, OpenCV axes
        float *V = viewmats + 16 * (size_t)c;
        for (int r = 0; r < 3; ++r) {
            double acc = 0.0;
            for (int j = 0; j < 3; ++j) {
                V[4 * r + j] = (float)R[3 * j + r];             // R^T
                acc += R[3 * j + r] * position[3 * c + j];
            }
            V[4 * r + 3] = (float)(-acc);
        }
        V[12] = V[13] = V[14] = 0.0f;
        V[15] = 1.0f;
        float *K = Ks + 9 * (size_t)c;
        K[0] = (float)f; K[1] = 0.0f; K[2] = (float)(0.5 * width);
        K[3] = 0.0f; K[4] = (float)f; K[5] = (float)(0.5 * height);
        K[6] = 0.0f; K[7] = 0.0f; K[8] = 1.0f;
    }
    return SAS_OK;
}

int sas_set_link_poses(sas_ctx *c, int k_links, const double *q_msg, const double *p_msg, float *Rt_out)
{
    if (!c) return SAS_ERR_INVALID;
    if (!has(c, HAVE_SCENE)) return fail(c, SAS_ERR_NO_SCENE, "no scene uploaded");
    const LinkConsts &L = c->links;
    if (k_links < 0 || k_links > L.n) return fail(c, SAS_ERR_INVALID, "%d link poses, constants for %d (sas_set_link_constants)", k_links, L.n);
    if (k_links > 0 && (!q_msg || !p_msg)) return fail(c, SAS_ERR_INVALID, "q_msg and p_msg are required");
    float rows[12 * 256];
    if (k_links > 0)
        sas_link_group_poses(k_links, L.scale, L.Ri, L.ti, L.Rfk.data(), L.tfk.data(), L.weld, q_msg, p_msg, rows);
    for (int k = 0; k < k_links; ++k) memcpy(&c->group_host[12 * (size_t)L.group[(size_t)k]], rows + 12 * k, sizeof(float) * 12);
    if (Rt_out && !c->group_host.empty()) memcpy(Rt_out, c->group_host.data(), sizeof(float) * c->group_host.size());
    return SAS_OK;
}

int sas_link_attached_frame(sas_ctx *c, const double *q_link, const double *p_link, const double *local_xyz, double *wxyz_out,
                            double *xyz_out)
{
    if (!c) return SAS_ERR_INVALID;
    if (c->links.n <= 0) return fail(c, SAS_ERR_INVALID, "sas_set_link_constants first (the ICP similarity)");
    const int rc = sas_attached_frame(c->links.scale, c->links.Ri, c->links.ti, q_link, p_link, local_xyz, wxyz_out, xyz_out);
    return rc ? fail(c, rc, "sas_link_attached_frame: null argument") : SAS_OK;
}

int sas_get_group_poses(sas_ctx *c, int n_groups, float *Rt)
{
    if (!c || !Rt) return SAS_ERR_INVALID;
    if (!has(c, HAVE_SCENE)) return fail(c, SAS_ERR_NO_SCENE, "no scene uploaded");
    if (n_groups != c->scene.n_groups) return fail(c, SAS_ERR_INVALID, "scene has %d groups, got %d", c->scene.n_groups, n_groups);
    if (n_groups > 0) memcpy(Rt, c->group_host.data(), sizeof(float) * 12 * (size_t)n_groups);
    return SAS_OK;
}

struct ViewCall {
    const float *viewmat, *K;
    ViewOut out;
    const float *poses = nullptr;   // [n_groups,12] group poses of THIS view (a pose set), or nullptr: the context's current poses
    const float *fbg = nullptr;     // sas_render_features: feature background [feat_c] of out.features (nullptr: 0)
    int feat_c = 0;
    float min_alpha = 0.0f;         // sas_render_batch_labels: of out.labels
};

static int check_view(sas_ctx *c, const ViewCall &v, int width, int height)
{
    if (!has(c, HAVE_SCENE)) return fail(c, SAS_ERR_NO_SCENE, "sas_render before sas_scene_upload");
    if (!v.viewmat || !v.K) return fail(c, SAS_ERR_INVALID, "viewmat and K are required");
    if (width <= 0 || height <= 0 || width > 65535 * SAS_TILE || height > 65535 * SAS_TILE)
        return fail(c, SAS_ERR_INVALID, "bad image size %dx%d", width, height);
    if (!(v.K[0] > 0.0f) || !(v.K[4] > 0.0f)) return fail(c, SAS_ERR_INVALID, "focal lengths must be positive");
    if ((v.out.points || v.out.mask) && !v.out.depth) return fail(c, SAS_ERR_INVALID, "points / mask need the depth output");
    return SAS_OK;
}

static void fill_args(RenderArgs &a, const ViewCall &v, int width, int height, const float *background, unsigned flags,
                      const float *max_depth, hipStream_t st, bool solo)
{
    const ViewOut &o = v.out;
    a.solo = solo;
    // rgb8 beside rgb8_host is the context's own staging frame (sas_render_batch_host): nothing of the caller's on the device
    a.order_caller = o.rgb || o.alpha || o.depth || o.points || o.mask || o.features || o.labels || o.reader != ViewOut::NO_READER || (o.rgb8 && !o.rgb8_host);
    memcpy(a.viewmat, v.viewmat, sizeof(a.viewmat));
    memcpy(a.K, v.K, sizeof(a.K));
    for (int k = 0; k < 3; ++k) a.bg[k] = background ? background[k] : 0.0f;
    a.W = width; a.H = height; a.flags = flags;
    a.out = o;
    a.feat_c = o.features ? v.feat_c : 0;
    for (int k = 0; k < a.feat_c; ++k) a.fbg[k] = v.fbg ? v.fbg[k] : 0.0f;
    a.min_alpha = v.min_alpha;
    a.use_max_depth = max_depth != nullptr;
    a.max_depth = max_depth ? *max_depth : 0.0f;
    a.stream = st;
}

// the poses the slot's frame is rendered with: the view's own set, else the context's current ones
static void snapshot_poses(sas_ctx *c, Slot &sl, const ViewCall &v)
{
    if (c->scene.n_groups <= 0) return;
    memcpy(sl.poses_host, v.poses ? v.poses : c->group_host.data(), sizeof(float) * 12 * (size_t)c->scene.n_groups);
}

// One view (n == 1), a pair of views that share one projection pass (n == 2), or -- `grouped` -- up to
// SAS_MAX_GROUP views that share every launch.
static int render_views(sas_ctx *c, const ViewCall *views, int n, int width, int height, const float *background,
                        unsigned flags, const float *max_depth, void *stream, bool grouped = false, bool solo = false)
{
    if (!c) return SAS_ERR_INVALID;
    flags = frame_flags(c, flags);
    for (int k = 0; k < n; ++k)
        if (const int rc = check_view(c, views[k], width, height)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (c->inflight > 0 && (st != c->stream || (flags & SAS_TIMING)))
        if (const int rc = complete_all(c)) return rc;   // one caller stream at a time; timed frames run alone
    while (c->inflight > c->n_slots - n)
        if (const int rc = complete_oldest(c)) return rc;
    c->stream = st;
    if (c->ring_restart && c->inflight == 0) c->head = 0;
    Slot *sl[SAS_MAX_GROUP] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < n; ++k) {
        sl[k] = &c->slots[(c->head + c->inflight + k) % c->n_slots];
        fill_args(sl[k]->args, views[k], width, height, background, flags, max_depth, st, solo && n == 1 && c->inflight == 0);
        snapshot_poses(c, *sl[k], views[k]);
    }
    const int rc = enqueue_launch(c, sl, n, n == 2 && !grouped);
    if (rc) { mark_dirty(c); return rc; }
    c->inflight += n;
    c->frames_submitted += n;
    c->last_slot = (int)(sl[n - 1] - c->slots);
    if (flags & SAS_ASYNC) return SAS_OK;
    return complete_all(c);
}

int sas_render(sas_ctx *c, const float *viewmat, const float *K, int width, int height, const float *background,
               unsigned flags, float *rgb, float *alpha, float *depth, uint8_t *rgb8, void *stream)
{
    const ViewCall v = {viewmat, K, {rgb, alpha, depth, rgb8}};
    return render_views(c, &v, 1, width, height, background, flags, nullptr, stream, false, !(flags & SAS_ASYNC));
}

int sas_scene_features(sas_ctx *c, int64_t n, int channels, const float *features)
{
    if (const int rc = need_scene(c, "sas_scene_features")) return rc;
    forget(c, HAVE_MESH_FEAT);   // the triangles' rows belong to the store they were set beside
    if (n != c->scene.n) return fail(c, SAS_ERR_INVALID, "features for %lld Gaussians, the scene has %lld", (long long)n, (long long)c->scene.n);
    if (channels < 1 || channels > SAS_MAX_FEATURES) return fail(c, SAS_ERR_INVALID, "channels %d out of [1,%d]", channels, SAS_MAX_FEATURES);
    if (!features && c->scene.n_groups <= 0) return fail(c, SAS_ERR_INVALID, "one-hot group features need a scene with splat groups");
    if (!features && channels != c->scene.n_groups)
        return fail(c, SAS_ERR_INVALID, "one-hot group features have n_groups=%d channels, got %d", c->scene.n_groups, channels);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // frames in flight read the store
    forget(c, HAVE_FEAT);
    const int64_t n_pad = c->scene.n_pad;
    const int rc = fill_feature_store(c, c->feat, (size_t)(n_pad > 0 ? n_pad : 64), channels, features, (size_t)n, "feature store",
                                      [&](hipStream_t st, const float *src, float *store) {
                                          sas_launch_feature_store(st, n, n_pad, c->scene.perm, c->scene.gid8, src, channels, store);
                                      });
    if (rc) return rc;
    c->feat_c = channels;
    c->feat_onehot = features == nullptr;
    c->have |= HAVE_FEAT;
    return SAS_OK;
}

int sas_render_features(sas_ctx *c, const float *viewmat, const float *K, int width, int height, const float *background,
                        const float *feature_background, unsigned flags, float *rgb, float *alpha, float *depth, float *features,
                        void *stream)
{
    if (const int rc = need_scene(c, "sas_render_features")) return rc;
    if (!has(c, HAVE_FEAT)) return fail(c, SAS_ERR_INVALID, "no features set for this scene (sas_scene_features)");
    if (has(c, HAVE_MESH) && !has(c, HAVE_MESH_FEAT))
        return fail(c, SAS_ERR_INVALID, "feature frames of a context with meshes are not supported (sas_scene_meshes) until the meshes "
                                        "have features (sas_scene_mesh_features)");
    if (!features) return fail(c, SAS_ERR_INVALID, "the features output is required");
    ViewCall v = {viewmat, K, {rgb, alpha, depth}};
    v.out.features = features;
    v.fbg = feature_background;
    v.feat_c = c->feat_c;
    return render_views(c, &v, 1, width, height, background, flags | SAS_FULL_SORT, nullptr, stream, false, !(flags & SAS_ASYNC));
}

int sas_scene_mesh_features(sas_ctx *c, int64_t n_triangles, int channels, const float *features)
{
    if (const int rc = need_scene(c, "sas_scene_mesh_features")) return rc;
    if (!has(c, HAVE_MESH)) return fail(c, SAS_ERR_INVALID, "no meshes set for this scene (sas_scene_meshes)");
    if (!has(c, HAVE_FEAT)) return fail(c, SAS_ERR_INVALID, "no features set for this scene (sas_scene_features)");
    if (n_triangles != c->mesh.nt)
        return fail(c, SAS_ERR_INVALID, "features for %lld triangles, the meshes have %d", (long long)n_triangles, c->mesh.nt);
    if (channels != c->feat_c) return fail(c, SAS_ERR_INVALID, "%d channels, the feature store has %d", channels, c->feat_c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // frames in flight read the rows
    const size_t nt = (size_t)n_triangles;
    if (!features) {   // one-hot of the triangles' pose groups: every group needs a channel
        std::vector<int4> t4(nt);
        HIP_TRY(c, hipMemcpy(t4.data(), c->mesh_tri.p, sizeof(int4) * nt, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < nt; ++t)
            if (t4[t].w >= channels) return fail(c, SAS_ERR_INVALID, "one-hot: triangle %zu is of group %d >= %d channels", t, t4[t].w, channels);
    }
    forget(c, HAVE_MESH_FEAT);
    const int rc = fill_feature_store(c, c->mesh_feat, nt, channels, features, nt, "mesh feature store",
                                      [&](hipStream_t st, const float *src, float *store) {
                                          sas_launch_mesh_feature_store(st, n_triangles, c->mesh.tri, src, channels, store);
                                      });
    if (rc) return rc;
    c->mesh_feat_onehot = features == nullptr;
    c->have |= HAVE_MESH_FEAT;
    return SAS_OK;
}

int sas_scene_meshes(sas_ctx *c, int64_t n_vertices, const float *vertices, int64_t n_triangles, const int32_t *triangles,
                     const float *colors, const uint8_t *group, float ambient, float diffuse)
{
    if (const int rc = need_scene(c, "sas_scene_meshes")) return rc;
    forget(c, HAVE_MESH_FEAT | HAVE_MESH_ATTR);   // every call forgets the triangles' feature rows (sas_scene_mesh_features) and the vertex attributes
    if (n_triangles < 0 || n_vertices < 0 || n_triangles > (1 << 29) || n_vertices > 0x7fffffffll)
        return fail(c, SAS_ERR_INVALID, "bad mesh sizes: %lld vertices, %lld triangles", (long long)n_vertices, (long long)n_triangles);
    if (!std::isfinite(ambient) || !std::isfinite(diffuse)) return fail(c, SAS_ERR_INVALID, "ambient and diffuse must be finite");
    if (n_triangles > 0 && (!vertices || !triangles || !colors || !group)) return fail(c, SAS_ERR_INVALID, "vertices, triangles, colors and group are required");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // frames in flight read the meshes
    if (n_triangles == 0) {
        forget(c, HAVE_MESH);
        return SAS_OK;
    }
    const size_t nv = (size_t)n_vertices, nt = (size_t)n_triangles;
    std::vector<float> v(3 * nv), col(3 * nt);
    std::vector<int32_t> tri(3 * nt);
    std::vector<uint8_t> g(nt);
    if (nv) HIP_TRY(c, hipMemcpy(v.data(), vertices, sizeof(float) * 3 * nv, hipMemcpyDefault));
    HIP_TRY(c, hipMemcpy(tri.data(), triangles, sizeof(int32_t) * 3 * nt, hipMemcpyDefault));
    HIP_TRY(c, hipMemcpy(col.data(), colors, sizeof(float) * 3 * nt, hipMemcpyDefault));
    HIP_TRY(c, hipMemcpy(g.data(), group, nt, hipMemcpyDefault));
    const int ng = std::max(1, c->scene.n_groups);
    std::vector<float4> v4(nv), c4(nt);
    std::vector<int4> t4(nt);
    for (size_t i = 0; i < nv; ++i) v4[i] = make_float4(v[3 * i], v[3 * i + 1], v[3 * i + 2], 0.0f);
    for (size_t t = 0; t < nt; ++t) {
        for (int k = 0; k < 3; ++k)
            if (tri[3 * t + k] < 0 || (int64_t)tri[3 * t + k] >= n_vertices)
                return fail(c, SAS_ERR_INVALID, "triangles[%zu][%d]=%d out of [0,%lld)", t, k, tri[3 * t + k], (long long)n_vertices);
        if (g[t] >= ng) return fail(c, SAS_ERR_INVALID, "group[%zu]=%d >= %d pose groups", t, (int)g[t], ng);
        t4[t] = make_int4(tri[3 * t], tri[3 * t + 1], tri[3 * t + 2], (int)g[t]);
        c4[t] = make_float4(col[3 * t], col[3 * t + 1], col[3 * t + 2], 0.0f);
    }
    // validated: only now are the previous meshes replaced (a rejected call leaves them in place; a failed device copy
    // below leaves none)
    forget(c, HAVE_MESH);
    if (const int rc = ensure(c, {{c->mesh_vert, sizeof(float4) * std::max<size_t>(nv, 1)}, {c->mesh_tri, sizeof(int4) * nt}, {c->mesh_col, sizeof(float4) * nt}}))
        return rc;
    if (nv) HIP_TRY(c, hipMemcpy(c->mesh_vert.p, v4.data(), sizeof(float4) * nv, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->mesh_tri.p, t4.data(), sizeof(int4) * nt, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->mesh_col.p, c4.data(), sizeof(float4) * nt, hipMemcpyHostToDevice));
    c->mesh = SasMeshScene{};
    c->mesh.vert = (const float4 *)c->mesh_vert.p;
    c->mesh.tri = (const int4 *)c->mesh_tri.p;
    c->mesh.color = (const float4 *)c->mesh_col.p;
    c->mesh.nv = (int)n_vertices;
    c->mesh.nt = (int)n_triangles;
    c->mesh.n_groups = c->scene.n_groups;
    c->mesh.ka = ambient;
    c->mesh.kd = diffuse;
    for (Slot &sl : c->slots) sl.msc.cap = 0;   // re-derive the list capacity for the new meshes
    c->have |= HAVE_MESH;
    return SAS_OK;
}

int sas_scene_mesh_vertex_attributes(sas_ctx *c, int64_t n_vertices, const float *normals, const float *colors)
{
    if (const int rc = need_scene(c, "sas_scene_mesh_vertex_attributes")) return rc;
    if (!has(c, HAVE_MESH)) return fail(c, SAS_ERR_INVALID, "no meshes set for this scene (sas_scene_meshes)");
    if (n_vertices != c->mesh.nv)
        return fail(c, SAS_ERR_INVALID, "attributes for %lld vertices, the meshes have %d", (long long)n_vertices, c->mesh.nv);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // frames in flight read the attributes
    if (!normals && !colors) {   // cleared: the device copies and the slots' planes go back (flat frames keep their footprint)
        forget(c, HAVE_MESH_ATTR);
        int rc;
        if ((rc = c->mesh_nrm.release(c)) || (rc = c->mesh_vcol.release(c))) return rc;
        for (Slot &sl : c->slots)
            if ((rc = sl.msc.planes.release(c))) return rc;
        return SAS_OK;
    }
    const size_t nv = (size_t)n_vertices;
    std::vector<float> in(3 * nv);
    std::vector<float4> n4(nv, make_float4(0.0f, 0.0f, 0.0f, 0.0f)), c4(nv);
    if (normals) {
        if (nv) HIP_TRY(c, hipMemcpy(in.data(), normals, sizeof(float) * 3 * nv, hipMemcpyDefault));
        for (size_t i = 0; i < nv; ++i) {   // a non-finite normal counts as none
            const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
            if (std::isfinite(x) && std::isfinite(y) && std::isfinite(z)) n4[i] = make_float4(x, y, z, 0.0f);
        }
    }
    if (colors) {
        if (nv) HIP_TRY(c, hipMemcpy(in.data(), colors, sizeof(float) * 3 * nv, hipMemcpyDefault));
        for (size_t i = 0; i < nv; ++i) c4[i] = make_float4(in[3 * i], in[3 * i + 1], in[3 * i + 2], 0.0f);
    }
    forget(c, HAVE_MESH_ATTR);   // (a failed copy below leaves none)
    int rc;
    if ((rc = ensure(c, c->mesh_nrm, sizeof(float4) * std::max<size_t>(nv, 1)))) return rc;
    if (nv) HIP_TRY(c, hipMemcpy(c->mesh_nrm.p, n4.data(), sizeof(float4) * nv, hipMemcpyHostToDevice));
    if (colors) {
        if ((rc = ensure(c, c->mesh_vcol, sizeof(float4) * std::max<size_t>(nv, 1)))) return rc;
        if (nv) HIP_TRY(c, hipMemcpy(c->mesh_vcol.p, c4.data(), sizeof(float4) * nv, hipMemcpyHostToDevice));
    }
    c->mesh_has_vcol = colors != nullptr;
    c->have |= HAVE_MESH_ATTR;
    return SAS_OK;
}

// ---- what the calls that need no scene share: sas_query_meshes, sas_match_points, sas_sample_points, sas_fuse_depth ----------------------

static int check_max_distance(sas_ctx *c, float max_distance)
{
    if (!(max_distance >= 0.0f)) return fail(c, SAS_ERR_INVALID, "max_distance must be >= 0 (INFINITY allowed), got %g", (double)max_distance);
    return SAS_OK;
}

// rows: a row-major 3x4 block A|t, or nullptr: the identity
static SasAffine pack_affine(const float *rows)
{
    SasAffine m;
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) m.A[3 * k + j] = rows ? rows[4 * k + j] : (k == j ? 1.0f : 0.0f);
        m.t[k] = rows ? rows[4 * k + 3] : 0.0f;
    }
    return m;
}

static SasDepthView pack_depth_view(const float *K, const float *rows) { return SasDepthView{K[0], K[4], K[2], K[5], pack_affine(rows)}; }

// What a call that takes depth views checks of them: C views of W x H pixels, `depth`, Ks [C,9], transform [C,12] or nullptr, flags.
// sized_without_views: W and H must be positive, and a view within the pixel limit, even when C is 0 (sas_fuse_depth; sas_sample_points
// accepts any size with no view).  C itself is the caller's to check, first.
static int check_depth_views(sas_ctx *c, const char *who, int C, int W, int H, const float *depth, const float *Ks, const float *transform,
                             unsigned flags, bool sized_without_views)
{
    if (flags & ~SAS_TIMING) return fail(c, SAS_ERR_INVALID, "%s: flags 0x%x not accepted (SAS_TIMING; blocking only)", who, flags);
    if (C > 0 || sized_without_views) {
        if (W <= 0 || H <= 0) return fail(c, SAS_ERR_INVALID, "%s: bad image size %dx%d", who, W, H);
        const long long px_max = 0x7fffffffll - 256, px_view = (long long)H * W;   // (no product beyond 2^62)
        if (px_view > px_max || (long long)C * px_view > px_max)
            return fail(c, SAS_ERR_INVALID, "%s: %d views of %dx%d are more than 2^31 - 256 pixels", who, C, W, H);
    }
    if (C > 0 && (!depth || !Ks)) return fail(c, SAS_ERR_INVALID, "%s: depth and Ks are required", who);
    for (int v = 0; v < C; ++v) {
        const float *Kv = Ks + 9 * (size_t)v, *Tv = transform ? transform + 12 * (size_t)v : nullptr;
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(Kv[k])) return fail(c, SAS_ERR_INVALID, "%s: Ks[%d][%d] = %g is not finite", who, v, k, (double)Kv[k]);
        if (!(Kv[0] > 0.0f) || !(Kv[4] > 0.0f)) return fail(c, SAS_ERR_INVALID, "%s: view %d: fx = %g, fy = %g must be > 0", who, v, (double)Kv[0], (double)Kv[4]);
        for (int k = 0; Tv && k < 12; ++k)
            if (!std::isfinite(Tv[k])) return fail(c, SAS_ERR_INVALID, "%s: transform[%d][%d] = %g is not finite", who, v, k, (double)Tv[k]);
    }
    return SAS_OK;
}

int sas_query_meshes(sas_ctx *c, int64_t n_points, const float *points, int64_t n_vertices, const float *vertices, int64_t n_triangles,
                     const int32_t *triangles, int n_meshes, const int64_t *mesh_offsets, float max_distance, float *distance,
                     float *winding, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    if (n_points < 0 || n_points > 0x7fffff00ll || n_vertices < 0 || n_vertices > 0x7fffffffll || n_triangles < 0 || n_triangles > (1 << 29))
        return fail(c, SAS_ERR_INVALID, "bad query sizes: %lld points, %lld vertices, %lld triangles", (long long)n_points,
                    (long long)n_vertices, (long long)n_triangles);
    if (n_meshes < 1 || n_meshes > 256) return fail(c, SAS_ERR_INVALID, "n_meshes %d out of [1,256]", n_meshes);
    if (const int rc = check_max_distance(c, max_distance)) return rc;
    if (!distance && !winding) return fail(c, SAS_ERR_INVALID, "distance and winding are both NULL");
    if (!mesh_offsets || (n_points > 0 && !points) || (n_triangles > 0 && (!vertices || !triangles)))
        return fail(c, SAS_ERR_INVALID, "points, vertices, triangles and mesh_offsets are required");
    if (mesh_offsets[0] != 0 || mesh_offsets[n_meshes] != n_triangles)
        return fail(c, SAS_ERR_INVALID, "mesh_offsets must run from 0 to n_triangles=%lld, got %lld .. %lld", (long long)n_triangles,
                    (long long)mesh_offsets[0], (long long)mesh_offsets[n_meshes]);
    for (int m = 0; m < n_meshes; ++m)
        if (mesh_offsets[m + 1] < mesh_offsets[m])
            return fail(c, SAS_ERR_INVALID, "mesh_offsets decrease at mesh %d: %lld > %lld", m, (long long)mesh_offsets[m], (long long)mesh_offsets[m + 1]);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nv = (size_t)n_vertices, nt = (size_t)n_triangles, np = (size_t)n_points;
    std::vector<float> v(3 * nv);
    std::vector<int32_t> tri(3 * nt);
    if (nv && nt) HIP_TRY(c, hipMemcpy(v.data(), vertices, sizeof(float) * 3 * nv, hipMemcpyDefault));
    if (nt) HIP_TRY(c, hipMemcpy(tri.data(), triangles, sizeof(int32_t) * 3 * nt, hipMemcpyDefault));
    // the kept triangles (three finite vertices) as records, mesh by mesh, and each mesh's box over their vertices
    std::vector<float4> rec;
    rec.reserve(3 * nt);
    std::vector<SasQueryMesh> table((size_t)n_meshes);
    for (int m = 0; m < n_meshes; ++m) {
        SasQueryMesh &q = table[(size_t)m];
        q.start = (int)(rec.size() / 3);
        for (int k = 0; k < 3; ++k) { q.lo[k] = INFINITY; q.hi[k] = -INFINITY; }
        for (size_t t = (size_t)mesh_offsets[m]; t < (size_t)mesh_offsets[m + 1]; ++t) {
            bool finite = true;
            for (int k = 0; k < 3; ++k) {
                const int32_t id = tri[3 * t + k];
                if (id < 0 || (int64_t)id >= n_vertices)
                    return fail(c, SAS_ERR_INVALID, "triangles[%zu][%d]=%d out of [0,%lld)", t, k, id, (long long)n_vertices);
                const float *p = &v[3 * (size_t)id];
                finite = finite && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
            }
            if (!finite) continue;
            for (int k = 0; k < 3; ++k) {
                const float *p = &v[3 * (size_t)tri[3 * t + k]];
                rec.push_back(make_float4(p[0], p[1], p[2], 0.0f));
                for (int a = 0; a < 3; ++a) { q.lo[a] = std::min(q.lo[a], p[a]); q.hi[a] = std::max(q.hi[a], p[a]); }
            }
        }
        q.count = (int)(rec.size() / 3) - q.start;
    }
    if (n_points == 0) return SAS_OK;
    if (const int rc = complete_all(c)) return rc;
    if (const int rc = ensure(c, {{c->query_pts, sizeof(float) * 3 * np},
                                  {c->query_tri, sizeof(float4) * std::max<size_t>(rec.size(), 1)},
                                  {c->query_mesh, sizeof(SasQueryMesh) * table.size()},
                                  {c->query_list, sizeof(int) * np * table.size()},
                                  {c->query_count, sizeof(int) * table.size()}}))
        return rc;
    HIP_TRY(c, hipMemcpy(c->query_pts.p, points, sizeof(float) * 3 * np, hipMemcpyDefault));
    if (!rec.empty()) HIP_TRY(c, hipMemcpy(c->query_tri.p, rec.data(), sizeof(float4) * rec.size(), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->query_mesh.p, table.data(), sizeof(SasQueryMesh) * table.size(), hipMemcpyHostToDevice));
    SasQuery q{};
    q.points = (const float *)c->query_pts.p;
    q.tri = (const float4 *)c->query_tri.p;
    q.mesh = (const SasQueryMesh *)c->query_mesh.p;
    q.list = (int *)c->query_list.p;
    q.count = (int *)c->query_count.p;
    q.distance = distance;
    q.winding = winding;
    q.n = n_points;
    q.n_tri = (long long)(rec.size() / 3);
    q.n_meshes = n_meshes;
    q.max_distance = max_distance;
    hipStream_t st = (hipStream_t)stream;
    sas_launch_query(st, q);
    return finish_launches(c, st, "mesh query");
}

// The slice count of a sas_match_points call: `asked`, or (0) as many as bring the grid of k_match_slice to four workgroups per compute
// unit; never more than the target has chunks (nor than a grid's y extent), at least one.
static int match_slices(long long n_blocks, long long n_chunks, int asked, int cus)
{
    long long s = asked > 0 ? asked : (4ll * cus + n_blocks - 1) / std::max(1ll, n_blocks);
    s = std::min(s, std::min(n_chunks, 65535ll));
    return (int)std::max(1ll, s);
}

int sas_match_points(sas_ctx *c, int64_t n_source, const float *source, int64_t n_target, const float *target, const float *transform,
                     float max_distance, int slices, int32_t *index, float *dist2, double *moments, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    if (n_source < 0 || n_source > 0x7fffff00ll || n_target < 0 || n_target > 0x7fffff00ll)
        return fail(c, SAS_ERR_INVALID, "bad match sizes: %lld source points, %lld target points", (long long)n_source, (long long)n_target);
    if ((n_source > 0 && !source) || (n_target > 0 && !target)) return fail(c, SAS_ERR_INVALID, "source and target are required");
    if (const int rc = check_max_distance(c, max_distance)) return rc;
    if (slices < 0) return fail(c, SAS_ERR_INVALID, "slices must be >= 0 (0: the library's choice), got %d", slices);
    if (!index && !dist2 && !moments) return fail(c, SAS_ERR_INVALID, "index, dist2 and moments are all NULL");
    for (int k = 0; transform && k < 12; ++k)
        if (!std::isfinite(transform[k])) return fail(c, SAS_ERR_INVALID, "transform[%d] = %g is not finite", k, (double)transform[k]);
    SasMatch m{};
    m.m = pack_affine(transform);
    if (moments) std::fill(moments, moments + SAS_MATCH_MOMENTS, 0.0);
    if (n_source == 0) return SAS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    if (c->match_cus <= 0) {
        HIP_TRY(c, hipDeviceGetAttribute(&c->match_cus, hipDeviceAttributeMultiprocessorCount, c->device));
        if (c->match_cus <= 0) c->match_cus = 1;
    }
    const size_t ns = (size_t)n_source, nt = (size_t)n_target;
    m.n_source = n_source;
    m.n_target = n_target;
    m.n_blocks = (n_source + 255) / 256;
    const long long n_chunks = (n_target + SAS_MATCH_CHUNK - 1) / SAS_MATCH_CHUNK;
    m.slices = match_slices(m.n_blocks, n_chunks, slices, c->match_cus);
    m.slice_targets = std::max(1ll, (n_chunks + m.slices - 1) / m.slices) * SAS_MATCH_CHUNK;
    m.slices = (int)std::max(1ll, (n_target + m.slice_targets - 1) / m.slice_targets);   // (no slice is empty)
    m.md2 = max_distance * max_distance;
    if (const int rc = ensure(c, {{c->match_src, sizeof(float) * 3 * ns},
                                  {c->match_tgt, sizeof(float) * 3 * std::max<size_t>(nt, 1)},
                                  {c->match_keys, sizeof(unsigned long long) * ns * (size_t)m.slices},
                                  {c->match_index, sizeof(int32_t) * ns},
                                  {c->match_dist2, sizeof(float) * ns},
                                  {c->match_partial, sizeof(double) * SAS_MATCH_MOMENTS * ((size_t)m.n_blocks + 1)}}))
        return rc;
    HIP_TRY(c, hipMemcpy(c->match_src.p, source, sizeof(float) * 3 * ns, hipMemcpyDefault));
    if (nt) HIP_TRY(c, hipMemcpy(c->match_tgt.p, target, sizeof(float) * 3 * nt, hipMemcpyDefault));
    m.source = (const float *)c->match_src.p;
    m.target = (const float *)c->match_tgt.p;
    m.keys = (unsigned long long *)c->match_keys.p;
    m.index = index ? (int *)c->match_index.p : nullptr;
    m.dist2 = dist2 ? (float *)c->match_dist2.p : nullptr;
    m.partial = moments ? (double *)c->match_partial.p : nullptr;                                        // rows [0, n_blocks)
    m.moments = moments ? (double *)c->match_partial.p + SAS_MATCH_MOMENTS * (size_t)m.n_blocks : nullptr;   // the row behind them
    hipStream_t st = (hipStream_t)stream;
    sas_launch_match(st, m);
    if (const int rc = finish_launches(c, st, "point matching")) return rc;
    if (index) HIP_TRY(c, hipMemcpy(index, c->match_index.p, sizeof(int32_t) * ns, hipMemcpyDefault));
    if (dist2) HIP_TRY(c, hipMemcpy(dist2, c->match_dist2.p, sizeof(float) * ns, hipMemcpyDefault));
    if (moments) HIP_TRY(c, hipMemcpy(moments, m.moments, sizeof(double) * SAS_MATCH_MOMENTS, hipMemcpyDeviceToHost));
    return SAS_OK;
}

int sas_sample_points(sas_ctx *c, int n_views, int width, int height, const float *depth, const uint8_t *rgb8, const uint8_t *labels,
                      const float *Ks, const float *transform, const int32_t *cloud, int n_clouds, const uint8_t *keep,
                      const float *bounds, float voxel, int stride, int n_points, unsigned flags, float *points, int32_t *index,
                      uint8_t *colors, uint8_t *labels_out, int32_t *count, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    const char *who = "sas_sample_points";
    const int C = n_views, E = n_clouds, K = n_points;
    if (C < 0 || C > 65535) return fail(c, SAS_ERR_INVALID, "%s: n_views %d out of [0,65535]", who, C);
    if (E < 1) return fail(c, SAS_ERR_INVALID, "%s: n_clouds %d, at least one is needed", who, E);
    if (K < 0) return fail(c, SAS_ERR_INVALID, "%s: n_points %d is negative", who, K);
    if (stride < 1) return fail(c, SAS_ERR_INVALID, "%s: stride %d, must be >= 1", who, stride);
    if ((long long)E * std::max(K, 1) > 0x7fffff00ll) return fail(c, SAS_ERR_INVALID, "%s: %d clouds of %d points are too many", who, E, K);
    if (const int rc = check_depth_views(c, who, C, width, height, depth, Ks, transform, flags, false)) return rc;
    if (K > 0 && !index) return fail(c, SAS_ERR_INVALID, "%s: the index output is required", who);
    if (colors && !rgb8) return fail(c, SAS_ERR_INVALID, "%s: colors without rgb8", who);
    if (labels_out && !labels) return fail(c, SAS_ERR_INVALID, "%s: labels_out without labels", who);
    if (!(voxel >= 0.0f) || !(voxel < INFINITY)) return fail(c, SAS_ERR_INVALID, "%s: voxel %g, must be finite and >= 0", who, (double)voxel);
    if (voxel > 0.0f && !bounds) return fail(c, SAS_ERR_INVALID, "%s: a voxel grid needs bounds", who);
    SasCloud q{};
    q.cells = 0;
    for (int k = 0; bounds && k < 3; ++k) {
        q.lo[k] = bounds[k];
        q.hi[k] = bounds[3 + k];
        if (!(q.lo[k] <= q.hi[k])) return fail(c, SAS_ERR_INVALID, "%s: bounds lo[%d] = %g, hi[%d] = %g", who, k, (double)q.lo[k], k, (double)q.hi[k]);
    }
    q.has_bounds = bounds != nullptr;
    q.voxel = voxel;
    if (voxel > 0.0f) {
        q.cells = 1;
        for (int k = 0; k < 3; ++k) {
            const float cells = ceilf((q.hi[k] - q.lo[k]) / voxel);   // float32, as the contract has it
            if (!(cells <= 16777216.0f)) return fail(c, SAS_ERR_INVALID, "%s: the voxel grid is too large along axis %d", who, k);
            q.n[k] = std::max(1, (int)cells);
            q.cells *= q.n[k];
            if (q.cells > (1ll << 24))
                return fail(c, SAS_ERR_INVALID, "%s: a voxel grid of more than 2^24 cells (%d x %d x ...)", who, q.n[0], q.n[1]);
        }
    }
    for (int v = 0; cloud && v < C; ++v)
        if (cloud[v] < 0 || cloud[v] >= E) return fail(c, SAS_ERR_INVALID, "%s: cloud[%d] = %d out of [0,%d)", who, v, cloud[v], E);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    q.C = C; q.E = E; q.W = width; q.H = height; q.stride = stride; q.K = K;
    q.Ws = C > 0 ? (width + stride - 1) / stride : 0;
    q.S = C > 0 ? (long long)q.Ws * ((height + stride - 1) / stride) : 0;
    q.n_rows = (long long)C * q.S;
    q.n_pix = (long long)C * height * width;
    q.bpv = (int)((q.S + 255) / 256);
    q.n_blocks = (long long)C * q.bpv;
    q.n_grid = (long long)E * q.cells;
    // the per-view rows, the clouds' first rows and the keep table: one host block, one copy
    const size_t off_base = sizeof(SasCloudView) * (size_t)C, off_keep = off_base + sizeof(long long) * (size_t)E;
    std::vector<unsigned char> par(off_keep + 256);
    SasCloudView *view = reinterpret_cast<SasCloudView *>(par.data());
    long long *base = reinterpret_cast<long long *>(par.data() + off_base);
    std::vector<long long> views_of(E, 0);
    for (int v = 0; v < C; ++v) ++views_of[cloud ? cloud[v] : 0];
    long long first = 0;
    for (int e = 0; e < E; ++e) { base[e] = first; first += views_of[e] * q.S; }
    for (int v = 0; v < C; ++v) {
        SasCloudView &V = view[v];
        V.cam = pack_depth_view(Ks + 9 * (size_t)v, transform ? transform + 12 * (size_t)v : nullptr);
        V.cloud = cloud ? cloud[v] : 0;
        V.pad = 0;
        V.base = base[V.cloud];
    }
    const bool use_keep = keep && labels;
    if (use_keep) std::copy(keep, keep + 256, par.data() + off_keep);
    const size_t rows = (size_t)std::max(q.n_rows, 1ll), blocks = (size_t)std::max(q.n_blocks, 1ll);
    if (const int rc = ensure(c, {{c->cloud_par, par.size()},
                                  {c->cloud_grid, sizeof(unsigned) * (size_t)std::max(q.n_grid, 1ll)},
                                  {c->cloud_cand, sizeof(float4) * rows},
                                  {c->cloud_blk, sizeof(unsigned) * 2 * blocks},
                                  {c->cloud_rows, sizeof(float4) * rows},
                                  {c->cloud_dist, sizeof(float) * rows},
                                  {c->cloud_count, sizeof(int) * (size_t)E}}))
        return rc;
    HIP_TRY(c, hipMemcpy(c->cloud_par.p, par.data(), par.size(), hipMemcpyHostToDevice));
    unsigned char *dpar = (unsigned char *)c->cloud_par.p;
    q.depth = depth; q.rgb8 = rgb8; q.labels = labels;
    q.view = reinterpret_cast<const SasCloudView *>(dpar);
    q.cloud_base = reinterpret_cast<const long long *>(dpar + off_base);
    q.keep = use_keep ? dpar + off_keep : nullptr;
    q.grid = (unsigned *)c->cloud_grid.p;
    q.cand = (float4 *)c->cloud_cand.p;
    q.blk_count = (unsigned *)c->cloud_blk.p;
    q.blk_off = q.blk_count + blocks;
    q.rows = (float4 *)c->cloud_rows.p;
    q.dist = (float *)c->cloud_dist.p;
    q.m_count = (int *)c->cloud_count.p;
    q.points = points; q.index = index; q.colors = colors; q.labels_out = labels_out; q.count = count;
    hipStream_t st = (hipStream_t)stream;
    if (q.n_grid > 0) HIP_TRY(c, hipMemsetAsync(q.grid, 0xff, sizeof(unsigned) * (size_t)q.n_grid, st));
    Event ev[4];
    hipEvent_t evh[4];
    if (flags & SAS_TIMING)
        for (int k = 0; k < 4; ++k) {
            HIP_TRY(c, hipEventCreate(ev[k].put()));
            evh[k] = ev[k];
        }
    sas_launch_cloud(st, q, (flags & SAS_TIMING) ? evh : nullptr);
    if (const int rc = finish_launches(c, st, "point cloud")) return rc;
    if (flags & SAS_TIMING) {
        std::fill(c->stage_ms, c->stage_ms + SAS_T_COUNT, 0.0f);
        (void)hipEventElapsedTime(&c->stage_ms[SAS_T_PROJECT], evh[0], evh[1]);
        (void)hipEventElapsedTime(&c->stage_ms[SAS_T_SCATTER], evh[1], evh[2]);
        (void)hipEventElapsedTime(&c->stage_ms[SAS_T_BLEND], evh[2], evh[3]);
        (void)hipEventElapsedTime(&c->stage_ms[SAS_T_TOTAL], evh[0], evh[3]);
    }
    return SAS_OK;
}

int sas_fuse_depth(sas_ctx *c, int n_views, int width, int height, const float *depth, const uint8_t *rgb8, const uint8_t *labels,
                   const float *Ks, const float *transform, const uint8_t *keep, const float lo[3], float voxel, const int dims[3],
                   float trunc, float near_z, float pixel_centre, float max_weight, unsigned flags, float *tsdf, float *weight,
                   float *color, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    const char *who = "sas_fuse_depth";
    const int C = n_views;
    if (C < 0) return fail(c, SAS_ERR_INVALID, "%s: n_views %d is negative", who, C);
    if (const int rc = check_depth_views(c, who, C, width, height, depth, Ks, transform, flags, true)) return rc;
    if (!lo || !dims) return fail(c, SAS_ERR_INVALID, "%s: lo and dims are required", who);
    SasFuse q{};
    q.n_vox = 1;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] < 1 || dims[k] > 1024) return fail(c, SAS_ERR_INVALID, "%s: dims[%d] = %d out of [1,1024]", who, k, dims[k]);
        if (!std::isfinite(lo[k])) return fail(c, SAS_ERR_INVALID, "%s: lo[%d] = %g is not finite", who, k, (double)lo[k]);
        q.n_vox *= dims[k];
        q.lo[k] = lo[k];
    }
    if (q.n_vox > (1ll << 27)) return fail(c, SAS_ERR_INVALID, "%s: a volume of more than 2^27 voxels (%d x %d x %d)", who, dims[0], dims[1], dims[2]);
    const struct { const char *name; float v; } positive[] = {{"voxel", voxel}, {"trunc", trunc}, {"near_z", near_z}, {"max_weight", max_weight}};
    for (const auto &a : positive)
        if (!(a.v > 0.0f) || !(a.v < INFINITY)) return fail(c, SAS_ERR_INVALID, "%s: %s %g, must be finite and > 0", who, a.name, (double)a.v);
    if (max_weight < 1.0f) return fail(c, SAS_ERR_INVALID, "%s: max_weight %g, must be >= 1", who, (double)max_weight);
    if (!std::isfinite(pixel_centre)) return fail(c, SAS_ERR_INVALID, "%s: pixel_centre %g is not finite", who, (double)pixel_centre);
    if (keep && !labels) return fail(c, SAS_ERR_INVALID, "%s: keep without labels", who);
    if (color && !rgb8) return fail(c, SAS_ERR_INVALID, "%s: color without rgb8", who);
    if (!tsdf || !weight) return fail(c, SAS_ERR_INVALID, "%s: tsdf and weight are required", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    if (C == 0) return SAS_OK;
    q.W = width; q.H = height;
    q.nx = dims[0]; q.ny = dims[1]; q.nz = dims[2];
    q.voxel = voxel; q.trunc = trunc; q.near_z = near_z; q.pixel_centre = pixel_centre; q.max_weight = max_weight;
    q.tsdf = tsdf; q.weight = weight; q.color = color;
    // the per-view rows and the keep table: one host block, one copy per launch (one launch unless the call has more than
    // SAS_FUSE_MAX_ROWS views: then launches in view order, which is what the contract's view order asks for)
    const int rows_max = std::min(C, SAS_FUSE_MAX_ROWS);
    const size_t off_keep = sizeof(SasDepthView) * (size_t)rows_max;
    std::vector<unsigned char> par(off_keep + 256);
    if (keep) std::copy(keep, keep + 256, par.data() + off_keep);
    if (const int rc = ensure(c, c->fuse_par, par.size())) return rc;
    unsigned char *dpar = (unsigned char *)c->fuse_par.p;
    q.view = reinterpret_cast<const SasDepthView *>(dpar);
    q.keep = keep ? dpar + off_keep : nullptr;
    hipStream_t st = (hipStream_t)stream;
    Event ev[2];
    if (flags & SAS_TIMING) {
        for (int k = 0; k < 2; ++k) HIP_TRY(c, hipEventCreate(ev[k].put()));
        HIP_TRY(c, hipEventRecord(ev[0], st));
    }
    const size_t px = (size_t)width * (size_t)height;
    for (int v0 = 0; v0 < C; v0 += rows_max) {
        const int n = std::min(rows_max, C - v0);
        SasDepthView *view = reinterpret_cast<SasDepthView *>(par.data());
        for (int r = 0; r < n; ++r)
            view[r] = pack_depth_view(Ks + 9 * (size_t)(v0 + r), transform ? transform + 12 * (size_t)(v0 + r) : nullptr);
        // (the block is the call's own: the launch before this one, if any, has been waited for)
        HIP_TRY(c, hipMemcpy(dpar, par.data(), par.size(), hipMemcpyHostToDevice));
        q.C = q.n_rows = n;
        q.n_pix = (long long)n * (long long)px;
        q.depth = depth + (size_t)v0 * px;
        q.rgb8 = rgb8 ? rgb8 + 3 * (size_t)v0 * px : nullptr;
        q.labels = labels ? labels + (size_t)v0 * px : nullptr;
        sas_launch_fuse(st, q);
        // (SAS_TIMING: the closing stamp goes behind the last launch, in front of its wait)
        if (const int rc = finish_launches(c, st, "depth fusion", v0 + n == C && (flags & SAS_TIMING) ? (hipEvent_t)ev[1] : nullptr)) return rc;
    }
    if (flags & SAS_TIMING) {
        std::fill(c->stage_ms, c->stage_ms + SAS_T_COUNT, 0.0f);
        (void)hipEventElapsedTime(&c->stage_ms[SAS_T_BLEND], ev[0], ev[1]);
        c->stage_ms[SAS_T_TOTAL] = c->stage_ms[SAS_T_BLEND];
    }
    return SAS_OK;
}

int sas_render_rgbd(sas_ctx *c, const float *viewmat, const float *K, int width, int height, const float *background,
                    unsigned flags, const float *max_depth, float *rgb, float *alpha, float *depth, float *points,
                    uint8_t *mask, void *stream)
{
    const ViewCall v = {viewmat, K, {rgb, alpha, depth, nullptr, points, mask}};
    return render_views(c, &v, 1, width, height, background, flags, max_depth, stream, false, !(flags & SAS_ASYNC));
}

// label frames of a batch (sas_render_batch_labels): every view also delivers labels [H,W]
struct LabelOut {
    uint8_t *labels = nullptr;   // [n_views,H,W] device
    float min_alpha = 0.0f;
};

// pose sets of a batch: view v is rendered with rows pose_sets[pose_set[v]] (each set [n_groups,12]); no sets: the
// context's current poses for every view
struct PoseSets {
    const int *pose_set = nullptr;
    int n_sets = 0;
    const float *Rt = nullptr;
};

static int render_batch_impl(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height,
                             const float *background, unsigned flags, float *rgb, float *alpha, float *depth, uint8_t *rgb8,
                             uint8_t *rgb8_host, void *stream, const PoseSets &ps = PoseSets(), const LabelOut &lab = LabelOut())
{
    if (!c) return SAS_ERR_INVALID;
    flags = frame_flags(c, flags);
    if (lab.labels) flags |= SAS_FULL_SORT;   // the labels are composited from the complete tile lists, one view per frame
    if (n_views < 0 || (n_views > 0 && (!viewmats || !Ks))) return fail(c, SAS_ERR_INVALID, "bad view batch");
    if (ps.Rt) {
        if (!has(c, HAVE_SCENE)) return fail(c, SAS_ERR_NO_SCENE, "no scene uploaded");
        if (c->scene.n_groups <= 0) return fail(c, SAS_ERR_INVALID, "pose sets given but the scene has no splat groups");
        if (ps.n_sets <= 0 || !ps.pose_set) return fail(c, SAS_ERR_INVALID, "pose sets need pose_set[n_views] and n_sets > 0");
        for (int v = 0; v < n_views; ++v)
            if (ps.pose_set[v] < 0 || ps.pose_set[v] >= ps.n_sets)
                return fail(c, SAS_ERR_INVALID, "pose_set[%d]=%d out of [0,%d)", v, ps.pose_set[v], ps.n_sets);
    }
    const size_t px = (size_t)width * (size_t)height;
    auto view = [&](int v) {
        ViewCall vc{viewmats + 16 * v, Ks + 9 * v, {rgb ? rgb + 3 * px * v : nullptr, alpha ? alpha + px * v : nullptr,
                    depth ? depth + px * v : nullptr, rgb8 ? rgb8 + 3 * px * v : nullptr}};
        vc.out.rgb8_host = rgb8_host ? rgb8_host + 3 * px * v : nullptr;
        vc.poses = ps.Rt ? ps.Rt + (size_t)12 * c->scene.n_groups * ps.pose_set[v] : nullptr;
        vc.out.labels = lab.labels ? lab.labels + px * v : nullptr;
        vc.min_alpha = lab.min_alpha;
        return vc;
    };
    // Views go through the frame slots two at a time: one pass over the scene projects both
    // (timed and full-sort frames keep to one view per pass; so do two views of different pose sets).
    const bool want_pairs = c->pair_views < 0 ? c->scene.n >= sas_ctx::kPairMinGaussians : c->pair_views != 0;
    const bool share = !(flags & (SAS_TIMING | SAS_FULL_SORT));
    const bool pair = share && want_pairs && c->n_slots >= 2;
    // small scenes (not paired): launch groups, by default half of the slots each so that two can be in flight
    int gsz = c->group_views > 0 ? c->group_views : std::max(2, c->n_slots / 2);
    gsz = std::min(std::min(gsz, SAS_MAX_GROUP), c->n_slots);
    const bool group = share && !pair && gsz >= 2 && n_views >= 2;
    for (int v = 0; v < n_views;) {
        if (group && v + 1 < n_views) {
            const int n = std::min(gsz, n_views - v);
            ViewCall vc[SAS_MAX_GROUP];
            for (int k = 0; k < n; ++k) vc[k] = view(v + k);
            int rc = render_views(c, vc, n, width, height, background, flags | SAS_ASYNC, nullptr, stream, true);
            if (rc) return rc;
            v += n;
            continue;
        }
        const ViewCall v0 = view(v);
        const int n = (pair && v + 1 < n_views && view(v + 1).poses == v0.poses) ? 2 : 1;
        const ViewCall vc[2] = {v0, view(n == 2 ? v + 1 : v)};
        int rc = render_views(c, vc, n, width, height, background, flags | SAS_ASYNC, nullptr, stream, false, n_views == 1 && !(flags & SAS_ASYNC));
        if (rc) return rc;
        v += n;
    }
    if (flags & SAS_ASYNC) return SAS_OK;
    return sas_wait(c);
}

int sas_render_batch(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height,
                     const float *background, unsigned flags, float *rgb, float *alpha, float *depth, uint8_t *rgb8,
                     void *stream)
{
    return render_batch_impl(c, n_views, viewmats, Ks, width, height, background, flags, rgb, alpha, depth, rgb8, nullptr, stream);
}

int sas_render_batch_posed(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, const int *pose_set, int n_sets,
                           const float *Rt, int width, int height, const float *background, unsigned flags, float *rgb,
                           float *alpha, float *depth, uint8_t *rgb8, void *stream)
{
    const PoseSets ps = {pose_set, n_sets, Rt};
    if (!Rt) return fail(c, SAS_ERR_INVALID, "sas_render_batch_posed: Rt is required");
    return render_batch_impl(c, n_views, viewmats, Ks, width, height, background, flags, rgb, alpha, depth, rgb8, nullptr, stream, ps);
}

// What a label frame needs in place, and the flags it takes: the call selects no store behind the caller's back.
static int check_labels(sas_ctx *c, const char *who, unsigned flags, const uint8_t *labels)
{
    if (const int rc = need_scene(c, who)) return rc;
    if (!labels) return fail(c, SAS_ERR_INVALID, "%s: the labels output is required", who);
    if (flags & SAS_ASYNC) return fail(c, SAS_ERR_INVALID, "%s: blocking only (SAS_ASYNC is not supported)", who);
    if (flags & ~(SAS_MESH_SURFACE | SAS_DEPTH_FILL_MAX | SAS_FAST_EXP | SAS_TIMING))
        return fail(c, SAS_ERR_INVALID, "%s: flags 0x%x not accepted (SAS_MESH_SURFACE, SAS_DEPTH_FILL_MAX, SAS_FAST_EXP, SAS_TIMING)", who, flags);
    if (!has(c, HAVE_FEAT)) return fail(c, SAS_ERR_INVALID, "%s: no feature store; label frames need the one-hot group store (sas_scene_features with NULL)", who);
    if (!c->feat_onehot)
        return fail(c, SAS_ERR_INVALID, "%s: the feature store holds the caller's features, not the one-hot group store (sas_scene_features with NULL)", who);
    if (has(c, HAVE_MESH) && !(has(c, HAVE_MESH_FEAT) && c->mesh_feat_onehot))
        return fail(c, SAS_ERR_INVALID, "%s: the meshes lack their one-hot rows (sas_scene_mesh_features with NULL)", who);
    return SAS_OK;
}

int sas_render_batch_labels(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height,
                            const float *background, float min_alpha, unsigned flags, float *rgb, float *alpha, float *depth,
                            uint8_t *rgb8, uint8_t *labels, void *stream)
{
    if (const int rc = check_labels(c, "sas_render_batch_labels", flags, labels)) return rc;
    const LabelOut lab = {labels, min_alpha};
    return render_batch_impl(c, n_views, viewmats, Ks, width, height, background, flags, rgb, alpha, depth, rgb8, nullptr, stream, PoseSets(), lab);
}

int sas_render_batch_labels_posed(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, const int *pose_set, int n_sets,
                                  const float *Rt, int width, int height, const float *background, float min_alpha, unsigned flags,
                                  float *rgb, float *alpha, float *depth, uint8_t *rgb8, uint8_t *labels, void *stream)
{
    if (const int rc = check_labels(c, "sas_render_batch_labels_posed", flags, labels)) return rc;
    if (!Rt) return fail(c, SAS_ERR_INVALID, "sas_render_batch_labels_posed: Rt is required");
    const PoseSets ps = {pose_set, n_sets, Rt};
    const LabelOut lab = {labels, min_alpha};
    return render_batch_impl(c, n_views, viewmats, Ks, width, height, background, flags, rgb, alpha, depth, rgb8, nullptr, stream, ps, lab);
}

// What every lift call checks first, and the flags it takes.
static int check_lift(sas_ctx *c, const char *who, unsigned flags)
{
    if (const int rc = need_scene(c, who)) return rc;
    if (flags & ~(SAS_FAST_EXP | SAS_TIMING))
        return fail(c, SAS_ERR_INVALID, "%s: flags 0x%x not accepted (SAS_FAST_EXP, SAS_TIMING; blocking only)", who, flags);
    if (has(c, HAVE_MESH))
        return fail(c, SAS_ERR_INVALID, "%s: lift frames do not take occlusion by meshes; clear the meshes first (sas_scene_meshes with none)", who);
    return SAS_OK;
}

// The views of a lift call; `view_out(v)` names view v's image and the sums it adds to.
// Lift frames are SAS_FULL_SORT frames: one view at a time through the frame slots, nothing drains between views.  (A frame that
// outgrew its key buffer adds nothing and is rendered again: k_lift_labels, k_lift_features.)
static int lift_views(sas_ctx *c, const char *who, int n_views, const float *viewmats, const float *Ks, int width, int height,
                      unsigned flags, void *stream, const std::function<ViewOut(int)> &view_out)
{
    if (n_views < 1 || !viewmats || !Ks) return fail(c, SAS_ERR_INVALID, "%s: bad view batch (n_views %d)", who, n_views);
    if (width <= 0 || height <= 0) return fail(c, SAS_ERR_INVALID, "%s: bad image size %dx%d", who, width, height);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // frames in flight are completed first
    for (int v = 0; v < n_views; ++v) {
        ViewCall vc{viewmats + 16 * v, Ks + 9 * v, view_out(v)};
        if (const int rc = render_views(c, &vc, 1, width, height, nullptr, flags | SAS_FULL_SORT | SAS_ASYNC, nullptr, stream)) return rc;
    }
    return sas_wait(c);
}

int sas_lift_labels(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height, const uint8_t *labels,
                    int n_labels, unsigned flags, int64_t *votes, int64_t *seen, void *stream)
{
    if (const int rc = check_lift(c, "sas_lift_labels", flags)) return rc;
    if (n_labels < 1 || n_labels > 256) return fail(c, SAS_ERR_INVALID, "sas_lift_labels: n_labels %d out of [1,256]", n_labels);
    if (!labels) return fail(c, SAS_ERR_INVALID, "sas_lift_labels: the label images are required");
    if (!votes && !seen) return fail(c, SAS_ERR_INVALID, "sas_lift_labels: votes and seen are both NULL");
    const size_t px = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0);
    return lift_views(c, "sas_lift_labels", n_views, viewmats, Ks, width, height, flags, stream, [&](int v) {
        ViewOut o;
        o.reader = ViewOut::LIFT_LABELS;
        o.lift = SasLift{labels + px * v, (unsigned long long *)votes, (unsigned long long *)seen, c->scene.n, n_labels};
        return o;
    });
}

int sas_lift_features(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height, const float *images,
                      int channels, float feature_scale, const uint8_t *mask, unsigned flags, int64_t *sums, int64_t *weight,
                      void *stream)
{
    if (const int rc = check_lift(c, "sas_lift_features", flags)) return rc;
    if (channels < 1 || channels > SAS_MAX_FEATURES)
        return fail(c, SAS_ERR_INVALID, "sas_lift_features: channels %d out of [1,%d]", channels, SAS_MAX_FEATURES);
    if (!(feature_scale > 0.0f) || !std::isfinite(feature_scale))
        return fail(c, SAS_ERR_INVALID, "sas_lift_features: feature_scale %g is not finite and positive", (double)feature_scale);
    if (!images) return fail(c, SAS_ERR_INVALID, "sas_lift_features: the feature images are required");
    if (!sums && !weight) return fail(c, SAS_ERR_INVALID, "sas_lift_features: sums and weight are both NULL");
    const size_t px = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0);
    return lift_views(c, "sas_lift_features", n_views, viewmats, Ks, width, height, flags, stream, [&](int v) {
        ViewOut o;
        o.reader = ViewOut::LIFT_FEATURES;
        o.lift_features = SasLiftFeatures{images + px * (size_t)channels * v, mask ? mask + px * v : nullptr, (unsigned long long *)sums,
                                          (unsigned long long *)weight, c->scene.n, channels, feature_scale};
        return o;
    });
}

// a rate or a threshold: finite and not negative
static int check_rate(sas_ctx *c, const char *who, const char *what, float v)
{
    return v >= 0.0f && v < INFINITY ? SAS_OK : fail(c, SAS_ERR_INVALID, "%s: %s %g is negative or not finite", who, what, (double)v);
}

// A scene holds quaternions and scales or covariances: the arrays of the other form are refused (`d`: "d_" for gradients, "" for values).
static int check_form(sas_ctx *c, const char *who, bool quats_or_scales, bool cov6, const char *d)
{
    const bool cov = c->scene.cov_mode != 0;
    if (cov ? !quats_or_scales : !cov6) return SAS_OK;
    char ask[48];
    snprintf(ask, sizeof(ask), cov ? "%scov6" : "%squats / %sscales", d, d);
    return fail(c, SAS_ERR_INVALID, "%s: the scene was uploaded as %s: ask for %s", who, cov ? "covariances" : "quaternions and scales", ask);
}

// Behind work on the caller's stream that reads or writes what the frames' own streams touch (a frame's projection does not wait for the
// caller's stream: enqueue_chain, ORDER): every slot's stream is put behind it.
static int slots_wait_for(sas_ctx *c, Event &ev, hipStream_t st)
{
    if (!ev.h) HIP_TRY(c, hipEventCreateWithFlags(ev.put(), hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(ev, st));
    for (int s = 0; s < c->n_slots; ++s) HIP_TRY(c, hipStreamWaitEvent(c->slots[s].fs, ev, 0));
    return SAS_OK;
}

// A backward frame's ViewOut: the view's pixel gradients and the five screen-space sums it adds to.
static ViewOut grad_view(const SasGrad &tiles)
{
    ViewOut o;
    o.reader = ViewOut::BACKWARD;
    o.back.tiles = tiles;
    return o;
}

// The backward pass of one view on its complete lists (k_grad_tiles): a lift frame whose sums are the screen-space gradients.
int sas_render_backward_screen(sas_ctx *c, const float *viewmat, const float *K, int width, int height, unsigned flags,
                               const float *g_rgb, const float *g_alpha, const float *g_depth, float *d_means2d, float *d_conics,
                               float *d_opacities, float *d_colors, float *d_depths, void *stream)
{
    if (const int rc = check_lift(c, "sas_render_backward_screen", flags)) return rc;
    if (!g_rgb && !g_alpha && !g_depth) return fail(c, SAS_ERR_INVALID, "sas_render_backward_screen: g_rgb, g_alpha and g_depth are all NULL");
    if (!d_means2d && !d_conics && !d_opacities && !d_colors && !d_depths)
        return fail(c, SAS_ERR_INVALID, "sas_render_backward_screen: every output is NULL");
    const int rc = lift_views(c, "sas_render_backward_screen", 1, viewmat, K, width, height, flags, stream,
                              [&](int) { return grad_view({g_rgb, g_alpha, g_depth, d_means2d, d_conics, d_opacities, d_colors, d_depths, c->scene.n}); });
    if (!rc) c->grad_frame = 1;
    return rc;
}

// ... and chained through the view's projection (k_grad_project): the screen-space sums live in the context's scratch, zeroed on the
// caller's stream in front of the frame.
static int render_backward(sas_ctx *c, const char *who, const float *viewmat, const float *K, int width, int height, unsigned flags,
                           const float *g_rgb, const float *g_alpha, const float *g_depth, float *d_means, float *d_opacities, float *d_sh,
                           float *d_quats, float *d_scales, float *d_cov6, float *d_viewmat, int n_sel, const uint8_t *sel,
                           float *d_group_poses, void *stream)
{
    if (const int rc = check_lift(c, who, flags)) return rc;
    if (!g_rgb && !g_alpha && !g_depth) return fail(c, SAS_ERR_INVALID, "%s: g_rgb, g_alpha and g_depth are all NULL", who);
    if (n_sel < 0 || n_sel > SAS_MAX_POSE_GRAD_GROUPS)
        return fail(c, SAS_ERR_INVALID, "%s: n_sel %d out of [0,%d]", who, n_sel, SAS_MAX_POSE_GRAD_GROUPS);
    if (!d_means && !d_opacities && !d_sh && !d_quats && !d_scales && !d_cov6 && !d_viewmat && !(n_sel > 0 && d_group_poses))
        return fail(c, SAS_ERR_INVALID, "%s: every output is NULL", who);
    SasPoseSel S{};
    if (n_sel > 0) {
        if (!sel || !d_group_poses) return fail(c, SAS_ERR_INVALID, "%s: n_sel %d but sel or d_group_poses is NULL", who, n_sel);
        if (c->scene.n_groups <= 0) return fail(c, SAS_ERR_INVALID, "%s: the scene was uploaded without splat groups: it has no group poses", who);
        bool seen[256] = {};
        for (int q = 0; q < n_sel; ++q) {
            if ((int)sel[q] >= c->scene.n_groups) return fail(c, SAS_ERR_INVALID, "%s: sel[%d]=%d >= n_groups=%d", who, q, (int)sel[q], c->scene.n_groups);
            if (seen[sel[q]]) return fail(c, SAS_ERR_INVALID, "%s: sel[%d]=%d is a duplicate", who, q, (int)sel[q]);
            seen[sel[q]] = true;
            S.ids[q >> 2] |= (unsigned)sel[q] << (8 * (q & 3));
        }
        S.n_sel = n_sel;
        S.d_group_poses = d_group_poses;
    }
    if (const int rc = check_form(c, who, d_quats || d_scales, d_cov6 != nullptr, "d_")) return rc;
    if (width <= 0 || height <= 0) return fail(c, SAS_ERR_INVALID, "%s: bad image size %dx%d", who, width, height);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->scene.n, n_wg = (n + 255) / 256;
    const size_t floats = 10 * n + 12 * n_wg;   // (zeroed; the pose rows behind them are all written by the kernel)
    if (const int rc = ensure(c, c->grad_screen, (floats + 12 * n_wg * (size_t)n_sel) * sizeof(float))) return rc;
    float *s = (float *)c->grad_screen.p;
    if (const int rc = complete_all(c)) return rc;   // (nothing in flight reads the scratch)
    HIP_TRY(c, hipMemsetAsync(s, 0, floats * sizeof(float), (hipStream_t)stream));
    S.partial = n_sel > 0 ? s + floats : nullptr;
    const int rc = lift_views(c, who, 1, viewmat, K, width, height, flags, stream, [&](int) {
        ViewOut o = grad_view({g_rgb, g_alpha, g_depth, s, s + 2 * n, s + 5 * n, s + 6 * n, s + 9 * n, c->scene.n});
        const SasGrad &g = o.back.tiles;
        o.back.proj = SasGradProj{g.d_means2d, g.d_conics, g.d_opacities, g.d_colors, g.d_depths, d_means, d_opacities, d_sh, d_quats, d_scales,
                                  d_cov6, d_viewmat ? s + 10 * n : nullptr, d_viewmat, c->scene.n};
        o.back.poses = S;
        return o;
    });
    if (!rc) c->grad_frame = 2;   // (sas_density_accumulate may read the sums in grad_screen)
    return rc;
}

int sas_render_backward(sas_ctx *c, const float *viewmat, const float *K, int width, int height, unsigned flags, const float *g_rgb,
                        const float *g_alpha, const float *g_depth, float *d_means, float *d_opacities, float *d_sh, float *d_quats,
                        float *d_scales, float *d_cov6, float *d_viewmat, void *stream)
{
    return render_backward(c, "sas_render_backward", viewmat, K, width, height, flags, g_rgb, g_alpha, g_depth, d_means, d_opacities, d_sh,
                           d_quats, d_scales, d_cov6, d_viewmat, 0, nullptr, nullptr, stream);
}

// ... and to the poses of the selected groups (k_grad_project<true>): one row of scratch per (workgroup, selected group) behind the
// view-matrix rows.
int sas_render_backward_poses(sas_ctx *c, const float *viewmat, const float *K, int width, int height, unsigned flags, const float *g_rgb,
                              const float *g_alpha, const float *g_depth, float *d_means, float *d_opacities, float *d_sh, float *d_quats,
                              float *d_scales, float *d_cov6, float *d_viewmat, int n_sel, const uint8_t *sel, float *d_group_poses,
                              void *stream)
{
    return render_backward(c, "sas_render_backward_poses", viewmat, K, width, height, flags, g_rgb, g_alpha, g_depth, d_means, d_opacities,
                           d_sh, d_quats, d_scales, d_cov6, d_viewmat, n_sel, sel, d_group_poses, stream);
}

static int redeform(sas_ctx *c, hipStream_t st);

// The fused Adam step (k_adam_scene) behind sas_scene_adam_step and sas_scene_adam_step_rest.  Host work: validation, the first-step
// allocations, one launch, one event.  rest: the planes stepped are the skin's rest planes (colours step where they live: they are no part of
// the snapshot), and the last deformation is applied to the stepped rest planes again.
static int adam_step(sas_ctx *c, const char *who, bool rest, const sas_adam_config *cfg, const float *d_means, const float *d_opacities,
                     const float *d_sh, const float *d_quats, const float *d_scales, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    if (!cfg) return fail(c, SAS_ERR_INVALID, "%s: cfg is NULL", who);
    if (const int rc = need_scene(c, who)) return rc;
    if (!rest) {
        if (const int rc = need_unskinned(c, who)) return rc;
    } else if (!c->skin.bound()) {
        return fail(c, SAS_ERR_INVALID, "%s: no skin is bound: the unskinned scene steps through sas_scene_adam_step", who);
    }
    if (!d_means && !d_opacities && !d_sh && !d_quats && !d_scales) return fail(c, SAS_ERR_INVALID, "%s: every gradient is NULL", who);
    if (cfg->step < 1) return fail(c, SAS_ERR_INVALID, "%s: step %d < 1 (the count is 1-based)", who, cfg->step);
    for (const float lr : {cfg->lr_means, cfg->lr_opacities, cfg->lr_sh_dc, cfg->lr_sh_rest, cfg->lr_quats, cfg->lr_scales})
        if (const int rc = check_rate(c, who, "learning rate", lr)) return rc;
    if (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f))
        return fail(c, SAS_ERR_INVALID, "%s: betas (%g, %g) outside [0, 1)", who, (double)cfg->beta1, (double)cfg->beta2);
    if (const int rc = check_rate(c, who, "eps", cfg->eps)) return rc;
    if (cfg->flags & ~SAS_ADAM_VISIBLE_ONLY) return fail(c, SAS_ERR_INVALID, "%s: unknown flags 0x%x", who, cfg->flags);
    if (c->scene.cov_mode && (d_quats || d_scales))
        return fail(c, SAS_ERR_INVALID, "%s: the scene was uploaded as covariances, which are not variables: d_quats / d_scales must be NULL", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // (no frame reads the planes while they change)
    const SasScene &sc = c->scene;
    const bool on_means = d_means && cfg->lr_means > 0.0f, on_opac = d_opacities && cfg->lr_opacities > 0.0f,
               on_sh = d_sh && (cfg->lr_sh_dc > 0.0f || cfg->lr_sh_rest > 0.0f), on_quats = d_quats && cfg->lr_quats > 0.0f,
               on_scales = d_scales && cfg->lr_scales > 0.0f;
    if (sc.n <= 0 || !(on_means || on_opac || on_sh || on_quats || on_scales)) return SAS_OK;   // nothing moves: the last frame stays valid
    bool stepped[Adam::GROUPS];
    stepped[Adam::MEANS] = on_means; stepped[Adam::OPACITIES] = on_opac; stepped[Adam::SH] = on_sh; stepped[Adam::QUATS] = on_quats; stepped[Adam::SCALES] = on_scales;
    hipStream_t st = (hipStream_t)stream;
    const int coeff_floats = sas_coeff_floats(sc.sh_degree), planes = sas_colour_planes(sc.sh_degree);
    Adam &a = c->adam;
    // a group stepped for the first time: zero moments (and raw values from the resident ones), on the caller's stream, group by group
    bool fresh[Adam::GROUPS];
    for (int g = 0; g < Adam::GROUPS; ++g) {
        fresh[g] = stepped[g] && !a.on[g];
        for (int k = 0; k < Adam::kRows && fresh[g]; ++k)
            if (Adam::rows[k].group == g)
                if (const int rc = a.alloc(c, k, sc.n_pad, planes, st, Adam::rows[k].zeroed)) return rc;
    }
    if (fresh[Adam::OPACITIES] || fresh[Adam::SCALES]) {
        sas_launch_adam_init(st, sc.n, rest ? (const float4 *)c->skin.rest0.p : sc.g0, rest ? (const float4 *)c->skin.rest2.p : sc.g2, a.view(fresh));
        HIP_TRY(c, hipGetLastError());
    }
    for (int g = 0; g < Adam::GROUPS; ++g) a.on[g] = a.on[g] || fresh[g];
    SasAdam k{};
    k.g0 = (float4 *)(rest ? c->skin.rest0.p : c->planes.g0.p);
    k.g1 = (float4 *)(rest ? c->skin.rest1.p : c->planes.g1.p);
    k.g2 = (float4 *)(rest ? c->skin.rest2.p : c->planes.g2.p);
    k.col = (float4 *)c->planes.col.p;
    k.perm = sc.perm;
    k.n = sc.n; k.n_pad = sc.n_pad;
    k.coeff_floats = coeff_floats; k.planes = planes;
    k.d_means = on_means ? d_means : nullptr;
    k.d_opac = on_opac ? d_opacities : nullptr;
    k.d_sh = on_sh ? d_sh : nullptr;
    k.d_quats = on_quats ? d_quats : nullptr;
    k.d_scales = on_scales ? d_scales : nullptr;
    k.s = a.view();
    k.lr_means = cfg->lr_means; k.lr_opac = cfg->lr_opacities; k.lr_sh_dc = cfg->lr_sh_dc; k.lr_sh_rest = cfg->lr_sh_rest;
    k.lr_quats = cfg->lr_quats; k.lr_scales = cfg->lr_scales;
    k.beta1 = cfg->beta1; k.beta2 = cfg->beta2;
    k.omb1 = 1.0f - cfg->beta1; k.omb2 = 1.0f - cfg->beta2;
    k.bc1 = (float)(1.0 - std::pow((double)cfg->beta1, (double)cfg->step));
    k.bc2 = (float)(1.0 - std::pow((double)cfg->beta2, (double)cfg->step));
    k.eps = cfg->eps;
    k.visible_only = (cfg->flags & SAS_ADAM_VISIBLE_ONLY) != 0;
    k.sh_aligned = coeff_floats % 4 == 0 && ((uintptr_t)d_sh & 15u) == 0;
    if (rest && c->skin_done.h) HIP_TRY(c, hipStreamWaitEvent(st, c->skin_done, 0));   // (the snapshot and the records were made on a caller's stream)
    sas_launch_adam_scene(st, k);
    HIP_TRY(c, hipGetLastError());
    if (rest)
        if (const int rc = redeform(c, st)) return rc;   // the live planes: the stepped rest scene in its current bend
    if (const int rc = slots_wait_for(c, rest ? c->skin_done : c->adam_done, st)) return rc;
    scene_changed(c, Changed::Values);   // the last frame showed the scene before the step
    return SAS_OK;
}

int sas_scene_adam_step(sas_ctx *c, const sas_adam_config *cfg, const float *d_means, const float *d_opacities, const float *d_sh,
                        const float *d_quats, const float *d_scales, void *stream)
{
    return adam_step(c, "sas_scene_adam_step", false, cfg, d_means, d_opacities, d_sh, d_quats, d_scales, stream);
}

// ... on the REST planes of a skinned scene: the same kernel, the same optimiser state.
int sas_scene_adam_step_rest(sas_ctx *c, const sas_adam_config *cfg, const float *d_means, const float *d_opacities, const float *d_sh,
                             const float *d_quats, const float *d_scales, void *stream)
{
    return adam_step(c, "sas_scene_adam_step_rest", true, cfg, d_means, d_opacities, d_sh, d_quats, d_scales, stream);
}

// The photometric loss and its gradient (k_loss_stats, k_loss_tail, k_loss_grad).  Host work: validation, the scratch, the window, the launches.
int sas_photometric_loss(sas_ctx *c, int width, int height, const float *rgb, const float *target, const uint8_t *mask_or_null,
                         const float *alpha_or_null, const float *background, float lambda_dssim, float *terms, float *g_rgb_or_null,
                         float *g_alpha_or_null, void *stream)
{
    const char *who = "sas_photometric_loss";
    if (!c) return SAS_ERR_INVALID;
    if (width <= 0 || height <= 0) return fail(c, SAS_ERR_INVALID, "%s: bad image size %dx%d", who, width, height);
    if (!rgb || !target || !terms) return fail(c, SAS_ERR_INVALID, "%s: rgb, target and terms are required", who);
    if (!(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f)) return fail(c, SAS_ERR_INVALID, "%s: lambda_dssim %g outside [0, 1]", who, (double)lambda_dssim);
    if (g_alpha_or_null && !alpha_or_null) return fail(c, SAS_ERR_INVALID, "%s: g_alpha is the prechained form: it requires alpha", who);
    if (alpha_or_null && !background) return fail(c, SAS_ERR_INVALID, "%s: alpha given without a background", who);
    HIP_TRY(c, hipSetDevice(c->device));
    SasLoss q{};
    q.x = rgb; q.y = target; q.mask = mask_or_null;
    q.W = width; q.H = height;
    q.tiles_x = (width + 15) / 16; q.tiles_y = (height + 15) / 16;
    q.lambda = lambda_dssim;
    double g[11], sum = 0.0;
    for (int k = 0; k < 11; ++k) sum += g[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < 11; ++k) q.win[k] = (float)(g[k] / sum);
    for (int k = 0; k < 3; ++k) q.bg[k] = alpha_or_null ? background[k] : 0.0f;
    q.gate = alpha_or_null != nullptr;
    const bool grad = g_rgb_or_null || g_alpha_or_null;
    const size_t n_pix = (size_t)width * (size_t)height, tiles = (size_t)q.tiles_x * (size_t)q.tiles_y;
    const size_t map_floats = grad && lambda_dssim != 0.0f ? 9 * n_pix : 0;
    if (const int rc = ensure(c, c->loss_scratch, sizeof(float) * (map_floats + 4 * tiles + 4))) return rc;
    float *s = (float *)c->loss_scratch.p;
    q.maps = map_floats ? s : nullptr;
    q.partial = s + map_floats;
    q.norm = q.partial + 4 * tiles;
    q.terms = terms;
    q.g_rgb = g_rgb_or_null; q.g_alpha = g_alpha_or_null;
    sas_launch_loss((hipStream_t)stream, q);
    HIP_TRY(c, hipGetLastError());
    return SAS_OK;
}

int sas_scene_adam_reset(sas_ctx *c)
{
    if (!c) return SAS_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    return c->adam.drop(c);   // (hipFree waits for the step that may still be using the state)
}

// The statistics of the last backward frame (k_density_accumulate): its info records are in the slot's scratch, its screen-space sums in the
// caller's array or in grad_screen.
int sas_density_accumulate(sas_ctx *c, int width, int height, const float *d_means2d, float *grad_sum, int32_t *count, float *max_radius,
                           void *stream)
{
    const char *who = "sas_density_accumulate";
    if (const int rc = need_scene(c, who)) return rc;
    if (width <= 0 || height <= 0) return fail(c, SAS_ERR_INVALID, "%s: bad image size %dx%d", who, width, height);
    if (!grad_sum || !count) return fail(c, SAS_ERR_INVALID, "%s: grad_sum and count are required", who);
    if (!c->has_frame || c->grad_frame == 0)
        return fail(c, SAS_ERR_NO_SCENE, "%s: no backward frame since the last upload, optimiser step, densify or opacity reset", who);
    if (!d_means2d && c->grad_frame != 2)
        return fail(c, SAS_ERR_NO_SCENE, "%s: d_means2d is NULL and the last backward frame was not sas_render_backward's: the context holds no sums", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    const Slot &ls = c->slots[c->last_slot];
    if (!ls.info_kept) return fail(c, SAS_ERR_INVALID, "%s: the backward frame kept no radii", who);
    SasDensityStats q{};
    q.info = (const uint4 *)ls.scr.info.p;
    q.perm = c->scene.perm;
    q.d_means2d = d_means2d ? d_means2d : (const float *)c->grad_screen.p;
    q.grad_sum = grad_sum; q.count = count; q.max_radius = max_radius;
    q.n = c->scene.n;
    q.half_w = 0.5f * (float)width; q.half_h = 0.5f * (float)height;
    hipStream_t st = (hipStream_t)stream;
    sas_launch_density_accumulate(st, q);
    HIP_TRY(c, hipGetLastError());
    return slots_wait_for(c, c->density_done, st);   // (the next frame of that slot writes its info records anew)
}

// The host clock of a densify or refine call, lap by lap (sas_scene_densify_times).
struct Laps {
    using clock = std::chrono::steady_clock;
    float *ms;
    clock::time_point t0 = clock::now();
    void operator()(int k)
    {
        const auto t1 = clock::now();
        ms[k] = std::chrono::duration<float, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

// The rows of a new scene in the caller's order (device, as sas_scene_upload takes them), each new Gaussian's old index, and which rows
// start their optimiser state anew: the ones `fresh` marks, or (nullptr) the ones from n_survivors on.
struct NewRows {
    int64_t n;
    const float *means, *quats, *scales, *cov6, *opac, *colors;
    const uint8_t *gid;       // or nullptr: no groups
    const int *parents;
    const uint8_t *fresh;
    int64_t n_survivors;
};

// The tail sas_scene_densify and sas_scene_mcmc_refine share: the storage order of the new rows (device_order, where they lie; SAS_ORDER=0: on the host, from read-back copies), new planes
// and new optimiser state beside the old ones, relayout, the carried state, and the swap.  inv_old: caller's index -> old slot.  Laps 1 to 3
// are taken here.  Nothing changes the context before the last wait: a failure leaves the scene as it was.
static int commit_rows(sas_ctx *c, const NewRows &r, const int *inv_old, hipStream_t st, Laps &lap)
{
    const SasScene sc = c->scene;
    const int coeff_floats = sas_coeff_floats(sc.sh_degree), planes = sas_colour_planes(sc.sh_degree);
    int rc;
    Planes np;
    Adam na;
    if (c->order_on_device) {
        // the new `perm` alone, in front of lap 1: lap 2 is the order's enqueue and nothing else (np.alloc below finds it in place)
        if ((rc = ensure(c, np.perm, sizeof(int) * (size_t)std::max<int64_t>((r.n + 63) & ~63ll, 64)))) return rc;
        lap(1);   // (the scatter's enqueue: nothing is read back for the order)
        if ((rc = device_order(c, r.n, r.means, r.gid, (int *)np.perm.p, st))) return rc;
        lap(2);
        if ((rc = np.alloc(c, r.n, planes))) return rc;   // (in lap 3, as on the host path)
    } else {   // SAS_ORDER=0
        OrderInput in;
        if ((rc = in.fetch(c, r.n, r.means, r.gid, true, st))) return rc;
        lap(1);
        in.order(np.perm_host);
        np.perm_host_valid = true;
        lap(2);
        if ((rc = np.alloc(c, r.n, planes))) return rc;
    }
    std::copy(c->adam.on, c->adam.on + Adam::GROUPS, na.on);
    for (int k = 0; k < Adam::kRows; ++k)   // (every buffer zeroed: the lanes n .. n_pad)
        if (na.on[Adam::rows[k].group] && (rc = na.alloc(c, k, np.n_pad, planes, st, true))) return rc;
    if (!c->order_on_device) HIP_TRY(c, hipMemcpyAsync(np.perm.p, np.perm_host.data(), sizeof(int) * (size_t)r.n, hipMemcpyHostToDevice, st));
    sas_launch_relayout(st, r.n, np.n_pad, (const int *)np.perm.p, r.means, r.quats, r.scales, r.cov6, r.opac, r.colors, coeff_floats, planes,
                        r.gid, (float4 *)np.g0.p, (float4 *)np.g1.p, (float4 *)np.g2.p, (float4 *)np.col.p, (uint8_t *)np.gid8.p);
    SasDensityState s{};
    s.perm_new = (const int *)np.perm.p; s.parents = r.parents; s.inv_old = inv_old;
    s.g0_new = (const float4 *)np.g0.p; s.g2_new = (const float4 *)np.g2.p;
    s.n_new = r.n; s.n_survivors = r.n_survivors; s.n_old = sc.n; s.n_pad_old = sc.n_pad; s.n_pad_new = np.n_pad;
    s.planes = planes;
    s.old_ = c->adam.view();
    s.new_ = na.view();
    sas_launch_density_state(st, s, r.fresh);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));

    // the context takes the new scene (the old buffers go with this scope)
    std::swap(c->planes, np);
    std::swap(c->adam, na);
    c->planes.bind(c->scene);
    scene_changed(c, Changed::CountAndOrder);
    lap(3);
    return SAS_OK;
}

// Densify, prune and re-order (sas_density.hip, sas_order.hip).  Host work: validation, one read-back (the class totals; SAS_ORDER=0: the new
// means and group ids too, for storage_order), the allocations.  Everything the new scene needs is allocated before the context changes.
int sas_scene_densify(sas_ctx *c, const sas_densify_config *cfg, const float *grad_sum, const int32_t *count, int32_t *parents_out,
                      int64_t counts_out[4], void *stream)
{
    const char *who = "sas_scene_densify";
    if (const int rc = need_scene(c, who)) return rc;
    if (const int rc = need_unskinned(c, who)) return rc;
    if (!cfg) return fail(c, SAS_ERR_INVALID, "%s: cfg is NULL", who);
    if (!grad_sum || !count || !counts_out) return fail(c, SAS_ERR_INVALID, "%s: grad_sum, count and counts_out are required", who);
    if (cfg->flags & ~(SAS_DENSIFY_GROW | SAS_DENSIFY_PRUNE_OPACITY | SAS_DENSIFY_PRUNE_SCALE))
        return fail(c, SAS_ERR_INVALID, "%s: unknown flags 0x%x", who, cfg->flags);
    for (const float t : {cfg->grow_grad2d, cfg->grow_scale3d, cfg->prune_opacity, cfg->prune_scale3d})
        if (const int rc = check_rate(c, who, "threshold", t)) return rc;
    if (!(cfg->scene_extent > 0.0f && cfg->scene_extent < INFINITY)) return fail(c, SAS_ERR_INVALID, "%s: scene_extent %g is not positive and finite", who, (double)cfg->scene_extent);
    if (!(cfg->split_factor > 1.0f && cfg->split_factor < INFINITY)) return fail(c, SAS_ERR_INVALID, "%s: split_factor %g <= 1", who, (double)cfg->split_factor);
    if (cfg->max_gaussians < 0 || cfg->max_gaussians > 0x7fffffffll) return fail(c, SAS_ERR_INVALID, "%s: max_gaussians %lld out of range", who, (long long)cfg->max_gaussians);
    if (c->scene.cov_mode && (cfg->flags & (SAS_DENSIFY_GROW | SAS_DENSIFY_PRUNE_SCALE)))
        return fail(c, SAS_ERR_INVALID, "%s: the scene was uploaded as covariances, which have no scales: only SAS_DENSIFY_PRUNE_OPACITY applies", who);
    const SasScene sc = c->scene;
    if (sc.n <= 0) return fail(c, SAS_ERR_INVALID, "%s: the scene is empty", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int coeff_floats = sas_coeff_floats(sc.sh_degree), planes = sas_colour_planes(sc.sh_degree);
    const size_t n = (size_t)sc.n, nb = (n + 255) / 256;
    int rc;
    if ((rc = ensure(c, {{c->density_inv, sizeof(int) * n}, {c->density_cls, n}, {c->density_blk, sizeof(unsigned) * (6 * nb + 4)}}))) return rc;
    SasDensity q{};
    q.g0 = sc.g0; q.g1 = sc.g1; q.g2 = sc.g2; q.col = sc.col; q.gid8 = sc.gid8; q.perm = sc.perm;
    q.inv = (int *)c->density_inv.p;
    q.n = sc.n; q.n_pad = sc.n_pad;
    q.coeff_floats = coeff_floats; q.planes = planes; q.cov_mode = sc.cov_mode;
    q.grad_sum = grad_sum; q.count = count;
    q.grow_grad2d = cfg->grow_grad2d;
    q.grow_scale = cfg->grow_scale3d * cfg->scene_extent;
    q.prune_opacity = cfg->prune_opacity;
    q.prune_scale = cfg->prune_scale3d * cfg->scene_extent;
    q.split_factor = cfg->split_factor;
    q.flags = cfg->flags; q.seed = cfg->seed;
    q.max_gaussians = cfg->max_gaussians;
    q.cls = (uint8_t *)c->density_cls.p;
    q.blk_count = (unsigned *)c->density_blk.p;
    q.blk_off = q.blk_count + 3 * nb;
    q.totals = q.blk_off + 3 * nb;
    q.nb = (long long)nb;
    Laps lap{c->densify_ms};
    sas_launch_density_classes(st, q);
    HIP_TRY(c, hipGetLastError());
    unsigned totals[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(totals, q.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const SasDensityPlan pl = sas_density_plan(totals[0], totals[1], totals[2], cfg->max_gaussians);
    if (pl.n_new <= 0) return fail(c, SAS_ERR_INVALID, "%s: every Gaussian would be pruned: refused, the scene stays", who);
    if (pl.n_new > 0x7fffffffll) return fail(c, SAS_ERR_INVALID, "%s: %lld Gaussians are out of range", who, pl.n_new);

    lap(0);
    // the new scene in the caller's order
    const size_t m = (size_t)pl.n_new;
    DevBuf a_means, a_q, a_s, a_cov, a_op, a_col, a_gid, a_par;
    if ((rc = ensure(c, {{a_means, sizeof(float) * 3 * m}, {a_op, sizeof(float) * m}, {a_col, sizeof(float) * (size_t)coeff_floats * m}}))) return rc;
    if (sc.cov_mode ? (rc = ensure(c, a_cov, sizeof(float) * 6 * m)) : ((rc = ensure(c, a_q, sizeof(float) * 4 * m)) || (rc = ensure(c, a_s, sizeof(float) * 3 * m)))) return rc;
    if (sc.n_groups > 0 && (rc = ensure(c, a_gid, m))) return rc;
    if (!parents_out && (rc = ensure(c, a_par, sizeof(int) * m))) return rc;
    q.means = (float *)a_means.p; q.quats = (float *)a_q.p; q.scales = (float *)a_s.p; q.cov6 = (float *)a_cov.p;
    q.opac = (float *)a_op.p; q.colors = (float *)a_col.p;
    q.gid = (uint8_t *)a_gid.p;
    q.parents = parents_out ? parents_out : (int *)a_par.p;
    q.n_new = pl.n_new;
    sas_launch_density_scatter(st, q);
    HIP_TRY(c, hipGetLastError());
    NewRows rows{pl.n_new, q.means, q.quats, q.scales, q.cov6, q.opac, q.colors, q.gid, q.parents, nullptr, pl.survivors};
    if ((rc = commit_rows(c, rows, q.inv, st, lap))) return rc;
    counts_out[0] = pl.n_new;
    counts_out[1] = pl.clones;
    counts_out[2] = pl.splits;
    counts_out[3] = sc.n - (long long)totals[0];
    return SAS_OK;
}

// Noise on the means (k_mcmc_noise).  Host work: validation, one launch, one event.
int sas_scene_mcmc_noise(sas_ctx *c, float scale, int step, unsigned seed, void *stream)
{
    const char *who = "sas_scene_mcmc_noise";
    if (const int rc = need_scene(c, who)) return rc;
    if (const int rc = need_unskinned(c, who)) return rc;
    if (const int rc = check_rate(c, who, "scale", scale)) return rc;
    if (step < 1) return fail(c, SAS_ERR_INVALID, "%s: step %d < 1 (the count is 1-based)", who, step);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // (no frame reads the planes while they change)
    if (c->scene.n <= 0 || scale == 0.0f) return SAS_OK;   // nothing moves: the last frame stays valid
    SasMcmcNoise q{};
    q.g0 = (float4 *)c->planes.g0.p; q.g1 = c->scene.g1; q.g2 = c->scene.g2;
    q.perm = c->scene.perm;
    q.n = c->scene.n;
    q.cov_mode = c->scene.cov_mode;
    q.scale = scale; q.seed = seed; q.step = (unsigned)step;
    hipStream_t st = (hipStream_t)stream;
    sas_launch_mcmc_noise(st, q);
    HIP_TRY(c, hipGetLastError());
    if (const int rc = slots_wait_for(c, c->density_done, st)) return rc;
    scene_changed(c, Changed::Values);
    return SAS_OK;
}

// Relocate and grow (sas_mcmc.hip).  Host work: validation, one read-back (the totals; SAS_ORDER=0: the new means and group ids too),
// the allocations, and the tail it shares with sas_scene_densify.
int sas_scene_mcmc_refine(sas_ctx *c, const sas_mcmc_config *cfg, int32_t *parents_out, int64_t counts_out[3], void *stream)
{
    const char *who = "sas_scene_mcmc_refine";
    if (const int rc = need_scene(c, who)) return rc;
    if (const int rc = need_unskinned(c, who)) return rc;
    if (!cfg || !counts_out) return fail(c, SAS_ERR_INVALID, "%s: cfg and counts_out are required", who);
    if (!(cfg->min_opacity >= 0.0f && cfg->min_opacity < 1.0f)) return fail(c, SAS_ERR_INVALID, "%s: min_opacity %g outside [0, 1)", who, (double)cfg->min_opacity);
    if (cfg->cap_max < 1 || cfg->cap_max > 0x7fffffffll - 256) return fail(c, SAS_ERR_INVALID, "%s: cap_max %lld out of range", who, (long long)cfg->cap_max);
    if (!(cfg->grow_factor >= 1.0 && cfg->grow_factor < (double)INFINITY)) return fail(c, SAS_ERR_INVALID, "%s: grow_factor %g < 1 or not finite", who, cfg->grow_factor);
    if (c->scene.cov_mode) return fail(c, SAS_ERR_INVALID, "%s: the scene was uploaded as covariances, which have no scales to relocate", who);
    const SasScene sc = c->scene;
    if (sc.n <= 0) return fail(c, SAS_ERR_INVALID, "%s: the scene is empty", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int coeff_floats = sas_coeff_floats(sc.sh_degree), planes = sas_colour_planes(sc.sh_degree);
    const size_t n = (size_t)sc.n, nb = (n + 255) / 256;
    int rc;
    // scratch: inv | weight, copies (4 n each) | prefix (8 n) | reloc (16 n) | the workgroup sums, their offsets and the totals
    if ((rc = ensure(c, {{c->density_inv, sizeof(int) * n}, {c->mcmc_u32, sizeof(unsigned) * 2 * n}, {c->mcmc_u64, sizeof(unsigned long long) * n},
                         {c->mcmc_reloc, sizeof(float4) * n}, {c->density_blk, sizeof(unsigned long long) * (3 * nb + 2)}}))) return rc;
    SasMcmc q{};
    q.g0 = sc.g0; q.g1 = sc.g1; q.g2 = sc.g2; q.col = sc.col; q.gid8 = sc.gid8;
    q.inv = (const int *)c->density_inv.p;
    q.n = sc.n; q.n_pad = sc.n_pad;
    q.coeff_floats = coeff_floats; q.planes = planes;
    q.min_opacity = cfg->min_opacity; q.seed = cfg->seed;
    q.weight = (unsigned *)c->mcmc_u32.p; q.copies = q.weight + n;
    q.prefix = (unsigned long long *)c->mcmc_u64.p;
    q.reloc = (float4 *)c->mcmc_reloc.p;
    q.blk_weight = (unsigned long long *)c->density_blk.p; q.blk_weight_off = q.blk_weight + nb; q.totals = q.blk_weight_off + nb;
    q.blk_alive = (unsigned *)(q.totals + 2); q.blk_alive_off = q.blk_alive + nb;
    q.nb = (long long)nb;
    Laps lap{c->densify_ms};
    sas_launch_density_inverse(st, sc.n, sc.perm, (int *)c->density_inv.p);
    sas_launch_mcmc_weights(st, q);
    HIP_TRY(c, hipGetLastError());
    unsigned long long totals[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(totals, q.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (totals[0] == 0 || totals[1] == 0) return fail(c, SAS_ERR_INVALID, "%s: no alive Gaussian (opacity > %g): refused, the scene stays", who, (double)cfg->min_opacity);
    const SasMcmcPlan pl = sas_mcmc_plan(sc.n, (long long)totals[0], cfg->cap_max, cfg->grow_factor);
    lap(0);
    if (pl.draws == 0) {   // nothing to do: the scene, its order and its state stay
        if (parents_out) {
            sas_launch_mcmc_identity(st, sc.n, parents_out);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(st));
        }
        for (int k = 1; k < 4; ++k) c->densify_ms[k] = 0.0f;
        counts_out[0] = sc.n; counts_out[1] = 0; counts_out[2] = 0;
        return SAS_OK;
    }
    // the new scene in the caller's order
    const size_t m = (size_t)pl.n_new;
    DevBuf a_means, a_q, a_s, a_op, a_col, a_gid, a_par, a_fresh, a_src;
    if ((rc = ensure(c, {{a_means, sizeof(float) * 3 * m}, {a_q, sizeof(float) * 4 * m}, {a_s, sizeof(float) * 3 * m}, {a_op, sizeof(float) * m},
                         {a_col, sizeof(float) * (size_t)coeff_floats * m}, {a_fresh, m}, {a_src, sizeof(int) * (size_t)pl.draws}}))) return rc;
    if (sc.n_groups > 0 && (rc = ensure(c, a_gid, m))) return rc;
    if (!parents_out && (rc = ensure(c, a_par, sizeof(int) * m))) return rc;
    q.n_alive = (long long)totals[0]; q.draws = pl.draws; q.n_new = pl.n_new;
    q.total_weight = totals[1];
    q.source = (int *)a_src.p;
    q.means = (float *)a_means.p; q.quats = (float *)a_q.p; q.scales = (float *)a_s.p; q.opac = (float *)a_op.p; q.colors = (float *)a_col.p;
    q.gid = (uint8_t *)a_gid.p;
    q.parents = parents_out ? parents_out : (int *)a_par.p;
    q.fresh = (uint8_t *)a_fresh.p;
    HIP_TRY(c, hipMemsetAsync(q.copies, 0, sizeof(unsigned) * n, st));
    sas_launch_mcmc_rows(st, q);
    HIP_TRY(c, hipGetLastError());
    NewRows rows{pl.n_new, q.means, q.quats, q.scales, nullptr, q.opac, q.colors, q.gid, q.parents, q.fresh, 0};
    if ((rc = commit_rows(c, rows, q.inv, st, lap))) return rc;
    counts_out[0] = pl.n_new;
    counts_out[1] = pl.n_dead;
    counts_out[2] = pl.n_grow;
    return SAS_OK;
}

int sas_scene_densify_times(sas_ctx *c, float *ms, int n)
{
    if (!c || !ms) return SAS_ERR_INVALID;
    for (int k = 0; k < n && k < 4; ++k) ms[k] = c->densify_ms[k];
    return SAS_OK;
}

int sas_scene_reset_opacity(sas_ctx *c, float max_opacity, void *stream)
{
    const char *who = "sas_scene_reset_opacity";
    if (const int rc = need_scene(c, who)) return rc;
    if (const int rc = need_unskinned(c, who)) return rc;
    if (!(max_opacity > 0.0f && max_opacity < 1.0f)) return fail(c, SAS_ERR_INVALID, "%s: max_opacity %g outside (0, 1)", who, (double)max_opacity);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // (no frame reads the planes while they change)
    if (c->scene.n <= 0) return SAS_OK;
    hipStream_t st = (hipStream_t)stream;
    sas_launch_opacity_reset(st, c->scene.n, max_opacity, (float4 *)c->planes.g0.p, c->adam.on[Adam::OPACITIES] ? c->adam.view().opac : nullptr);
    HIP_TRY(c, hipGetLastError());
    if (const int rc = slots_wait_for(c, c->density_done, st)) return rc;
    scene_changed(c, Changed::Values);
    return SAS_OK;
}

// The storage order of any means and group ids (device arrays), scene-free: device_order on the caller's stream.  Nothing is waited for.
int sas_storage_order(sas_ctx *c, int64_t n, const float *means, const uint8_t *group_id_or_null, int32_t *perm_out, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    if (n < 0 || n > 0x7fffffffll) return fail(c, SAS_ERR_INVALID, "sas_storage_order: n=%lld out of range", (long long)n);
    if (n == 0) return SAS_OK;
    if (!means || !perm_out) return fail(c, SAS_ERR_INVALID, "sas_storage_order: means and perm_out are required");
    HIP_TRY(c, hipSetDevice(c->device));
    return device_order(c, n, means, group_id_or_null, perm_out, (hipStream_t)stream);
}

// The k nearest other points of every point of one cloud (sas_knn.hip), scene-free, device arrays: enqueued on the caller's stream, nothing is
// waited for.  The scratch is the context's and grows with the largest call; a call on another stream than the one before runs behind it.
//   knn_rec:   [SasOrderRecord | SasKnnGrid | pad to 256 | occupancy words | partial bounds of sas_launch_order_bounds]
//   knn_table: [4 zero words | table_len cell entries | table_len / SAS_KNN_SCAN_BLOCK block sums]
int sas_knn_points(sas_ctx *c, int64_t n, const float *points, int k, float *dist2_out, int32_t *index_out_or_null, void *stream)
{
    const char *who = "sas_knn_points";
    if (!c) return SAS_ERR_INVALID;
    if (k < 1 || k > SAS_KNN_MAX_K) return fail(c, SAS_ERR_INVALID, "%s: k=%d out of [1,%d]", who, k, SAS_KNN_MAX_K);
    if (n < 0 || n > 0x7fffffffll) return fail(c, SAS_ERR_INVALID, "%s: n=%lld out of range", who, (long long)n);
    if (n == 0) return SAS_OK;
    if (!points || !dist2_out) return fail(c, SAS_ERR_INVALID, "%s: points and dist2_out are required", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t m = (size_t)n;
    const int K = k <= 3 ? 3 : SAS_KNN_MAX_K;
    SasKnn q{};
    q.points = points; q.n = n; q.k = k; q.forced_g = c->knn_grid;
    q.dist2 = dist2_out; q.index = index_out_or_null;
    q.cells_cap = std::min<long long>(SAS_KNN_MAX_CELLS, std::max<long long>(4096, 2 * (long long)n));
    q.table_len = (q.cells_cap + 1 + SAS_KNN_SCAN_BLOCK - 1) / SAS_KNN_SCAN_BLOCK * SAS_KNN_SCAN_BLOCK;
    // slices of k_knn_brute: as many as keep the slice keys within 256 MiB, 32 at most; never more than the cloud has chunks
    const long long n_chunks = (n + SAS_KNN_CHUNK - 1) / SAS_KNN_CHUNK;
    long long slices = std::min<long long>(32, std::max<long long>(1, (256ll << 20) / (long long)(sizeof(unsigned long long) * m * K)));
    slices = std::min(slices, n_chunks);
    q.slice_points = (n_chunks + slices - 1) / slices * SAS_KNN_CHUNK;
    q.slices = (int)((n + q.slice_points - 1) / q.slice_points);   // (no slice is empty)
    SasOrder b{};
    b.means = points; b.n = n; b.n_tiles = (n + SAS_ORDER_TILE - 1) / SAS_ORDER_TILE; b.n_groups = 256;
    const size_t rec_bytes = 256, occ_bytes = sizeof(unsigned) * SAS_KNN_COARSE * SAS_KNN_COARSE;
    static_assert(sizeof(SasOrderRecord) + sizeof(SasKnnGrid) <= 256, "the two records share the block's first 256 bytes");
    const size_t table_words = 4 + (size_t)q.table_len + (size_t)(q.table_len / SAS_KNN_SCAN_BLOCK);
    if (const int rc = ensure(c, {{c->knn_pts, sizeof(float4) * m}, {c->knn_table, sizeof(unsigned) * table_words}, {c->knn_left, sizeof(int) * m},
                                  {c->knn_keys, sizeof(unsigned long long) * m * (size_t)K * (size_t)q.slices},
                                  {c->knn_rec, rec_bytes + occ_bytes + sizeof(int) * SAS_ORDER_PARTIAL * (size_t)b.n_tiles}}))
        return rc;
    char *rec = (char *)c->knn_rec.p;
    b.rec = (SasOrderRecord *)rec;
    b.partial = (int *)(rec + rec_bytes + occ_bytes);
    q.bounds = b.rec;
    q.grid = (SasKnnGrid *)(rec + sizeof(SasOrderRecord));
    q.occ = (unsigned *)(rec + rec_bytes);
    q.table = (unsigned *)c->knn_table.p + 4;
    q.blk = q.table + q.table_len;
    q.pts = (float4 *)c->knn_pts.p;
    q.left = (int *)c->knn_left.p;
    q.keys = (unsigned long long *)c->knn_keys.p;
    if (!c->knn_done.h) HIP_TRY(c, hipEventCreateWithFlags(c->knn_done.put(), hipEventDisableTiming));
    else HIP_TRY(c, hipStreamWaitEvent(st, c->knn_done, 0));
    HIP_TRY(c, hipMemsetAsync(rec, 0, rec_bytes + occ_bytes, st));
    HIP_TRY(c, hipMemsetAsync(c->knn_table.p, 0, sizeof(unsigned) * table_words, st));
    sas_launch_order_bounds(st, b);
    sas_launch_knn(st, q);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->knn_done, st));
    return SAS_OK;
}

// The k nearest nodes of a second cloud for every point (k_knn_cross), scene-free, device arrays: one launch on the caller's stream, no
// scratch, nothing is waited for.
int sas_knn_cross(sas_ctx *c, int64_t n, const float *points, int64_t m, const float *nodes, int k, float max_distance, float *dist2_out,
                  int32_t *index_out_or_null, void *stream)
{
    const char *who = "sas_knn_cross";
    if (!c) return SAS_ERR_INVALID;
    if (k < 1 || k > SAS_KNN_MAX_K) return fail(c, SAS_ERR_INVALID, "%s: k=%d out of [1,%d]", who, k, SAS_KNN_MAX_K);
    if (n < 0 || n > 0x7fffffffll) return fail(c, SAS_ERR_INVALID, "%s: n=%lld out of range", who, (long long)n);
    if (m < 1 || m > SAS_KNN_CROSS_MAX_NODES) return fail(c, SAS_ERR_INVALID, "%s: m=%lld out of [1,%d]", who, (long long)m, SAS_KNN_CROSS_MAX_NODES);
    if (const int rc = check_max_distance(c, max_distance)) return rc;
    if (n == 0) return SAS_OK;
    if (!points || !nodes || !dist2_out) return fail(c, SAS_ERR_INVALID, "%s: points, nodes and dist2_out are required", who);
    HIP_TRY(c, hipSetDevice(c->device));
    const SasKnnCross q{points, nodes, n, (int)m, k, max_distance * max_distance, dist2_out, index_out_or_null};
    sas_launch_knn_cross((hipStream_t)stream, q);
    HIP_TRY(c, hipGetLastError());
    return SAS_OK;
}

// The rigidity term of a deformation graph and its gradient (k_nodes_rigidity, k_nodes_value), scene-free, device arrays, binary64: two launches
// on the caller's stream, nothing is waited for.  The partial sums of the value are the context's (2 KiB, allocated by the first call); a call
// on another stream than the one before runs behind it.
int sas_nodes_rigidity(sas_ctx *c, int64_t m, const float *nodes, const double *Rt64, int kn, const int32_t *nb, const int32_t *rev_start,
                       const int32_t *rev_edge, double *d_Rt64_out, double *value_out, void *stream)
{
    const char *who = "sas_nodes_rigidity";
    if (!c) return SAS_ERR_INVALID;
    if (m < 1 || m > SAS_KNN_CROSS_MAX_NODES) return fail(c, SAS_ERR_INVALID, "%s: m=%lld out of [1,%d]", who, (long long)m, SAS_KNN_CROSS_MAX_NODES);
    if (kn < 0 || kn > SAS_NODES_MAX_K) return fail(c, SAS_ERR_INVALID, "%s: kn=%d out of [0,%d]", who, kn, SAS_NODES_MAX_K);
    if (!nodes || !Rt64 || !d_Rt64_out || !value_out) return fail(c, SAS_ERR_INVALID, "%s: nodes, Rt64, d_Rt64_out and value_out are required", who);
    if (kn > 0 && (!nb || !rev_start || !rev_edge)) return fail(c, SAS_ERR_INVALID, "%s: nb, rev_start and rev_edge are required with kn > 0", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = ensure(c, c->nodes_partial, sizeof(double) * SAS_NODES_MAX_PARTIALS)) return rc;
    if (!c->nodes_done.h) HIP_TRY(c, hipEventCreateWithFlags(c->nodes_done.put(), hipEventDisableTiming));
    else HIP_TRY(c, hipStreamWaitEvent(st, c->nodes_done, 0));
    const SasNodesRigidity q{nodes, Rt64, nb, rev_start, rev_edge, (int)m, kn, d_Rt64_out, (double *)c->nodes_partial.p, value_out};
    sas_launch_nodes_rigidity(st, q);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->nodes_done, st));
    return SAS_OK;
}

// One Adam step of every node's se(3) twist about the node's current position (k_nodes_twist_step), scene-free, device arrays, binary64: one
// launch on the caller's stream, no scratch, nothing is waited for.
int sas_nodes_twist_step(sas_ctx *c, int64_t m, const float *nodes, const float *d_Rt32_or_null, const double *d_Rt64_or_null, double weight64,
                         double *Rt64, double *m1, double *m2, float *Rt32_out, const sas_node_step_config *cfg, void *stream)
{
    const char *who = "sas_nodes_twist_step";
    if (!c) return SAS_ERR_INVALID;
    if (m < 1 || m > SAS_KNN_CROSS_MAX_NODES) return fail(c, SAS_ERR_INVALID, "%s: m=%lld out of [1,%d]", who, (long long)m, SAS_KNN_CROSS_MAX_NODES);
    if (!cfg || !nodes || !Rt64 || !m1 || !m2 || !Rt32_out) return fail(c, SAS_ERR_INVALID, "%s: cfg, nodes, Rt64, m1, m2 and Rt32_out are required", who);
    if (!d_Rt32_or_null && !d_Rt64_or_null) return fail(c, SAS_ERR_INVALID, "%s: one of d_Rt32 and d_Rt64 is required", who);
    if (!std::isfinite(weight64)) return fail(c, SAS_ERR_INVALID, "%s: weight64 = %g is not finite", who, weight64);
    for (const double lr : {cfg->lr_rot, cfg->lr_trans})
        if (!(lr >= 0.0) || !std::isfinite(lr)) return fail(c, SAS_ERR_INVALID, "%s: rates (%g, %g) must be finite and >= 0", who, cfg->lr_rot, cfg->lr_trans);
    for (const double b : {cfg->beta1, cfg->beta2})
        if (!(b >= 0.0 && b < 1.0)) return fail(c, SAS_ERR_INVALID, "%s: betas (%g, %g) must lie in [0,1)", who, cfg->beta1, cfg->beta2);
    for (const double g : {cfg->gain1, cfg->gain2})
        if (!(g > 0.0 && g <= 1.0)) return fail(c, SAS_ERR_INVALID, "%s: gains (%g, %g) must lie in (0,1]", who, cfg->gain1, cfg->gain2);
    for (const double v : {cfg->c1, cfg->c2})
        if (!(v > 0.0) || !std::isfinite(v)) return fail(c, SAS_ERR_INVALID, "%s: c1 = %g, c2 = %g must be finite and > 0", who, cfg->c1, cfg->c2);
    if (!(cfg->eps >= 0.0) || !std::isfinite(cfg->eps)) return fail(c, SAS_ERR_INVALID, "%s: eps = %g must be finite and >= 0", who, cfg->eps);
    HIP_TRY(c, hipSetDevice(c->device));
    const SasNodesStep q{nodes, d_Rt32_or_null, d_Rt64_or_null, weight64, Rt64, m1, m2, Rt32_out, (int)m,
                         cfg->lr_rot, cfg->lr_trans, cfg->beta1, cfg->beta2, cfg->gain1, cfg->gain2, cfg->c1, cfg->c2, cfg->eps};
    sas_launch_nodes_step((hipStream_t)stream, q);
    HIP_TRY(c, hipGetLastError());
    return SAS_OK;
}

// Every node's rigid [R | t] from moved node positions (k_nodes_fit_rigid), scene-free, device arrays, binary64: one launch on the caller's
// stream, no scratch, nothing is waited for.
int sas_nodes_fit_rigid(sas_ctx *c, int steps, int64_t m, const float *nodes, const float *moved, int kn, const int32_t *nb, double *Rt64_out_or_null,
                        float *Rt32_out, void *stream)
{
    const char *who = "sas_nodes_fit_rigid";
    if (!c) return SAS_ERR_INVALID;
    if (m < 1 || m > SAS_KNN_CROSS_MAX_NODES) return fail(c, SAS_ERR_INVALID, "%s: m=%lld out of [1,%d]", who, (long long)m, SAS_KNN_CROSS_MAX_NODES);
    if (steps < 1 || (int64_t)steps * m > SAS_NODES_FIT_MAX_LANES)
        return fail(c, SAS_ERR_INVALID, "%s: steps=%d out of range (steps >= 1, steps * m <= %d)", who, steps, SAS_NODES_FIT_MAX_LANES);
    if (kn < 0 || kn > SAS_NODES_MAX_K) return fail(c, SAS_ERR_INVALID, "%s: kn=%d out of [0,%d]", who, kn, SAS_NODES_MAX_K);
    if (!nodes || !moved || !Rt32_out) return fail(c, SAS_ERR_INVALID, "%s: nodes, moved and Rt32_out are required", who);
    if (kn > 0 && !nb) return fail(c, SAS_ERR_INVALID, "%s: nb is required with kn > 0", who);
    HIP_TRY(c, hipSetDevice(c->device));
    const SasNodesFit q{nodes, moved, nb, steps, (int)m, kn, Rt64_out_or_null, Rt32_out};
    sas_launch_nodes_fit((hipStream_t)stream, q);
    HIP_TRY(c, hipGetLastError());
    return SAS_OK;
}

// Bind, replace or clear the skin (k_skin_bind).  Host work: validation, the planes' allocations, the rest snapshot as device copies on the
// caller's stream, one launch, one event.
int sas_scene_skin(sas_ctx *c, int k, const int32_t *indices, const float *weights, void *stream)
{
    const char *who = "sas_scene_skin";
    if (const int rc = need_scene(c, who)) return rc;
    if (k < 0 || k > SAS_SKIN_MAX_K) return fail(c, SAS_ERR_INVALID, "%s: k=%d out of [0,%d]", who, k, SAS_SKIN_MAX_K);
    const SasScene &sc = c->scene;
    if (k > 0 && sc.n > 0 && (!indices || !weights)) return fail(c, SAS_ERR_INVALID, "%s: indices and weights are required", who);
    Skin &sk = c->skin;
    if (k == 0 && !sk.bound()) return SAS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // (no frame reads the planes while they change)
    hipStream_t st = (hipStream_t)stream;
    Planes &pl = c->planes;
    const size_t np = (size_t)(pl.n_pad > 0 ? pl.n_pad : 64), plane = sizeof(float4) * np;
    DevBuf *rest[3] = {&sk.rest0, &sk.rest1, &sk.rest2}, *live[3] = {&pl.g0, &pl.g1, &pl.g2};
    if (k == 0) {   // the rest planes back, bit for bit
        for (int p = 0; p < 3; ++p) HIP_TRY(c, hipMemcpyAsync(live[p]->p, rest[p]->p, plane, hipMemcpyDeviceToDevice, st));
        sk.k = sk.m = 0;
        if (const int rc = slots_wait_for(c, c->skin_done, st)) return rc;
        scene_changed(c, Changed::Values);
        return SAS_OK;
    }
    const int kp = k <= 4 ? 4 : SAS_SKIN_MAX_K;
    if (const int rc = ensure(c, {{sk.idx, plane * (kp / 4)}, {sk.w, plane * (kp / 4)}})) return rc;
    if (!sk.bound()) {   // the first bind: what the planes hold now is the rest pose
        if (const int rc = ensure(c, {{sk.rest0, plane}, {sk.rest1, plane}, {sk.rest2, plane}})) return rc;
        for (int p = 0; p < 3; ++p) HIP_TRY(c, hipMemcpyAsync(rest[p]->p, live[p]->p, plane, hipMemcpyDeviceToDevice, st));
    }
    const SasSkinBind q{sc.perm, indices, weights, sc.n, pl.n_pad, k, kp, (int4 *)sk.idx.p, (float4 *)sk.w.p};
    sas_launch_skin_bind(st, q);
    HIP_TRY(c, hipGetLastError());
    sk.k = k;
    sk.m = 0;   // (the records belong to the entries before)
    return slots_wait_for(c, c->skin_done, st);   // (the planes' values stay: the last frame does too)
}

// The binding in the caller's order (k_skin_read), on the context's own stream; host or device destinations.  Blocking.
int sas_scene_skin_read(sas_ctx *c, int32_t *indices_out, float *weights_out)
{
    const char *who = "sas_scene_skin_read";
    if (const int rc = need_scene(c, who)) return rc;
    const Skin &sk = c->skin;
    if (!sk.bound()) return fail(c, SAS_ERR_INVALID, "%s: no skin is bound", who);
    if (!indices_out || !weights_out) return fail(c, SAS_ERR_INVALID, "%s: indices_out and weights_out are required", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    const SasScene &sc = c->scene;
    const size_t count = (size_t)sc.n * (size_t)sk.k;
    if (count == 0) return SAS_OK;
    DevBuf s_idx, s_w;
    if (const int rc = ensure(c, {{s_idx, sizeof(int) * count}, {s_w, sizeof(float) * count}})) return rc;
    HIP_TRY(c, hipDeviceSynchronize());   // (the bind ran on the caller's stream)
    const SasSkinRead q{sc.perm, (const int4 *)sk.idx.p, (const float4 *)sk.w.p, sc.n, sc.n_pad, sk.k, (int *)s_idx.p, (float *)s_w.p};
    hipStream_t st = c->slots[0].fs;
    sas_launch_skin_read(st, q);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipMemcpy(indices_out, s_idx.p, sizeof(int) * count, hipMemcpyDefault));
    HIP_TRY(c, hipMemcpy(weights_out, s_w.p, sizeof(float) * count, hipMemcpyDefault));
    return SAS_OK;
}

// What the deformation and its adjoints read of the bound skin, with m node records: the fields the three calls share.  (They are fields of
// each call and not one embedded record: the kernels take their arguments where the calls had them.)
static const auto skin_view = [](auto &q, const sas_ctx *c, int m) {   // (a generic lambda: no template may stand in this extern "C" block)
    const Skin &sk = c->skin;
    q.nodes = (SasSkinNode *)sk.nodes.p;
    q.idx = (const int4 *)sk.idx.p; q.w = (const float4 *)sk.w.p;
    q.n = c->scene.n; q.n_pad = c->scene.n_pad;
    q.m = m; q.kp = sk.kp();
};
// ... and the upstream gradients of the two adjoints, in the caller's order
static const auto skin_grads = [](auto &q, const sas_ctx *c, const float *d_means, const float *d_quats, const float *d_cov6) {
    q.perm = c->scene.perm;
    q.d_means = d_means; q.d_quats = d_quats; q.d_cov6 = d_cov6;
};

// k_deform's call on the bound skin with m node records: rest planes -> live planes.
static SasDeform deform_call(sas_ctx *c, int m)
{
    const Skin &sk = c->skin;
    SasDeform q{};
    skin_view(q, c, m);
    q.r0 = (const float4 *)sk.rest0.p; q.r1 = (const float4 *)sk.rest1.p; q.r2 = (const float4 *)sk.rest2.p;
    q.g0 = (float4 *)c->planes.g0.p; q.g1 = (float4 *)c->planes.g1.p; q.g2 = (float4 *)c->planes.g2.p;
    q.cov_mode = c->scene.cov_mode;
    q.lds = sizeof(SasSkinNode) * (size_t)m <= (size_t)c->skin_lds;
    return q;
}

// What both adjoints of the last sas_scene_deform refuse alike, in this order; flags: the caller's, of which it knows the bits `known`.
static int deform_backward_checks(sas_ctx *c, const char *who, const float *d_means, const float *d_quats, const float *d_cov6, unsigned flags = 0,
                                  unsigned known = 0)
{
    if (const int rc = need_scene(c, who)) return rc;
    const Skin &sk = c->skin;
    if (!sk.bound()) return fail(c, SAS_ERR_INVALID, "%s: no skin is bound: sas_scene_skin first", who);
    if (sk.m <= 0) return fail(c, SAS_ERR_INVALID, "%s: no sas_scene_deform since the skin was bound", who);
    if (flags & ~known) return fail(c, SAS_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
    if (!d_means && !d_quats && !d_cov6) return fail(c, SAS_ERR_INVALID, "%s: d_means, d_quats and d_cov6 are all NULL", who);
    const SasScene &sc = c->scene;
    if (sc.cov_mode ? d_quats != nullptr : d_cov6 != nullptr)
        return fail(c, SAS_ERR_INVALID, "%s: the scene was uploaded as %s: %s must be NULL", who, sc.cov_mode ? "covariances" : "quaternions",
                    sc.cov_mode ? "d_quats" : "d_cov6");
    return SAS_OK;
}

// The live planes again from rest planes that have changed (sas_scene_adam_step_rest): the last deformation from the node records it left on
// the device (k_deform alone), or, without a sas_scene_deform since the bind, the rest planes as they are.
static int redeform(sas_ctx *c, hipStream_t st)
{
    const Skin &sk = c->skin;
    if (sk.m > 0) {
        sas_launch_deform_planes(st, deform_call(c, sk.m));
        HIP_TRY(c, hipGetLastError());
        return SAS_OK;
    }
    const Planes &pl = c->planes;
    const size_t plane = sizeof(float4) * (size_t)(pl.n_pad > 0 ? pl.n_pad : 64);
    const DevBuf *rest[3] = {&sk.rest0, &sk.rest1, &sk.rest2}, *live[3] = {&pl.g0, &pl.g1, &pl.g2};
    for (int p = 0; p < 3; ++p) HIP_TRY(c, hipMemcpyAsync(live[p]->p, rest[p]->p, plane, hipMemcpyDeviceToDevice, st));
    return SAS_OK;
}

// Move the skinned scene to the nodes' transforms (k_skin_nodes, k_deform): always rest -> current.  Host work: validation, the node
// records' buffer (grown by the first call at a larger m), two launches, one event.
int sas_scene_deform(sas_ctx *c, int m, const float *node_Rt, void *stream)
{
    const char *who = "sas_scene_deform";
    if (const int rc = need_scene(c, who)) return rc;
    Skin &sk = c->skin;
    if (!sk.bound()) return fail(c, SAS_ERR_INVALID, "%s: no skin is bound: sas_scene_skin first", who);
    if (m < 1 || m > SAS_KNN_CROSS_MAX_NODES) return fail(c, SAS_ERR_INVALID, "%s: m=%d out of [1,%d]", who, m, SAS_KNN_CROSS_MAX_NODES);
    if (!node_Rt) return fail(c, SAS_ERR_INVALID, "%s: node_Rt is NULL", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;   // (no frame reads the planes while they change)
    const SasScene &sc = c->scene;
    if (sc.n <= 0) return SAS_OK;
    if (const int rc = ensure(c, sk.nodes, sizeof(SasSkinNode) * (size_t)m)) return rc;
    hipStream_t st = (hipStream_t)stream;
    SasDeform q = deform_call(c, m);
    q.node_Rt = node_Rt;
    sas_launch_deform(st, q);
    HIP_TRY(c, hipGetLastError());
    sk.m = m;
    if (const int rc = slots_wait_for(c, c->skin_done, st)) return rc;
    scene_changed(c, Changed::Values);   // the last frame showed the scene before the deformation
    return SAS_OK;
}

// The adjoint of the last sas_scene_deform (k_deform_grad, k_skin_nodes_grad).  Host work: validation, the accumulator (grown by the first call at
// a larger m), two stream waits, one memset, two launches, one event.  No host synchronisation.
int sas_scene_deform_backward(sas_ctx *c, const float *d_means, const float *d_quats, const float *d_cov6, float *d_node_Rt, void *stream)
{
    const char *who = "sas_scene_deform_backward";
    if (const int rc = deform_backward_checks(c, who, d_means, d_quats, d_cov6)) return rc;
    Skin &sk = c->skin;
    const SasScene &sc = c->scene;
    if (!d_node_Rt) return fail(c, SAS_ERR_INVALID, "%s: d_node_Rt is NULL", who);
    HIP_TRY(c, hipSetDevice(c->device));
    const int m = sk.m;
    const size_t acc_bytes = sizeof(float) * SAS_SKIN_GRAD_ROW * (size_t)m;
    if (const int rc = ensure(c, sk.grad_acc, acc_bytes)) return rc;
    if (c->match_cus <= 0) {
        HIP_TRY(c, hipDeviceGetAttribute(&c->match_cus, hipDeviceAttributeMultiprocessorCount, c->device));
        if (c->match_cus <= 0) c->match_cus = 1;
    }
    hipStream_t st = (hipStream_t)stream;
    SasDeformGrad q{};
    skin_grads(q, c, d_means, d_quats, d_cov6);
    skin_view(q, c, m);
    q.r0 = (const float4 *)sk.rest0.p; q.r1 = (const float4 *)sk.rest1.p; q.r2 = (const float4 *)sk.rest2.p;
    q.cov_mode = sc.cov_mode;
    q.lds = acc_bytes <= (size_t)c->skin_grad_lds;
    q.staged = c->skin_grad_staged >= 0 ? c->skin_grad_staged : (!q.lds || acc_bytes <= SAS_SKIN_GRAD_STAGED_LDS_BYTES);
    // a persistent grid: as many workgroups per CU as their LDS allows, 4 at the most
    const size_t lds_bytes = sas_deform_grad_lds_bytes(m, q.lds != 0, q.staged != 0);
    const long long per_cu = std::max<long long>(1, std::min<long long>(4, lds_bytes ? (160 * 1024) / (long long)lds_bytes : 4));
    q.blocks = (int)std::max<long long>(1, std::min<long long>((sc.n + 255) / 256, per_cu * c->match_cus));
    q.acc = (float *)sk.grad_acc.p;
    q.out = d_node_Rt;
    // behind the deformation whose records are read, and behind the call before, whose accumulator this is
    if (c->skin_done.h) HIP_TRY(c, hipStreamWaitEvent(st, c->skin_done, 0));
    if (!c->skin_grad_done.h) HIP_TRY(c, hipEventCreateWithFlags(c->skin_grad_done.put(), hipEventDisableTiming));
    else HIP_TRY(c, hipStreamWaitEvent(st, c->skin_grad_done, 0));
    HIP_TRY(c, hipMemsetAsync(q.acc, 0, acc_bytes, st));
    sas_launch_deform_grad(st, q);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->skin_grad_done, st));
    return SAS_OK;
}

// The adjoint of the last sas_scene_deform to the REST arrays (k_deform_rest_grad), added to the caller's arrays.  Host work: validation, one
// stream wait, one launch.  No host synchronisation.
int sas_scene_deform_backward_rest(sas_ctx *c, const float *d_means, const float *d_quats, const float *d_cov6, float *d_rest_means,
                                   float *d_rest_quats, float *d_rest_cov6, unsigned flags, void *stream)
{
    const char *who = "sas_scene_deform_backward_rest";
    if (const int rc = deform_backward_checks(c, who, d_means, d_quats, d_cov6, flags, SAS_DEFORM_REST_BOUND_ONLY)) return rc;
    const Skin &sk = c->skin;
    const SasScene &sc = c->scene;
    struct Pair { const char *name; const float *in; float *out; int width; };
    const Pair pairs[3] = {{"means", d_means, d_rest_means, 3}, {"quats", d_quats, d_rest_quats, 4}, {"cov6", d_cov6, d_rest_cov6, 6}};
    for (const Pair &p : pairs)
        if ((p.in != nullptr) != (p.out != nullptr))
            return fail(c, SAS_ERR_INVALID, "%s: d_%s and d_rest_%s go together: one is NULL and the other is not", who, p.name, p.name);
    // every lane reads its inputs and adds to its outputs while other lanes do the same: no output may overlap an input or another output
    auto overlap = [&](const float *a, int wa, const float *b, int wb) {
        const uintptr_t a0 = (uintptr_t)a, a1 = a0 + sizeof(float) * (size_t)wa * (size_t)sc.n, b0 = (uintptr_t)b, b1 = b0 + sizeof(float) * (size_t)wb * (size_t)sc.n;
        return a && b && a0 < b1 && b0 < a1;
    };
    for (int o = 0; o < 3; ++o)
        for (int k = 0; k < 3; ++k)
            if (overlap(pairs[o].out, pairs[o].width, pairs[k].in, pairs[k].width) ||
                (k != o && overlap(pairs[o].out, pairs[o].width, pairs[k].out, pairs[k].width)))
                return fail(c, SAS_ERR_INVALID, "%s: d_rest_%s overlaps d_%s%s: the call adds to its outputs, in place it has no meaning", who,
                            pairs[o].name, overlap(pairs[o].out, pairs[o].width, pairs[k].in, pairs[k].width) ? "" : "rest_", pairs[k].name);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    SasDeformRestGrad q{};
    skin_grads(q, c, d_means, d_quats, d_cov6);
    skin_view(q, c, sk.m);
    q.lds = sizeof(SasSkinNode) * (size_t)sk.m <= (size_t)c->skin_lds;
    q.bound_only = (flags & SAS_DEFORM_REST_BOUND_ONLY) != 0;
    q.o_means = d_rest_means; q.o_quats = d_rest_quats; q.o_cov6 = d_rest_cov6;
    if (c->skin_done.h) HIP_TRY(c, hipStreamWaitEvent(st, c->skin_done, 0));   // behind the deformation whose records are read
    sas_launch_deform_rest_grad(st, q);
    HIP_TRY(c, hipGetLastError());
    return SAS_OK;
}

// What the last sas_knn_points decided on the device, once its work is done (blocking): out[0] points the ring search handed to the brute-force
// kernel (the whole cloud without a grid: out[4] = 1), out[1..3] the grid's cells per axis, out[5], out[6] the occupied 32^3 / 16^3 coarse cells.
int sas_knn_last_counts(sas_ctx *c, int64_t *out, int n)
{
    if (!c || !out) return SAS_ERR_INVALID;
    SasKnnGrid G{};
    G.n[0] = G.n[1] = G.n[2] = 0;
    if (c->knn_rec.p) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipDeviceSynchronize());
        HIP_TRY(c, hipMemcpy(&G, (const char *)c->knn_rec.p + sizeof(SasOrderRecord), sizeof(G), hipMemcpyDeviceToHost));
    }
    const int64_t v[7] = {(int64_t)G.left_count, G.n[0], G.n[1], G.n[2], G.brute, G.occupied[0], G.occupied[1]};
    for (int k = 0; k < n && k < 7; ++k) out[k] = v[k];
    return SAS_OK;
}

// The resident scene's permutation (slot -> caller's index), behind everything in flight; host or device destination.
int sas_scene_order(sas_ctx *c, int32_t *perm_out)
{
    const char *who = "sas_scene_order";
    if (const int rc = need_scene(c, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    if (c->scene.n == 0) return SAS_OK;
    if (!perm_out) return fail(c, SAS_ERR_INVALID, "%s: perm_out is NULL", who);
    HIP_TRY(c, hipDeviceSynchronize());   // (optimiser steps and density calls run on the caller's streams)
    HIP_TRY(c, hipMemcpy(perm_out, c->planes.perm.p, sizeof(int32_t) * (size_t)c->scene.n, hipMemcpyDefault));
    return SAS_OK;
}

// The planes back in the caller's order (k_scene_gather), on the context's own stream, which runs behind every optimiser step.
int sas_scene_read(sas_ctx *c, float *means, float *quats, float *scales, float *cov6, float *opacities, float *colors)
{
    const char *who = "sas_scene_read";
    if (const int rc = need_scene(c, who)) return rc;
    if (const int rc = check_form(c, who, quats || scales, cov6 != nullptr, "")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    const SasScene &sc = c->scene;
    const size_t n = (size_t)sc.n;
    if (n == 0) return SAS_OK;
    const int coeff_floats = sas_coeff_floats(sc.sh_degree);
    float *user[6] = {means, quats, scales, cov6, opacities, colors};
    const size_t floats[6] = {3 * n, 4 * n, 3 * n, 6 * n, n, (size_t)coeff_floats * n};
    float *dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf stage[6];
    for (int k = 0; k < 6; ++k) {   // a device array of this context's device is written in place, anything else through a staging buffer
        if (!user[k]) continue;
        hipPointerAttribute_t at{};
        const bool on_device = hipPointerGetAttributes(&at, user[k]) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == c->device;
        (void)hipGetLastError();
        if (on_device) { dev[k] = user[k]; continue; }
        if (const int rc = ensure(c, stage[k], sizeof(float) * floats[k])) return rc;
        dev[k] = (float *)stage[k].p;
    }
    const SasGather q{sc.g0, sc.g1, sc.g2, sc.col, sc.perm, sc.n, sc.n_pad, coeff_floats, sas_colour_planes(sc.sh_degree),
                      dev[0], dev[1], dev[2], dev[3], dev[4], dev[5]};
    hipStream_t st = c->slots[0].fs;
    sas_launch_scene_gather(st, q);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int k = 0; k < 6; ++k)
        if (user[k] && dev[k] != user[k]) HIP_TRY(c, hipMemcpy(user[k], dev[k], sizeof(float) * floats[k], hipMemcpyDefault));
    return SAS_OK;
}

static int render_batch_host_impl(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height,
                                  const float *background, unsigned flags, uint8_t *rgb8_host, void *stream, const PoseSets &ps)
{
    if (!c) return SAS_ERR_INVALID;
    if (!rgb8_host || (flags & SAS_ASYNC)) return fail(c, SAS_ERR_INVALID, "sas_render_batch_host: host buffer required, blocking only");
    flags = frame_flags(c, flags);
    if (n_views <= 0) return n_views == 0 ? SAS_OK : fail(c, SAS_ERR_INVALID, "bad view batch");
    if (width <= 0 || height <= 0) return fail(c, SAS_ERR_INVALID, "bad image size");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->inflight > 0) {   // the staging buffer below may still be the target of frames in flight
        if (const int rc = complete_all(c)) return rc;
    }
    const size_t frame_bytes = 3 * (size_t)width * (size_t)height;
    c->host_query_base = nullptr;
    c->host_query_ok = kernel_can_write_host(c, rgb8_host);
    c->host_query_base = rgb8_host;   // the answer holds for this call's views
    c->host_query_end = rgb8_host + frame_bytes * (size_t)n_views;
    // the staging frames are needed only when the tile kernel cannot deliver every frame itself
    bool all_direct = true;
    for (int v = 0; v < n_views; ++v) all_direct = all_direct && host_direct_ok(c, rgb8_host + frame_bytes * v, width, height, flags);
    int rc = (all_direct && c->host_stage.p) ? SAS_OK : ensure(c, c->host_stage, frame_bytes * (size_t)n_views);
    if (!rc)
        rc = render_batch_impl(c, n_views, viewmats, Ks, width, height, background, flags, nullptr, nullptr, nullptr,
                               (uint8_t *)c->host_stage.p, rgb8_host, stream, ps);
    c->host_query_base = nullptr;
    return rc;
}

int sas_render_batch_host(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, int width, int height,
                          const float *background, unsigned flags, uint8_t *rgb8_host, void *stream)
{
    return render_batch_host_impl(c, n_views, viewmats, Ks, width, height, background, flags, rgb8_host, stream, PoseSets());
}

int sas_render_batch_host_posed(sas_ctx *c, int n_views, const float *viewmats, const float *Ks, const int *pose_set, int n_sets,
                                const float *Rt, int width, int height, const float *background, unsigned flags,
                                uint8_t *rgb8_host, void *stream)
{
    const PoseSets ps = {pose_set, n_sets, Rt};
    if (!Rt) return fail(c, SAS_ERR_INVALID, "sas_render_batch_host_posed: Rt is required");
    return render_batch_host_impl(c, n_views, viewmats, Ks, width, height, background, flags, rgb8_host, stream, ps);
}

int sas_render_cameras_host(sas_ctx *c, int n_views, const double *wxyz, const double *position, double fov, int width,
                            int height, const float *background, unsigned flags, uint8_t *rgb8_host, void *stream)
{
    if (!c) return SAS_ERR_INVALID;
    if (n_views <= 0) return n_views == 0 ? SAS_OK : fail(c, SAS_ERR_INVALID, "bad view batch");
    if (!wxyz || !position || !(fov > 0.0)) return fail(c, SAS_ERR_INVALID, "camera poses and a positive field of view are required");
    std::vector<float> V((size_t)16 * n_views), K((size_t)9 * n_views);
    sas_camera_matrices(n_views, wxyz, position, fov, width, height, V.data(), K.data());
    return render_batch_host_impl(c, n_views, V.data(), K.data(), width, height, background, flags, rgb8_host, stream, PoseSets());
}

int sas_wait(sas_ctx *c)
{
    if (!c) return SAS_ERR_INVALID;
    if (c->inflight <= 0) return SAS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return complete_all(c);
}

int sas_frames_completed(sas_ctx *c, int64_t *submitted, int64_t *completed)
{
    if (!c) return SAS_ERR_INVALID;
    if (submitted) *submitted = c->frames_submitted;
    if (completed) *completed = c->frames_completed;
    return SAS_OK;
}

#ifdef SAS_DEBUG_BOUNDS
// every kernel file's counter (SAS_BOUNDS_ACCESSOR in sas_device.h): one line per file, in the order their reports are looked at
#define SAS_BOUNDS_FILES(X) X(kernels) X(tiles) X(mesh) X(query) X(match) X(cloud) X(fuse) X(grad) X(fit) X(loss) X(density) X(mcmc) X(order) X(knn) X(skin) X(nodes)
#define SAS_BOUNDS_DECLARE(name) extern "C" int sas_debug_bounds_##name(unsigned long long *out, int reset);
#define SAS_BOUNDS_ENTRY(name) sas_debug_bounds_##name,
SAS_BOUNDS_FILES(SAS_BOUNDS_DECLARE)
/* Bounds-checked build only: out[0] = guarded accesses found out of range since the last reset (they were
 * skipped, not executed), out[1..3] = code, index and limit of the first one (0 if none): the first file's that has a report. */
int sas_debug_bounds(unsigned long long *out, int reset)
{
    int (*const files[])(unsigned long long *, int) = {SAS_BOUNDS_FILES(SAS_BOUNDS_ENTRY)};
    if (hipDeviceSynchronize() != hipSuccess) return SAS_ERR_HIP;
    unsigned long long sum = 0, first[4] = {0, 0, 0, 0};
    for (const auto file : files) {
        unsigned long long w[4] = {0, 0, 0, 0};
        if (file(w, reset)) return SAS_ERR_HIP;
        if (w[0] && !first[0]) std::copy(w, w + 4, first);
        sum += w[0];
    }
    out[0] = sum;
    std::copy(first + 1, first + 4, out + 1);
    return SAS_OK;
}
#endif

int sas_stage_times(sas_ctx *c, float *ms, int n)
{
    if (!c || !ms) return SAS_ERR_INVALID;
    for (int k = 0; k < n && k < SAS_T_COUNT; ++k) ms[k] = c->stage_ms[k];
    return SAS_OK;
}

int sas_stage_time_means(sas_ctx *c, float *ms, int n, int64_t *frames, int reset)
{
    if (!c || !ms) return SAS_ERR_INVALID;
    for (int k = 0; k < n && k < SAS_T_COUNT; ++k)
        ms[k] = c->stage_frames > 0 ? (float)(c->stage_sum[k] / (double)c->stage_frames) : 0.0f;
    if (frames) *frames = c->stage_frames;
    if (reset) {
        for (double &v : c->stage_sum) v = 0.0;
        c->stage_frames = 0;
    }
    return SAS_OK;
}

int sas_frame_stats(sas_ctx *c, int64_t *stats, int n)
{
    if (!c || !stats) return SAS_ERR_INVALID;
    for (int k = 0; k < n && k < SAS_S_COUNT; ++k) stats[k] = c->stats[k];
    return SAS_OK;
}

int sas_read_projection(sas_ctx *c, int32_t *radii, float *means2d, float *depths, float *conics, float *colors)
{
    if (!c) return SAS_ERR_INVALID;
    if (!has(c, HAVE_SCENE) || !c->has_frame) return fail(c, SAS_ERR_NO_SCENE, "no frame rendered");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    Slot &ls = c->slots[c->last_slot];
    const int64_t n = c->scene.n;
    if (!ls.info_kept && n > 0) {
        // Single-pass product frames do not write info[] (rectangles, radii: nothing on the device reads them).  The hook
        // projects the slot's frame once more with it -- same camera, same pose snapshot, the slot's own scratch; that
        // launch bins again, so the slot's counters are cleared in front of its next frame.
        Slot *mem[1] = {&ls};
        enqueue_poses(c, mem, 1, ls.fs);   // (a pair's follower never uploaded its own copy of the snapshot)
        sas_launch_project(ls.fs, c->scene, ls.params, frame_of(c, ls, true));
        HIP_TRY(c, hipStreamSynchronize(ls.fs));
        ls.scr.counters_zero = false;
    }
    const Scratch &q = ls.scr;
    std::vector<float> rec((size_t)8 * n), col((size_t)4 * n);
    std::vector<uint32_t> info((size_t)4 * n);
    if (n > 0) {
        HIP_TRY(c, hipMemcpy(rec.data(), q.rec.p, sizeof(float) * 8 * n, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(col.data(), q.col.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(info.data(), q.info.p, sizeof(uint32_t) * 4 * n, hipMemcpyDeviceToHost));
    }
    const int *perm = nullptr;
    if (const int rc = c->planes.host_perm(c, &perm)) return rc;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t i = perm[(size_t)j];   // slot j holds the caller's Gaussian i
        const uint32_t rx = info[4 * j + 2], ry = info[4 * j + 3];   // radii: 32 bits each
        const bool vis = rx != 0;
        const float *r = &rec[8 * j], *cl = &col[4 * j];
        if (radii) {
            radii[2 * i] = vis ? (int32_t)rx : 0;
            radii[2 * i + 1] = vis ? (int32_t)ry : 0;
        }
        if (means2d) { means2d[2 * i] = vis ? r[0] : 0.f; means2d[2 * i + 1] = vis ? r[1] : 0.f; }
        if (depths) depths[i] = vis ? r[7] : 0.f;
        if (conics) { conics[3 * i] = vis ? r[2] : 0.f; conics[3 * i + 1] = vis ? r[3] : 0.f; conics[3 * i + 2] = vis ? r[4] : 0.f; }
        if (colors) { colors[3 * i] = vis ? cl[0] : 0.f; colors[3 * i + 1] = vis ? cl[1] : 0.f; colors[3 * i + 2] = vis ? cl[2] : 0.f; }
    }
    return SAS_OK;
}

int sas_read_tile_lists(sas_ctx *c, int32_t *tile_offsets, int32_t *sorted_ids, int64_t cap)
{
    if (!c) return SAS_ERR_INVALID;
    if (!has(c, HAVE_SCENE) || !c->has_frame) return fail(c, SAS_ERR_NO_SCENE, "no frame rendered");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = complete_all(c)) return rc;
    const Slot &ls = c->slots[c->last_slot];
    const Scratch &q = ls.scr;
    const int tiles = tiles_of(ls);
    if (tile_offsets)
        HIP_TRY(c, hipMemcpy(tile_offsets, q.tilebuf.p, sizeof(int) * (size_t)(tiles + 1), hipMemcpyDeviceToHost));
    if (sorted_ids) {
        int64_t m = c->stats[SAS_S_NISECT];
        if (m > cap) m = cap;
        if (m > q.cap) m = q.cap;
        if (m > 0) HIP_TRY(c, hipMemcpy(sorted_ids, q.ids.p, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost));
        const int *perm = nullptr;
        if (const int rc = c->planes.host_perm(c, &perm)) return rc;
        for (int64_t k = 0; k < m; ++k) {   // storage slots -> caller indices
            const int j = sorted_ids[k];
            sorted_ids[k] = (j >= 0 && j < c->scene.n) ? perm[(size_t)j] : -1;
        }
    }
    return SAS_OK;
}

}  // extern "C"
