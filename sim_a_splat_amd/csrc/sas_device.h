// sas_device.h -- device-side helpers shared by sas_kernels.hip, sas_tile.hip, sas_mesh.hip, sas_query.hip, sas_match.hip, sas_cloud.hip, sas_fuse.hip, sas_grad.hip, sas_fit.hip, sas_loss.hip, sas_density.hip, sas_mcmc.hip, sas_order.hip, sas_knn.hip, sas_skin.hip and sas_nodes.hip: arithmetic, the bounds-checked build, DPP reductions and row sums, contract T6 per pair, and the start of a workgroup on one tile of a frame (pixel layout, pixel state, the tile's list, the truncated-list rule).
// Everything here follows the arithmetic contract of DESIGN.md: IEEE binary32 operations, fused
// only where fma_() is written (translation units are built with -ffp-contract=off).
#pragma once
#include "sas_internal.h"

#pragma clang fp contract(off)

#define DEV __device__ __forceinline__

constexpr float kNear = 0.01f, kFar = 1e10f, kEps2d = 0.3f;
constexpr float kAlphaThr = 1.0f / 255.0f, kMaxAlpha = 0.999f, kTStop = 1e-4f;

DEV float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// Contract T2 (round 5): a colour is FINITE when it leaves the projection: clamped to +-FLT_MAX (the identity on every finite value; a
// NaN becomes -FLT_MAX).  The compositing loop adds every staged entry to every pixel of its block with weight +0 where the entry is
// skipped -- exact for finite colours, but 0 * Inf = NaN would spread one bad SH coefficient over whole blocks.  The feature store
// (sas_scene_features) maps its channels the same way.
DEV float finite_colour(float v) { return fminf(fmaxf(v, -3.402823466e38f), 3.402823466e38f); }
// set bits of m below this lane's position (v_mbcnt_lo/hi: two instructions; hipcc does not form them from
// __popcll(m & lanes_below))
DEV unsigned mbcnt64(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }

// ---- bounds-checked build (-DSAS_DEBUG_BOUNDS; GPU AddressSanitizer is not available on this pool) ----------
// SAS_IN(i, n, code) is `true` in the product build.  In the debug build it tests 0 <= i < n; a violation
// is counted, its code and values are kept, and the guarded access is SKIPPED (no fault, the run goes on):
// `if (SAS_IN(pos, cap, 12)) keys[pos] = key;`.  Read back through sas_debug_bounds() (sas_api.cpp).
#ifdef SAS_DEBUG_BOUNDS
static __device__ unsigned long long g_sas_bounds[4];   // [0] violations [1] first code [2] first index [3] first limit (per translation unit)
DEV bool sas_in_bounds(long long i, long long n, int code)
{
    if (i >= 0 && i < n) return true;
    if (atomicAdd(&g_sas_bounds[0], 1ull) == 0ull) {
        g_sas_bounds[1] = (unsigned long long)code;
        g_sas_bounds[2] = (unsigned long long)i;
        g_sas_bounds[3] = (unsigned long long)n;
    }
    return false;
}
#define SAS_IN(i, n, code) sas_in_bounds((long long)(i), (long long)(n), (code))
#define SAS_BOUNDS_ACCESSOR(name)                                                                              \
    extern "C" int name(unsigned long long *out, int reset)                                                    \
    {                                                                                                          \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sas_bounds), sizeof(g_sas_bounds)) != hipSuccess) return -1; \
        unsigned long long z[4] = {0, 0, 0, 0};                                                                \
        if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_sas_bounds), z, sizeof(z)) != hipSuccess) return -1;       \
        return 0;                                                                                              \
    }
#else
#define SAS_IN(i, n, code) true
#define SAS_BOUNDS_ACCESSOR(name)
#endif

// 16-byte non-temporal (streaming) load
DEV float4 nt_load(const float4 *p)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// The inverse activations of the optimiser's raw variables (sas_fit.hip, sas_density.hip): logit(opacity) and log(scale).  NaN marks a
// value outside the domain -- an opacity outside (0, 1), a scale that is no positive finite number: that variable stays fixed.
DEV float raw_opacity(float o) { return (o > 0.0f && o < 1.0f) ? logf(o / (1.0f - o)) : NAN; }
DEV float raw_scale(float s) { return (s > 0.0f && s < INFINITY) ? logf(s) : NAN; }

// ---- the counter-based generator (sas_density.hip, sas_mcmc.hip) ------------------------------------------------------------
// Stateless: a 32-bit integer hash (two xorshift-multiply rounds) of the key, two hashes per normal, Box-Muller.  `base` is the hash of
// everything in the key but the counter `c` (even: the normal uses c + 1 and c + 2).
DEV unsigned mix32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
DEV float hashed_normal(unsigned base, unsigned c)
{
    const unsigned h1 = mix32(base ^ ((c + 1u) * 0x9e3779b9u)), h2 = mix32(base ^ ((c + 2u) * 0x9e3779b9u));
    const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-8f;   // (0, 1], a multiple of 2^-24
    const float u2 = (float)(h2 >> 8) * 5.9604644775390625e-8f;          // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

// ---- nearest-neighbour keys (sas_knn.hip, sas_skin.hip; DESIGN.md 3, "Scene from points") -----------------------------------------------
// A candidate j at squared distance d2 is the key bits(d2) << 32 | j: smaller is nearer, ties go to the lower index.
constexpr unsigned long long kKnnNone = (0x7f800000ull << 32) | 0xffffffffull;   // d2 = +inf: above the key of every neighbour
DEV bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
DEV bool finite3(float x, float y, float z) { return finite_f32(x) && finite_f32(y) && finite_f32(z); }
// the K smallest keys, ascending; x is no key of the set already (every candidate is met once)
template <int K>
DEV void keep_key(unsigned long long (&best)[K], unsigned long long x)
{
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        const unsigned long long below = best[j - 1];
        best[j] = x < below ? below : (x < best[j] ? x : best[j]);
    }
    best[0] = x < best[0] ? x : best[0];
}

// ---- wave64 reductions and scan on the DPP network --------------------------------------------------------------------------------
// hipcc lowers __shfl_xor / __shfl_up to ds_bpermute_b32: a trip through the LDS crossbar per step, six DEPENDENT trips per reduction
// (~0.3 us on the chain of a workgroup that does nothing else meanwhile).  The same steps as DPP operand modifiers cost a few
// issue slots each: butterflies inside the quads and rows (quad_perm, row_half_mirror, row_mirror: every lane of a row then holds
// its row's value), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3: lane 63 holds the wave's value, read by
// v_readlane.  Every lane of the wave must be active (the call sites are wave-uniform).  Result: uniform.
template <int CTRL, int ROW_MASK>
DEV int dpp_take(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }
template <typename Op>
DEV int wave_reduce_i32(int v, int identity, Op op)
{
    v = op(v, dpp_take<0xB1, 0xf>(identity, v));    // quad_perm [1,0,3,2]
    v = op(v, dpp_take<0x4E, 0xf>(identity, v));    // quad_perm [2,3,0,1]
    v = op(v, dpp_take<0x141, 0xf>(identity, v));   // row_half_mirror
    v = op(v, dpp_take<0x140, 0xf>(identity, v));   // row_mirror
    v = op(v, dpp_take<0x142, 0xa>(identity, v));   // row_bcast:15 -> rows 1, 3
    v = op(v, dpp_take<0x143, 0xc>(identity, v));   // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}
DEV int wave_min_i32(int v) { return wave_reduce_i32(v, 0x7fffffff, [](int a, int b) { return a < b ? a : b; }); }
DEV int wave_max_i32(int v) { return wave_reduce_i32(v, (int)0x80000000, [](int a, int b) { return a > b ? a : b; }); }
DEV int wave_sum_i32(int v) { return wave_reduce_i32(v, 0, [](int a, int b) { return a + b; }); }
DEV unsigned wave_min_u32(unsigned v)
{
    return (unsigned)wave_reduce_i32((int)v, -1, [](int a, int b) { return (int)((unsigned)a < (unsigned)b ? (unsigned)a : (unsigned)b); });
}
DEV unsigned wave_max_u32(unsigned v)
{
    return (unsigned)wave_reduce_i32((int)v, 0, [](int a, int b) { return (int)((unsigned)a > (unsigned)b ? (unsigned)a : (unsigned)b); });
}
// inclusive prefix sum over the wave's 64 lanes (row_shr 1, 2, 3 on the input, then 4 and 8 with bank masks, then the two row
// broadcasts: the scan of the GCN3 cross-lane note)
DEV unsigned wave_inclusive_sum_u32(unsigned x)
{
    const int v0 = (int)x;
    int v = v0 + __builtin_amdgcn_update_dpp(0, v0, 0x111, 0xf, 0xf, false);      // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v0, 0x112, 0xf, 0xf, false);              // row_shr:2 (of the input)
    v += __builtin_amdgcn_update_dpp(0, v0, 0x113, 0xf, 0xf, false);              // row_shr:3 (of the input)
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xe, false);               // row_shr:4, banks 1-3
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xc, false);               // row_shr:8, banks 2-3
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);               // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);               // row_bcast:31 -> rows 2, 3
    return (unsigned)v;
}

// sum over the 16 lanes of this lane's DPP row: the first four butterflies of wave_reduce_i32 on v_mov_dpp, for a value of 32 bits.  A row
// IS a 4x4 block of the tile's pixels (pixel_of): neighbours in a quad, the quad's other pair, then -- every lane of a quad holding the
// quad's sum -- the row's half mirror swaps the quads of a half and the row mirror the halves.  Every lane of the row then holds the
// sum; unsigned sums are modular (two's complement values add as well).  Every lane of the wave is active at the call sites.
template <int CTRL, typename T>
DEV T mov_dpp(T v) { return __builtin_bit_cast(T, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)); }
template <typename T>   // unsigned, float
DEV T row_sum(T v)
{
    v += mov_dpp<0xB1>(v);    // quad_perm:[1,0,3,2]
    v += mov_dpp<0x4E>(v);    // quad_perm:[2,3,0,1]
    v += mov_dpp<0x141>(v);   // row_half_mirror
    v += mov_dpp<0x140>(v);   // row_mirror
    return v;
}

// lane `src` (uniform) of a register: v_readlane_b32 (hipcc's __shfl(v, src) is a ds_bpermute_b32 round trip even when src is uniform)
DEV int lane_get(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
DEV unsigned lane_get(unsigned v, int src) { return (unsigned)__builtin_amdgcn_readlane((int)v, src); }
DEV float lane_get(float v, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src)); }

// ---- contract logarithm (mirrors sas_oracle_logf) ------------------------------------------------
DEV float c_logf(float x)
{
    unsigned u = __float_as_uint(x);
    int e = (int)(u >> 23) - 127;
    float m = __uint_as_float((u & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421356237f) { m = m * 0.5f; e += 1; }
    float s = (m - 1.0f) / (m + 1.0f);
    float s2 = s * s;
    float p = 0.1111111111f;
    p = fma_(p, s2, 0.1428571429f);
    p = fma_(p, s2, 0.2f);
    p = fma_(p, s2, 0.3333333333f);
    p = fma_(p, s2, 1.0f);
    float lnm = (2.0f * s) * p;
    return fma_((float)e, 0.6931471805599453f, lnm);
}

DEV float affine3(float r0, float r1, float r2, float t, float v0, float v1, float v2)
{
    return fma_(r0, v0, fma_(r1, v1, fma_(r2, v2, t)));
}
DEV float dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return fma_(a2, b2, fma_(a1, b1, a0 * b0));
}
// Row R of A p + t, p = (x, y, z), for the calls that need no scene; nothing fused: the association order is part of their contract.
// v: the record that holds the map as its member `m` (SasDepthView, SasMatch).  It takes the record and not the SasAffine because
// k_fuse, handed a pointer into the middle of its view row, keeps a second base register in its view loop: two more scalar instructions
// per view (tools/isa_gate.py).
template <int R, class V>
DEV float sas_affine_row(const V &v, float x, float y, float z)
{
    const SasAffine &m = v.m;
    return ((m.A[3 * R] * x + m.A[3 * R + 1] * y) + m.A[3 * R + 2] * z) + m.t[R];
}
// p moved by the 3x4 row block G = [R | t] (a group pose), in place
DEV void pose_point(const float *G, float *p)
{
    const float x = affine3(G[0], G[1], G[2], G[3], p[0], p[1], p[2]);
    const float y = affine3(G[4], G[5], G[6], G[7], p[0], p[1], p[2]);
    const float z = affine3(G[8], G[9], G[10], G[11], p[0], p[1], p[2]);
    p[0] = x; p[1] = y; p[2] = z;
}
// q = the world point p in the camera frame of c
DEV void to_camera(const SasCam &c, const float *p, float *q)
{
    q[0] = affine3(c.R[0], c.R[1], c.R[2], c.t[0], p[0], p[1], p[2]);
    q[1] = affine3(c.R[3], c.R[4], c.R[5], c.t[1], p[0], p[1], p[2]);
    q[2] = affine3(c.R[6], c.R[7], c.R[8], c.t[2], p[0], p[1], p[2]);
}

// out = R s R^T, s = xx xy xz yy yz zz
DEV void rot_sym3(const float *R, const float *s, float *out)
{
    const float S[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    float T[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            T[i][j] = dot3(R[3 * i + 0], R[3 * i + 1], R[3 * i + 2], S[0][j], S[1][j], S[2][j]);
    out[0] = dot3(T[0][0], T[0][1], T[0][2], R[0], R[1], R[2]);
    out[1] = dot3(T[0][0], T[0][1], T[0][2], R[3], R[4], R[5]);
    out[2] = dot3(T[0][0], T[0][1], T[0][2], R[6], R[7], R[8]);
    out[3] = dot3(T[1][0], T[1][1], T[1][2], R[3], R[4], R[5]);
    out[4] = dot3(T[1][0], T[1][1], T[1][2], R[6], R[7], R[8]);
    out[5] = dot3(T[2][0], T[2][1], T[2][2], R[6], R[7], R[8]);
}

// ---- contract T6 per (pixel, splat) pair: shared by the compositing loop (sas_tile.hip) and its backward pass (sas_grad.hip) ----------
// Contract exp for an argument the caller has clamped to [-86, rounding noise] (sas_oracle_expf clamps to
// [-86, 86]; -sigma never comes near the upper end).  n = round(x log2 e) is read off the low mantissa bits
// of x log2 e + 1.5 * 2^23 and added straight into the exponent field.
DEV float c_expf_neg(float x, float e5 /* 0.0013400432653725147f, pinned in a register */)
{
    const float magic = 12582912.0f;
    const float tm = fma_(x, 1.4426950408889634f, magic);
    const float n = tm - magic;
    const float fr = fma_(x, 1.4426950408889634f, -n);
    float p = fma_(e5, fr, 0.009676037356257439f);
    p = fma_(p, fr, 0.05550327152013779f);
    p = fma_(p, fr, 0.2402210682630539f);
    p = fma_(p, fr, 0.6931471824645996f);
    p = fma_(p, fr, 1.0000001192092896f);
    return __uint_as_float(__float_as_uint(p) + (__float_as_uint(tm) << 23));
}

// Contract T6 for one (pixel, splat) pair, step by step.  (dx, dy) = (u - x, v - y); K = (u, v, A/2, B), H = (C/2, opacity) as staged
// by blend_range.  A trip runs the steps of its entries side by side, in this order: where they are called decides the loop's schedule.
DEV float splat_sigma(const float4 K, const float2 H, float dx, float dy) { return fma_(dx, fma_(K.w, dy, K.z * dx), (H.x * dy) * dy); }
template <bool FAST_EXP>
DEV float splat_exp(float sigma, float sE5) { return FAST_EXP ? __expf(fmaxf(-sigma, -86.0f)) : c_expf_neg(fmaxf(-sigma, -86.0f), sE5); }
DEV float splat_alpha(const float2 H, float E) { return fminf(kMaxAlpha, H.y * E); }

// ---- a workgroup on one tile of a frame: the pixel layout, the pixel's start, the tile's list (sas_tile.hip, sas_grad.hip) ---------------
// Pixel of (wave, lane) inside the tile: wave w owns the 8x8 quadrant (w & 1, w >> 1); its four
// 16-lane groups own the quadrant's 4x4 blocks, so that each group can walk its own splat queue.
DEV void pixel_of(int wv, int lane, int &ox, int &oy)
{
    const int g = lane >> 4, q = lane & 15;
    ox = (wv & 1) * 8 + (g & 1) * 4 + (q & 3);
    oy = (wv >> 1) * 8 + (g >> 1) * 4 + (q >> 2);
}

// Per-pixel compositing state.  x is the pixel centre relative to the tile's centre.  A terminated
// pixel (transmittance test fired, or outside the image) is parked at x = NaN: every later sigma is
// then NaN and fails `sigma <= thr` by itself, so the inner loop carries no "done" flag.
struct PixState {
    float T, r, g, b, d;
    float x;
};
// Contract T6: the tile-local frame (u, v, x, y) has its origin at the CENTRE of the 16-pixel tile (x, y in -7.5 .. 7.5)
constexpr float kTileCentre = 8.0f;
DEV PixState pix_init(bool inside, int ox) { return PixState{1.0f, 0.f, 0.f, 0.f, 0.f, inside ? ((float)ox + 0.5f) - kTileCentre : __builtin_nanf("")}; }
// Pixel (ox, oy) of tile (tx, ty) starts: its image coordinates, whether it lies inside the image, its state; wdone: the wave has
// no pixel inside.
DEV PixState pixel_begin(const SasCam &c, int tx, int ty, int ox, int oy, int &ix, int &iy, bool &inside, bool &wdone)
{
    ix = tx * SAS_TILE + ox;
    iy = ty * SAS_TILE + oy;
    inside = ix < c.W && iy < c.H;
    const PixState p = pix_init(inside, ox);
    wdone = __all(!inside);
    return p;
}
// A tile's segment [beg, end) of the frame's key / id arrays.  (The clamp to the arrays' capacity is a safety check: the
// projection never hands out more.)
DEV void tile_segment(const SasFrame &f, int tile, long long &beg, long long &end)
{
    beg = f.tile_offset[tile];
    end = f.tile_offset[tile + 1];
    if (end > f.cap) end = f.cap;
}

// One lane of a workgroup on tile `tile`: its pixel and the tile's depth-ordered list -- what a kernel that composites a tile's list
// starts from, behind its own tile lookup and range checks (blend_tile inside its persistent loop; label_tile, k_lift_labels,
// k_lift_features).  tile_lane fills in the pixel, tile_list the list: entries ids[0, count) of f.sorted_ids.  Two steps, because each
// kernel reads what it needs at its pixel in between and hipcc schedules the loads in the order they are written; the range checks
// stay in the kernels, because returns that come out of a shared function compile to other code (profiles/list_readers_ab.txt).
// k_blend_features[_mesh] and k_grad_tiles keep their own text (see there).
struct TileLane {
    int tile, tx, ty, ox, oy, ix, iy;   // the tile; the pixel inside it (pixel_of) and in the image
    bool inside, wdone;                 // the pixel lies inside the image; the wave has no pixel inside
    PixState p;
    const int *ids;                     // (blend_range's slot lambda goes over a local copy: capturing this record changes k_blend*'s code)
    int count;
};
DEV TileLane tile_lane(const SasCam &c, int tile, int wv, int lane)
{
    TileLane w;
    w.tile = tile;
    w.tx = tile % c.tw;
    w.ty = tile / c.tw;
    pixel_of(wv, lane, w.ox, w.oy);
    w.p = pixel_begin(c, w.tx, w.ty, w.ox, w.oy, w.ix, w.iy, w.inside, w.wdone);
    return w;
}
template <bool CLAMP = true>   // (false: k_blend*'s text, which hands blend_range the difference as it is: a negative count is an empty list)
DEV void tile_list(const SasFrame &f, TileLane &w)
{
    long long beg, end;
    tile_segment(f, w.tile, beg, end);
    w.ids = f.sorted_ids + beg;
    w.count = (!CLAMP || end > beg) ? (int)(end - beg) : 0;
}
// The truncated-list rule of every kernel that walks a FINISHED frame's complete lists and ADDS into buffers of the caller's
// (k_lift_labels, k_lift_features, k_grad_tiles): a frame whose lists outgrew the key buffer is rendered again (complete_oldest), so
// its first rendering adds NOTHING -- the truncated lists would be counted on top of the second rendering's complete ones.  Uniform;
// such a kernel returns on it before it reads a list.
DEV bool lists_truncated(const SasFrame &f) { return (long long)f.tile_offset[f.n_tiles] > f.cap; }
