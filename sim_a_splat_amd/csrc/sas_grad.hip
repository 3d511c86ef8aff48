// sas_grad.hip -- the backward pass of a frame's compositing (sas_render_backward_screen; DESIGN.md 3, "Backward pass"): from per-pixel
// gradients of the raw accumulators (sum c alpha T, 1 - T_final, sum z alpha T) to per-Gaussian gradients of what the projection
// staged for the tile kernel: mean2d, conic, opacity, colour, depth.
//
//   k_grad_tiles   one workgroup per tile, one lane per pixel (the pixel_of layout of the tile kernel), on the complete depth-ordered
//                  lists of a SAS_FULL_SORT frame.  Pass 1 walks the list front to back in staged batches of 256 entries and leaves,
//                  per pixel, T_final and the number of entries in front of the one that stopped it.  Pass 2 walks the same batches
//                  back to front with T_i = T_{i+1} / (1 - alpha_i) and the running S_i = sum_{j>i} w_j (c_j . g_rgb + z_j g_depth).
//                  Every lane meets every entry of the tile (no block queues: the walk is two loops over LDS), and an entry that no
//                  pixel of a wave composites costs that wave its alpha evaluation and one ballot.
// Sums: a wave adds the ten gradients of an entry over the 16 lanes of each 4x4 block on the DPP network (a row IS a block), then
// into the entry's ten LDS accumulators (ds_add_f32, one lane per value and row: ten neighbouring floats).  After a batch's walk the
// workgroup hands the batch over with ONE global float atomic per (entry, tile, value): lane t takes values t, t + 256, ... of the
// batch's [256][10] block, so the lanes of a wave-instruction that belong to one entry write neighbouring floats of its rows.  Sizing: DESIGN.md 3.
// Float atomics: the sums depend on arrival order and vary in their last bits from run to run.
// Decisions (alpha against 1/255 and 0.999, T (1 - alpha) against 1e-4) are constants of the derivative.  Arithmetic: contract T6's
// sigma on (dx, dy) and its exponential; gradients of K and of mesh vertices are not computed anywhere.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kGradVals = 10;   // mean2d (2), conic (3), opacity, colour (3), depth
constexpr int kGradAccStride = kGradVals;   // an entry's ten accumulators lie side by side: a row's ten adds fall in ten banks, the handover reads linearly

struct GradLds {
    float4 k[256];    // (u, v, A/2, B): mean2d relative to the tile's centre, conic
    float4 h[256];    // (C/2, opacity, depth, caller's index bits)
    float4 c[256];    // (r, g, b, -)
    float acc[256 * kGradAccStride];   // [entry][value]
};

// alpha of one staged entry at the pixel (x, y) of the tile-local frame, by the compositing loop's own steps (sas_device.h)
struct PairEval { float dx, dy, sigma, E, oE, alpha; };
template <bool FAST_EXP>
DEV PairEval eval_pair(const float4 K, const float4 Hh, float x, float y)
{
    PairEval e;
    e.dx = K.x - x;
    e.dy = K.y - y;
    const float2 H2 = make_float2(Hh.x, Hh.y);
    e.sigma = splat_sigma(K, H2, e.dx, e.dy);
    e.E = splat_exp<FAST_EXP>(e.sigma, 0.0013400432653725147f);   // (the leading coefficient the tile kernel pins in a register)
    e.oE = Hh.y * e.E;
    e.alpha = splat_alpha(H2, e.E);
    return e;
}

template <bool FAST_EXP>
__global__ __launch_bounds__(256) void k_grad_tiles(SasParams P, SasFrame f, long long n_gauss, SasGrad B, const int *perm)
{
    __shared__ __attribute__((aligned(16))) GradLds L;
    const SasCam &c = P.cam;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int oi = (int)blockIdx.x;
    if (!SAS_IN(oi, f.n_tiles, 801) || oi >= f.n_tiles) return;
    if (lists_truncated(f)) return;   // (uniform) the frame's second rendering adds
    const int tile = f.tile_order[oi];
    if (!SAS_IN(tile, f.n_tiles, 802) || tile < 0 || tile >= f.n_tiles) return;   // (uniform)
    const int tx = tile % c.tw, ty = tile / c.tw;
    // the tile kernel's pixel layout (pixel_of: wave w owns the 8x8 quadrant w, its 16-lane rows the quadrant's 4x4 blocks), written out:
    // through pixel_of / tile_lane hipcc forms the coordinates with other bit operations, and the config-3 backward frame measured
    // 0.5 .. 1.6 % over the parent's range (profiles/list_readers_ab.txt)
    const int g4 = lane >> 4, q4 = lane & 15;
    const int ox = (wv & 1) * 8 + (g4 & 1) * 4 + (q4 & 3), oy = (wv >> 1) * 8 + (g4 >> 1) * 4 + (q4 >> 2);
    const int ix = tx * SAS_TILE + ox, iy = ty * SAS_TILE + oy;
    const bool inside = ix < c.W && iy < c.H;
    const long long pix = (long long)iy * c.W + ix;
    const float x = ((float)ox + 0.5f) - kTileCentre, y = ((float)oy + 0.5f) - kTileCentre;
    const float X0 = (float)(tx * SAS_TILE) + kTileCentre, Y0 = (float)(ty * SAS_TILE) + kTileCentre;
    float gr = 0.0f, gg = 0.0f, gb = 0.0f, ga = 0.0f, gd = 0.0f;
    if (inside && SAS_IN(pix, P.out.n_pixels, 803)) {
        if (B.g_rgb) { gr = B.g_rgb[3 * pix + 0]; gg = B.g_rgb[3 * pix + 1]; gb = B.g_rgb[3 * pix + 2]; }
        if (B.g_alpha) ga = B.g_alpha[pix];
        if (B.g_depth) gd = B.g_depth[pix];
    }
    long long beg, end;
    tile_segment(f, tile, beg, end);
    const int count = end > beg ? (int)(end - beg) : 0;
    const int *ids = f.sorted_ids + beg;

    // one batch of up to 256 entries into LDS (between two barriers of the caller)
    auto stage = [&](int at) {
        const int idx = at + tid;
        float4 ra = make_float4(0, 0, 0, 0), rb = ra, rc = ra;
        int who = -1;
        if (idx < count) {
            long long id = (long long)(unsigned)ids[idx];
            if (!SAS_IN(id, n_gauss, 804) || id >= n_gauss) id = n_gauss - 1;   // never dereference a bad index
            ra = f.rec[SAS_RS * id + 0];
            rb = f.rec[SAS_RS * id + 1];
            rc = f.col[SAS_CS * id];
            who = perm[id];
        }
        L.k[tid] = make_float4(ra.x - X0, ra.y - Y0, 0.5f * ra.z, ra.w);
        L.h[tid] = make_float4(0.5f * rb.x, rb.y, rb.w, __int_as_float(who));   // an empty slot has opacity 0: no pixel accepts it
        L.c[tid] = rc;
#pragma unroll
        for (int k = 0; k < kGradVals; ++k) L.acc[tid * kGradAccStride + k] = 0.0f;
    };

    // ---- pass 1: T_final, and `stop`: entries [0, stop) are the ones the pixel met before it terminated
    float T = 1.0f;
    int stop = inside ? count : 0;
    bool done = !inside;
    for (int at = 0; at < count; at += 256) {
        __syncthreads();   // the previous batch is consumed
        stage(at);
        __syncthreads();
        const int cnt = (count - at) < 256 ? (count - at) : 256;
        if (!__all(done)) {
            for (int e = 0; e < cnt; ++e) {
                const PairEval v = eval_pair<FAST_EXP>(L.k[e], L.h[e], x, y);
                if (done || v.sigma < 0.0f || !(v.alpha >= kAlphaThr)) continue;
                const float w = v.alpha * T, nT = T - w;   // (the frame's own form of T (1 - alpha))
                if (nT <= kTStop) { done = true; stop = at + e; continue; }   // the entry that ends a pixel is not composited
                T = nT;
            }
        }
        if (!__syncthreads_or(!done)) break;   // (uniform) every pixel of the tile has terminated
    }
    const float T_final = T;
    // the last batch any pixel of the tile needs (uniform)
    __shared__ int s_top;
    __syncthreads();
    if (tid == 0) s_top = 0;
    __syncthreads();
    if (stop > 0) atomicMax(&s_top, stop);
    __syncthreads();
    const int top = s_top;

    // ---- pass 2: back to front
    float S = 0.0f;   // sum over the entries behind of w (c . g_rgb + z g_depth)
    for (int at = ((top - 1) >> 8) << 8; top > 0 && at >= 0; at -= 256) {
        __syncthreads();   // the previous batch's sums have been handed over
        stage(at);
        __syncthreads();
        const int cnt = (top - at) < 256 ? (top - at) : 256;
        if (__any(stop > at)) {   // (wave-uniform)
            for (int e = cnt - 1; e >= 0; --e) {
                const float4 K = L.k[e], Hh = L.h[e], C = L.c[e];
                const PairEval v = eval_pair<FAST_EXP>(K, Hh, x, y);
                const bool use = at + e < stop && !(v.sigma < 0.0f) && v.alpha >= kAlphaThr;
                if (!__any(use)) continue;   // (wave-uniform) nobody in the wave composited this entry
                float d[kGradVals];
#pragma unroll
                for (int k = 0; k < kGradVals; ++k) d[k] = 0.0f;
                if (use) {
                    const float om = 1.0f - v.alpha, rom = 1.0f / om;
                    const float Ti = T * rom, w = v.alpha * Ti;
                    const float dot = fma_(Hh.z, gd, fma_(C.z, gb, fma_(C.y, gg, C.x * gr)));
                    const float dLda = fma_(ga * T_final, rom, fma_(Ti, dot, -(S * rom)));
                    S = fma_(w, dot, S);
                    T = Ti;
                    // a clamped alpha passes nothing to the opacity or to sigma
                    const bool clamped = v.oE > kMaxAlpha;
                    const float dsig = clamped ? 0.0f : -(v.alpha * dLda);
                    d[0] = fma_(2.0f * K.z, v.dx, K.w * v.dy) * dsig;            // d sigma / d mx = a dx + b dy
                    d[1] = fma_(2.0f * Hh.x, v.dy, K.w * v.dx) * dsig;           // d sigma / d my = c dy + b dx
                    d[2] = (0.5f * v.dx * v.dx) * dsig;
                    d[3] = (v.dx * v.dy) * dsig;
                    d[4] = (0.5f * v.dy * v.dy) * dsig;
                    d[5] = clamped ? 0.0f : v.E * dLda;
                    d[6] = w * gr;
                    d[7] = w * gg;
                    d[8] = w * gb;
                    d[9] = w * gd;
                }
                // over the block (a DPP row), then lane k of the row adds value k to the entry's accumulator
                float mine = 0.0f;
#pragma unroll
                for (int k = 0; k < kGradVals; ++k) {
                    const float s = row_sum(d[k]);
                    if (q4 == k) mine = s;
                }
                if (q4 < kGradVals && mine != 0.0f && SAS_IN(e * kGradAccStride + q4, 256 * kGradAccStride, 805)) atomicAdd(&L.acc[e * kGradAccStride + q4], mine);
            }
        }
        __syncthreads();
        // hand the batch over: value v = 10 entry + k, so the lanes of one entry write neighbouring floats
        for (int v = tid; v < cnt * kGradVals; v += 256) {
            const int e = v / kGradVals, k = v - e * kGradVals;
            const float s = L.acc[e * kGradAccStride + k];
            const int who = __float_as_int(L.h[e].w);
            if (s == 0.0f || who < 0 || (long long)who >= B.n || !SAS_IN(who, B.n, 806)) continue;
            float *dst = nullptr;
            if (k < 2) dst = B.d_means2d ? B.d_means2d + 2 * (long long)who + k : nullptr;
            else if (k < 5) dst = B.d_conics ? B.d_conics + 3 * (long long)who + (k - 2) : nullptr;
            else if (k == 5) dst = B.d_opacities ? B.d_opacities + who : nullptr;
            else if (k < 9) dst = B.d_colors ? B.d_colors + 3 * (long long)who + (k - 6) : nullptr;
            else dst = B.d_depths ? B.d_depths + who : nullptr;
            if (dst) atomicAdd(dst, s);
        }
    }
}

// ---- projection backward ---------------------------------------------------------------------------------------------------------
//   k_grad_project   one lane per Gaussian (storage slot j, caller's index perm[j]): recomputes T1 / T2 of the view in plain float32
//                    and chains the screen-space gradients of k_grad_tiles through them: the conic as the inverse of
//                    Sigma2 = J Sigma_c J^T + 0.3 I, the pinhole Jacobian J (its tx / ty clamp a constant where it binds), mean2d, the
//                    depth, Sigma_c = R Sigma3 R^T, Sigma3 from quaternion and scale or the uploaded covariance, the group pose, and the
//                    SH colour max(SH(d) . coeffs + 0.5, 0) with d = normalize(mean - campos).  A Gaussian the frame culled (its info
//                    record is zero) adds nothing.  Each lane ADDS to its own Gaussian's rows: no atomics.
//                    The view matrix' gradient is summed in a fixed order: butterflies over the wave, the four waves through LDS, one
//                    row of 12 per workgroup; k_grad_viewmat adds the rows in workgroup order.  One view's pose gradient is therefore
//                    reproducible given the screen-space gradients (which are float atomic sums).
//                    <POSES> (sas_render_backward_poses) forms the same kind of sum per selected group for dL/dG, G = [Rg | t] the group's
//                    pose: dL/dt = gm (the posed mean's gradient), dL/dRg = gm m0^T + 2 GSw Rg S0.  A lane's slot is its group's place in
//                    the selection; per wave each slot present (a ballot) is summed over its lanes, absent slots are skipped, the waves
//                    and then the workgroups (k_grad_poses) are added in order: no atomics.  <false> is the kernel without any of it.
struct Sym3 { float m[3][3]; };

// real SH basis and its derivatives with respect to the unit direction's components taken as independent (gsplat's signs)
DEV void sh_basis_grad(int deg, float x, float y, float z, float *Bv, float *Bx, float *By, float *Bz)
{
#pragma unroll
    for (int k = 0; k < 16; ++k) { Bv[k] = 0.0f; Bx[k] = 0.0f; By[k] = 0.0f; Bz[k] = 0.0f; }
    Bv[0] = 0.2820947917738781f;
    if (deg < 1) return;
    const float c1 = 0.48860251190292f;
    Bv[1] = -c1 * y; By[1] = -c1;
    Bv[2] = c1 * z;  Bz[2] = c1;
    Bv[3] = -c1 * x; Bx[3] = -c1;
    if (deg < 2) return;
    const float k4 = 0.5462742152960395f, k5 = 1.092548430592079f, k6 = 0.9461746957575601f;
    const float z2 = z * z, fC1 = x * x - y * y, fS1 = 2.0f * x * y;
    Bv[4] = k4 * fS1;        Bx[4] = k4 * 2.0f * y;  By[4] = k4 * 2.0f * x;
    Bv[5] = -k5 * z * y;     By[5] = -k5 * z;        Bz[5] = -k5 * y;
    Bv[6] = k6 * z2 - 0.3153915652525201f;           Bz[6] = 2.0f * k6 * z;
    Bv[7] = -k5 * z * x;     Bx[7] = -k5 * z;        Bz[7] = -k5 * x;
    Bv[8] = k4 * fC1;        Bx[8] = k4 * 2.0f * x;  By[8] = -k4 * 2.0f * y;
    if (deg < 3) return;
    const float k9 = 0.5900435899266435f, k10 = 1.445305721320277f, k11 = 2.285228997322329f, k12 = 1.865881662950577f;
    const float t0c = -k11 * z2 + 0.4570457994644658f;
    const float fC2 = x * fC1 - y * fS1, fS2 = x * fS1 + y * fC1;
    Bv[9] = -k9 * fS2;       Bx[9] = -k9 * 6.0f * x * y;          By[9] = -k9 * 3.0f * fC1;
    Bv[10] = k10 * z * fS1;  Bx[10] = k10 * 2.0f * y * z;         By[10] = k10 * 2.0f * x * z;   Bz[10] = k10 * fS1;
    Bv[11] = t0c * y;        By[11] = t0c;                        Bz[11] = -2.0f * k11 * z * y;
    Bv[12] = z * (k12 * z2 - 1.119528997770346f);                 Bz[12] = 3.0f * k12 * z2 - 1.119528997770346f;
    Bv[13] = t0c * x;        Bx[13] = t0c;                        Bz[13] = -2.0f * k11 * z * x;
    Bv[14] = k10 * z * fC1;  Bx[14] = k10 * 2.0f * x * z;         By[14] = -k10 * 2.0f * y * z;  Bz[14] = k10 * fC1;
    Bv[15] = -k9 * fC2;      Bx[15] = -k9 * 3.0f * fC1;           By[15] = k9 * 6.0f * x * y;
}

template <bool POSES>
__global__ __launch_bounds__(256) void k_grad_project(SasScene s, SasCam c, const uint4 *info, const float *poses, SasGradProj B, SasPoseSel S)
{
    __shared__ float s_part[4][12];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float gV[12];   // this lane's share of d_viewmat, rows [R | t]
#pragma unroll
    for (int k = 0; k < 12; ++k) gV[k] = 0.0f;
    float gP[12];   // POSES: this lane's dL/dG of its own group, rows [R | t]; slot: the group's place in the selection, or none
    int slot = -1;
#pragma unroll
    for (int k = 0; k < 12; ++k) gP[k] = 0.0f;
    bool live = j < s.n && SAS_IN(j, s.n, 810);
    if (live) {
        const uint4 inf = info[j];
        live = inf.z != 0u && inf.w != 0u;   // zero: culled by the frame's projection
    }
    if (live) {
        const int64_t i = s.perm[j];
        live = i >= 0 && i < B.n && SAS_IN(i, B.n, 811);
        if (live) {
            const float4 a0 = s.g0[j], a1 = s.g1[j], a2 = s.g2[j];
            const float m0[3] = {a0.x, a0.y, a0.z};
            float G[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
            const unsigned gid = __float_as_uint(a2.w) & 255u;
            const bool hasG = poses != nullptr && s.n_groups > 0 && gid < (unsigned)s.n_groups;
            if (hasG)
#pragma unroll
                for (int k = 0; k < 12; ++k) G[k] = poses[12 * gid + k];
            float m[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) m[r] = G[4 * r] * m0[0] + G[4 * r + 1] * m0[1] + G[4 * r + 2] * m0[2] + G[4 * r + 3];
            float q[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) q[r] = c.R[3 * r] * m[0] + c.R[3 * r + 1] * m[1] + c.R[3 * r + 2] * m[2] + c.t[r];
            const float x = q[0], y = q[1], z = q[2];

            // ---- forward: Sigma3 in the world frame
            float Rt[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, Rq[9], Mw[9], qn[4] = {1.f, 0.f, 0.f, 0.f}, qlen = 1.0f;
            const float sc[3] = {a2.x, a2.y, a2.z};
            const float Rg[9] = {G[0], G[1], G[2], G[4], G[5], G[6], G[8], G[9], G[10]};
            float Sw[3][3];
            if (!s.cov_mode) {
                qlen = sqrtf(a1.x * a1.x + a1.y * a1.y + a1.z * a1.z + a1.w * a1.w);
                const float qw = a1.x / qlen, qx = a1.y / qlen, qy = a1.z / qlen, qz = a1.w / qlen;
                qn[0] = qw; qn[1] = qx; qn[2] = qy; qn[3] = qz;
                Rq[0] = 1.0f - 2.0f * (qy * qy + qz * qz); Rq[1] = 2.0f * (qx * qy - qw * qz); Rq[2] = 2.0f * (qx * qz + qw * qy);
                Rq[3] = 2.0f * (qx * qy + qw * qz); Rq[4] = 1.0f - 2.0f * (qx * qx + qz * qz); Rq[5] = 2.0f * (qy * qz - qw * qx);
                Rq[6] = 2.0f * (qx * qz - qw * qy); Rq[7] = 2.0f * (qy * qz + qw * qx); Rq[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        Rt[3 * r + k] = Rg[3 * r] * Rq[k] + Rg[3 * r + 1] * Rq[3 + k] + Rg[3 * r + 2] * Rq[6 + k];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) Mw[3 * r + k] = Rt[3 * r + k] * sc[k];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        Sw[r][k] = Mw[3 * r] * Mw[3 * k] + Mw[3 * r + 1] * Mw[3 * k + 1] + Mw[3 * r + 2] * Mw[3 * k + 2];
            } else {
                const float S0[3][3] = {{a1.x, a1.y, a1.z}, {a1.y, a1.w, a2.x}, {a1.z, a2.x, a2.y}};
                float T0[3][3];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) T0[r][k] = Rg[3 * r] * S0[0][k] + Rg[3 * r + 1] * S0[1][k] + Rg[3 * r + 2] * S0[2][k];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) Sw[r][k] = T0[r][0] * Rg[3 * k] + T0[r][1] * Rg[3 * k + 1] + T0[r][2] * Rg[3 * k + 2];
            }
            // Sigma_c = R Sigma3 R^T
            float RS[3][3], Sc[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) RS[r][k] = c.R[3 * r] * Sw[0][k] + c.R[3 * r + 1] * Sw[1][k] + c.R[3 * r + 2] * Sw[2][k];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) Sc[r][k] = RS[r][0] * c.R[3 * k] + RS[r][1] * c.R[3 * k + 1] + RS[r][2] * c.R[3 * k + 2];
            // J and Sigma2
            const float rz = 1.0f / z, rz2 = rz * rz;
            const float ux = x * rz, uy = y * rz;
            const bool clx = ux > c.lim_x_pos || ux < -c.lim_x_neg, cly = uy > c.lim_y_pos || uy < -c.lim_y_neg;
            const float lx = fminf(c.lim_x_pos, fmaxf(-c.lim_x_neg, ux)), ly = fminf(c.lim_y_pos, fmaxf(-c.lim_y_neg, uy));
            const float tx = z * lx, ty = z * ly;
            const float J[2][3] = {{c.fx * rz, 0.0f, -((c.fx * tx) * rz2)}, {0.0f, c.fy * rz, -((c.fy * ty) * rz2)}};
            float T[2][3];   // J Sigma_c
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) T[r][k] = J[r][0] * Sc[0][k] + J[r][1] * Sc[1][k] + J[r][2] * Sc[2][k];
            const float c00 = T[0][0] * J[0][0] + T[0][1] * J[0][1] + T[0][2] * J[0][2] + kEps2d;
            const float c01 = T[0][0] * J[1][0] + T[0][1] * J[1][1] + T[0][2] * J[1][2];
            const float c11 = T[1][0] * J[1][0] + T[1][1] * J[1][1] + T[1][2] * J[1][2] + kEps2d;
            const float det = c00 * c11 - c01 * c01;
            const float idet = 1.0f / det;
            const float ca = c11 * idet, cb = -c01 * idet, cc = c00 * idet;

            // ---- backward
            const float gmx = B.s_means2d[2 * i], gmy = B.s_means2d[2 * i + 1];
            const float gca = B.s_conics[3 * i], gcb = B.s_conics[3 * i + 1], gcc = B.s_conics[3 * i + 2];
            const float gdet = -(gca * ca + gcb * cb + gcc * cc) * idet;
            const float g00 = gcc * idet + gdet * c11, g11 = gca * idet + gdet * c00, g01 = -gcb * idet - 2.0f * gdet * c01;
            const float G2[2][2] = {{g00, 0.5f * g01}, {0.5f * g01, g11}};
            float Wm[2][3];   // G2 J
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) Wm[r][k] = G2[r][0] * J[0][k] + G2[r][1] * J[1][k];
            float GSc[3][3];   // J^T G2 J: gradient of Sigma_c, entries taken as independent
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) GSc[r][k] = J[0][r] * Wm[0][k] + J[1][r] * Wm[1][k];
            float GJ[2][3];    // 2 G2 (J Sigma_c)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) GJ[r][k] = 2.0f * (G2[r][0] * T[0][k] + G2[r][1] * T[1][k]);
            float grz = c.fx * GJ[0][0] + c.fy * GJ[1][1];
            grz += -2.0f * c.fx * tx * rz * GJ[0][2] - 2.0f * c.fy * ty * rz * GJ[1][2];
            const float gtx = -c.fx * rz2 * GJ[0][2], gty = -c.fy * rz2 * GJ[1][2];
            float gq[3] = {0.0f, 0.0f, 0.0f};
            // tx = z clamp(x / z): x where the clamp does not bind, z lim where it does
            if (clx) gq[2] += lx * gtx; else gq[0] += gtx;
            if (cly) gq[2] += ly * gty; else gq[1] += gty;
            gq[0] += c.fx * rz * gmx;
            gq[1] += c.fy * rz * gmy;
            grz += c.fx * x * gmx + c.fy * y * gmy;
            gq[2] += -rz2 * grz + B.s_depths[i];
            // Sigma_c = R Sigma3 R^T
            float GSw[3][3], RtG[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) RtG[r][k] = c.R[r] * GSc[0][k] + c.R[3 + r] * GSc[1][k] + c.R[6 + r] * GSc[2][k];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) GSw[r][k] = RtG[r][0] * c.R[k] + RtG[r][1] * c.R[3 + k] + RtG[r][2] * c.R[6 + k];
            // d_viewmat: rotation from Sigma_c (2 GSc R Sigma3) and from the mean, translation from the mean
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    gV[4 * r + k] = 2.0f * (GSc[r][0] * RS[0][k] + GSc[r][1] * RS[1][k] + GSc[r][2] * RS[2][k]) + gq[r] * m[k];
                gV[4 * r + 3] = gq[r];
            }
            float gm[3];   // posed world mean
#pragma unroll
            for (int k = 0; k < 3; ++k) gm[k] = c.R[k] * gq[0] + c.R[3 + k] * gq[1] + c.R[6 + k] * gq[2];

            // ---- colour
            const float gc3[3] = {B.s_colors[3 * i], B.s_colors[3 * i + 1], B.s_colors[3 * i + 2]};
            if (s.sh_degree < 0) {
                if (B.d_sh)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) B.d_sh[3 * i + ch] += gc3[ch];
            } else {
                const int Kc = (s.sh_degree + 1) * (s.sh_degree + 1);
                const float d[3] = {m[0] - c.campos[0], m[1] - c.campos[1], m[2] - c.campos[2]};
                const float dl = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), idl = 1.0f / dl;
                const float ux3[3] = {d[0] * idl, d[1] * idl, d[2] * idl};
                float Bv[16], Bx[16], By[16], Bz[16];
                sh_basis_grad(s.sh_degree, ux3[0], ux3[1], ux3[2], Bv, Bx, By, Bz);
                float sh[48];
#pragma unroll
                for (int p = 0; p < 12; ++p) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (4 * p < 3 * Kc) v = s.col[(int64_t)p * s.n_pad + j];
                    sh[4 * p] = v.x; sh[4 * p + 1] = v.y; sh[4 * p + 2] = v.z; sh[4 * p + 3] = v.w;
                }
                float rgb[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < Kc)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) rgb[ch] += Bv[k] * sh[3 * k + ch];
                float gcm[3];   // through max(. , 0)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) gcm[ch] = rgb[ch] > 0.0f ? gc3[ch] : 0.0f;
                float gu[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if (k >= Kc) continue;
                    const float v = sh[3 * k] * gcm[0] + sh[3 * k + 1] * gcm[1] + sh[3 * k + 2] * gcm[2];
                    gu[0] += Bx[k] * v; gu[1] += By[k] * v; gu[2] += Bz[k] * v;
                    if (B.d_sh && SAS_IN((int64_t)3 * Kc * i + 3 * k + 2, (int64_t)3 * Kc * B.n, 812))
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) B.d_sh[(int64_t)3 * Kc * i + 3 * k + ch] += Bv[k] * gcm[ch];
                }
                const float ug = ux3[0] * gu[0] + ux3[1] * gu[1] + ux3[2] * gu[2];
                float gd3[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) gd3[k] = (gu[k] - ux3[k] * ug) * idl;
                // d = mean - campos, campos = -R^T t
#pragma unroll
                for (int k = 0; k < 3; ++k) gm[k] += gd3[k];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) gV[4 * r + k] += c.t[r] * gd3[k];
                    gV[4 * r + 3] += c.R[3 * r] * gd3[0] + c.R[3 * r + 1] * gd3[1] + c.R[3 * r + 2] * gd3[2];
                }
            }
            // ---- the uploaded arrays
            if (B.d_means)
#pragma unroll
                for (int k = 0; k < 3; ++k) B.d_means[3 * i + k] += Rg[k] * gm[0] + Rg[3 + k] * gm[1] + Rg[6 + k] * gm[2];
            if (B.d_opacities) B.d_opacities[i] += B.s_opacities[i];
            if (!s.cov_mode) {
                float GM[9];   // 2 GSw M
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) GM[3 * r + k] = 2.0f * (GSw[r][0] * Mw[k] + GSw[r][1] * Mw[3 + k] + GSw[r][2] * Mw[6 + k]);
                if (B.d_scales)
#pragma unroll
                    for (int k = 0; k < 3; ++k) B.d_scales[3 * i + k] += GM[k] * Rt[k] + GM[3 + k] * Rt[3 + k] + GM[6 + k] * Rt[6 + k];
                if (B.d_quats) {
                    float GRt[9], Gq[3][3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) GRt[3 * r + k] = GM[3 * r + k] * sc[k];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) Gq[r][k] = Rg[r] * GRt[k] + Rg[3 + r] * GRt[3 + k] + Rg[6 + r] * GRt[6 + k];
                    const float w = qn[0], qx = qn[1], qy = qn[2], qz = qn[3];
                    float gh[4];
                    gh[0] = 2.0f * (-qz * Gq[0][1] + qy * Gq[0][2] + qz * Gq[1][0] - qx * Gq[1][2] - qy * Gq[2][0] + qx * Gq[2][1]);
                    gh[1] = 2.0f * (qy * Gq[0][1] + qz * Gq[0][2] + qy * Gq[1][0] - 2.0f * qx * Gq[1][1] - w * Gq[1][2] + qz * Gq[2][0] + w * Gq[2][1] - 2.0f * qx * Gq[2][2]);
                    gh[2] = 2.0f * (-2.0f * qy * Gq[0][0] + qx * Gq[0][1] + w * Gq[0][2] + qx * Gq[1][0] + qz * Gq[1][2] - w * Gq[2][0] + qz * Gq[2][1] - 2.0f * qy * Gq[2][2]);
                    gh[3] = 2.0f * (-2.0f * qz * Gq[0][0] - w * Gq[0][1] + qx * Gq[0][2] + w * Gq[1][0] - 2.0f * qz * Gq[1][1] + qy * Gq[1][2] + qx * Gq[2][0] + qy * Gq[2][1]);
                    const float hg = qn[0] * gh[0] + qn[1] * gh[1] + qn[2] * gh[2] + qn[3] * gh[3];
#pragma unroll
                    for (int k = 0; k < 4; ++k) B.d_quats[4 * i + k] += (gh[k] - qn[k] * hg) / qlen;
                }
            } else if (B.d_cov6) {
                float T1[3][3], G0[3][3];   // Rg^T GSw Rg
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) T1[r][k] = Rg[r] * GSw[0][k] + Rg[3 + r] * GSw[1][k] + Rg[6 + r] * GSw[2][k];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) G0[r][k] = T1[r][0] * Rg[k] + T1[r][1] * Rg[3 + k] + T1[r][2] * Rg[6 + k];
                float *o = B.d_cov6 + 6 * i;
                o[0] += G0[0][0]; o[1] += 2.0f * G0[0][1]; o[2] += 2.0f * G0[0][2];
                o[3] += G0[1][1]; o[4] += 2.0f * G0[1][2]; o[5] += G0[2][2];
            }
            // ---- the group's pose, G's twelve entries taken as independent: t from the posed mean, Rg from the mean and from Sigma3 = Rg S0 Rg^T
            if constexpr (POSES) {
                if (hasG)
                    for (int q = 0; q < S.n_sel; ++q)   // (uniform trip count; the ids are distinct)
                        if (((S.ids[q >> 2] >> (8 * (q & 3))) & 255u) == gid) slot = q;
                if (slot >= 0) {
                    float X[9], Y[9];   // dL/dRg = X Y^T
                    if (!s.cov_mode) {  // 2 GSw Rg S0 = GM (Rq diag(sc))^T
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                X[3 * r + k] = 2.0f * (GSw[r][0] * Mw[k] + GSw[r][1] * Mw[3 + k] + GSw[r][2] * Mw[6 + k]);
                                Y[3 * r + k] = Rq[3 * r + k] * sc[k];
                            }
                    } else {            // 2 GSw (Rg S0)
                        const float S0[3][3] = {{a1.x, a1.y, a1.z}, {a1.y, a1.w, a2.x}, {a1.z, a2.x, a2.y}};
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                X[3 * r + k] = 2.0f * GSw[r][k];
                                Y[3 * r + k] = Rg[3 * k] * S0[0][r] + Rg[3 * k + 1] * S0[1][r] + Rg[3 * k + 2] * S0[2][r];   // (Rg S0)^T
                            }
                    }
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            gP[4 * r + k] = gm[r] * m0[k] + (X[3 * r] * Y[3 * k] + X[3 * r + 1] * Y[3 * k + 1] + X[3 * r + 2] * Y[3 * k + 2]);
                        gP[4 * r + 3] = gm[r];
                    }
                }
            }
        }
    }
    // the selected groups' poses: per slot present in the wave a butterfly over its lanes, the four waves in order, one row per
    // (workgroup, slot); k_grad_poses adds the rows in workgroup order.  Dead lanes and lanes of other groups hold zeros.
    if constexpr (POSES) {
        __shared__ float s_pose[4][SAS_MAX_POSE_GRAD_GROUPS][12];
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int q = 0; q < S.n_sel; ++q) {
            const bool mine = slot == q;
            const bool present = __any(mine);   // (wave-uniform)
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                float v = mine ? gP[k] : 0.0f;
                if (present)
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
                if (lane == 0) s_pose[wv][q][k] = v;
            }
        }
        __syncthreads();
        for (int t = (int)threadIdx.x; t < 12 * S.n_sel; t += 256) {   // (n_sel x 12 values, up to 384)
            const int q = t / 12, k = t - 12 * q;
            if (SAS_IN(12 * ((int64_t)blockIdx.x * S.n_sel) + t, 12 * (int64_t)gridDim.x * S.n_sel, 813))
                S.partial[12 * ((int64_t)blockIdx.x * S.n_sel) + t] = ((s_pose[0][q][k] + s_pose[1][q][k]) + s_pose[2][q][k]) + s_pose[3][q][k];
        }
    }
    // the view matrix: wave butterflies, then the four waves in order
    if (!B.partial) return;   // (uniform)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        float v = gV[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
        if (lane == 0) s_part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12)
        B.partial[12 * (int64_t)blockIdx.x + threadIdx.x] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
}

// d_group_poses[slot][k] += the workgroups' rows of that slot in workgroup order
__global__ __launch_bounds__(12 * SAS_MAX_POSE_GRAD_GROUPS) void k_grad_poses(const float *partial, int n_wg, int n_sel, float *d_group_poses)
{
    const int t = threadIdx.x;
    if (t >= 12 * n_sel) return;
    // the additions in workgroup order, one after the other; sixteen rows' loads are in flight at a time (a load per addition leaves
    // the one workgroup waiting on memory for every row: 3 907 rows at a million Gaussians)
    const int64_t stride = 12 * (int64_t)n_sel;
    float v = 0.0f;
    int w = 0;
    for (; w + 16 <= n_wg; w += 16) {
        float x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = partial[stride * (w + i) + t];
#pragma unroll
        for (int i = 0; i < 16; ++i) v += x[i];
    }
    for (; w < n_wg; ++w) v += partial[stride * w + t];
    d_group_poses[t] += v;
}

// d_viewmat[k] += the workgroups' rows in workgroup order
__global__ __launch_bounds__(64) void k_grad_viewmat(const float *partial, int n_wg, float *d_viewmat)
{
    const int k = threadIdx.x;
    if (k >= 12) return;
    float v = 0.0f;
    for (int w = 0; w < n_wg; ++w) v += partial[12 * (int64_t)w + k];
    d_viewmat[k] += v;
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_grad)

void sas_launch_grad_project(hipStream_t st, const SasScene &s, const SasParams &P, const SasFrame &f, const SasGradProj &B,
                             const SasPoseSel &S)
{
    if (s.n <= 0) return;
    const int n_wg = (int)((s.n + 255) / 256);
    const bool with_poses = S.n_sel > 0 && S.n_sel <= SAS_MAX_POSE_GRAD_GROUPS && S.partial && S.d_group_poses;
    if (with_poses) hipLaunchKernelGGL(k_grad_project<true>, dim3((unsigned)n_wg), dim3(256), 0, st, s, P.cam, (const uint4 *)f.info, f.group_Rt, B, S);
    else hipLaunchKernelGGL(k_grad_project<false>, dim3((unsigned)n_wg), dim3(256), 0, st, s, P.cam, (const uint4 *)f.info, f.group_Rt, B, S);
    if (B.partial && B.d_viewmat) hipLaunchKernelGGL(k_grad_viewmat, dim3(1), dim3(64), 0, st, (const float *)B.partial, n_wg, B.d_viewmat);
    if (with_poses)
        hipLaunchKernelGGL(k_grad_poses, dim3(1), dim3(12 * SAS_MAX_POSE_GRAD_GROUPS), 0, st, (const float *)S.partial, n_wg, S.n_sel, S.d_group_poses);
}

void sas_launch_grad_tiles(hipStream_t st, const SasScene &s, int tiles, const SasParams &P, const SasFrame &f, const SasGrad &B,
                           bool fast_exp)
{
    if (tiles <= 0 || s.n <= 0) return;
    if (fast_exp) hipLaunchKernelGGL(k_grad_tiles<true>, dim3((unsigned)tiles), dim3(256), 0, st, P, f, (long long)s.n, B, s.perm);
    else hipLaunchKernelGGL(k_grad_tiles<false>, dim3((unsigned)tiles), dim3(256), 0, st, P, f, (long long)s.n, B, s.perm);
}
