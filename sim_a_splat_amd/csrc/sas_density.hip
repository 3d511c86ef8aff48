// sas_density.hip -- adaptive density control on the resident scene (sas_density_accumulate, sas_scene_densify, sas_scene_reset_opacity;
// DESIGN.md 3, "Density control"), hand-written for gfx950 (CDNA4, wave64).
//
//   k_density_accumulate  one lane per storage slot: the screen-space gradient norm, the view count and the largest radius of the Gaussians
//                         the last backward frame saw, added to the caller's arrays at perm[slot].  No atomics: a Gaussian has one slot.
//   k_density_inverse     inv[perm[slot]] = slot: the decisions run in the CALLER's order, the planes are in storage order.
//   k_density_flag        one lane per Gaussian of the caller's order, 256 per workgroup: the three class bits (kept, clone candidate, split
//                         candidate) and the workgroup's count of each.
//   k_density_scan        ONE workgroup: the workgroup counts of the three classes -> exclusive offsets, and the totals.
//   k_density_scatter     the grid of k_density_flag again: rank in class = offset + rank in workgroup (ballots), then the new scene's
//                         rows in the caller's order (AoS, what sas_scene_upload takes) and `parents`: survivors, clones, pairs of children.
//   k_density_state       one lane per NEW storage slot: the optimiser state of its parent's old slot, or a fresh one.
//   k_density_state_fresh   behind it, the rows a mask marks started anew (sas_scene_mcmc_refine).
//   k_opacity_reset       one lane per storage slot: min(opacity, cap), and the opacity state of the lanes it changed.
// The planes of the new scene are laid out by k_relayout, as an upload lays them out.  The split between kernels is the one of
// sas_cloud.hip's compaction: no kernel waits for another workgroup, no look-back, no atomics.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_); correctly rounded / and sqrt, libm logf / cosf.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kKept = 1u, kClone = 2u, kSplit = 4u;

__global__ __launch_bounds__(kThreads) void k_density_accumulate(const SasDensityStats q)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // slot
    if (j >= q.n) return;
    const long long i = q.perm[j];                                        // caller's index
    if (!SAS_IN(i, q.n, 1001)) return;
    const uint4 inf = q.info[j];
    if (inf.z == 0u) return;   // culled in that frame
    const float gx = q.half_w * q.d_means2d[2 * i], gy = q.half_h * q.d_means2d[2 * i + 1];
    q.grad_sum[i] = q.grad_sum[i] + sqrtf(gx * gx + gy * gy);
    q.count[i] = q.count[i] + 1;
    if (q.max_radius) q.max_radius[i] = fmaxf(q.max_radius[i], (float)(inf.z > inf.w ? inf.z : inf.w));
}

__global__ __launch_bounds__(kThreads) void k_density_inverse(long long n, const int *perm, int *inv)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const long long i = perm[j];
    if (SAS_IN(i, n, 1002)) inv[i] = (int)j;
}

// the class bits of Gaussian i (the rules of DESIGN.md 3, "Density control": every decision on the old set)
DEV unsigned density_class(const SasDensity &q, long long i)
{
    const long long j = q.inv[i];
    if (!SAS_IN(j, q.n_pad, 1003)) return 0u;
    const float o = q.g0[j].w;
    const float4 G = q.g2[j];
    const float smax = q.cov_mode ? 0.0f : fmaxf(fmaxf(G.x, G.y), G.z);
    const int cnt = q.count[i];
    const float avg = q.grad_sum[i] / (float)(cnt > 1 ? cnt : 1);
    const bool high = (q.flags & SAS_DENSIFY_GROW) && cnt > 0 && avg > q.grow_grad2d;
    const bool small = smax <= q.grow_scale;
    const bool prune_o = (q.flags & SAS_DENSIFY_PRUNE_OPACITY) && o < q.prune_opacity;
    const bool prune_s = (q.flags & SAS_DENSIFY_PRUNE_SCALE) && smax > q.prune_scale;
    const bool pruned = prune_o || (prune_s && !(high && !small));
    if (pruned) return 0u;
    return kKept | (high && small ? kClone : 0u) | (high && !small ? kSplit : 0u);
}

__global__ __launch_bounds__(kThreads) void k_density_flag(const SasDensity q)
{
    __shared__ unsigned s_wave[3][kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    const unsigned c = i < q.n ? density_class(q, i) : 0u;
    if (i < q.n) q.cls[i] = (uint8_t)c;
    const unsigned long long mk = __ballot(c & kKept), mc = __ballot(c & kClone), ms = __ballot(c & kSplit);
    if ((tid & 63) == 0) {
        s_wave[0][wv] = (unsigned)__popcll(mk);
        s_wave[1][wv] = (unsigned)__popcll(mc);
        s_wave[2][wv] = (unsigned)__popcll(ms);
    }
    __syncthreads();
    const long long b = blockIdx.x;
    if (tid < 3 && SAS_IN(b, q.nb, 1004)) q.blk_count[tid * q.nb + b] = ((s_wave[tid][0] + s_wave[tid][1]) + s_wave[tid][2]) + s_wave[tid][3];
}

// one workgroup: blk_off <- exclusive offsets of blk_count per class, totals <- (kept, clone candidates, split candidates)
__global__ __launch_bounds__(kThreads) void k_density_scan(const SasDensity q)
{
    __shared__ unsigned s_wave[2][kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    for (int c = 0; c < 3; ++c) {
        unsigned running = 0;
        int slot = 0;
        __syncthreads();   // (the slots of the class before are no longer read)
        for (long long b0 = 0; b0 < q.nb; b0 += kThreads, slot ^= 1) {
            const long long b = b0 + tid;
            const unsigned n = b < q.nb ? q.blk_count[c * q.nb + b] : 0u;
            const unsigned incl = wave_inclusive_sum_u32(n);
            if ((tid & 63) == 63) s_wave[slot][wv] = incl;
            __syncthreads();   // (the slots alternate: one barrier per round)
            unsigned before = 0, total = 0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) {
                before += k < wv ? s_wave[slot][k] : 0u;
                total += s_wave[slot][k];
            }
            if (b < q.nb) q.blk_off[c * q.nb + b] = running + before + (incl - n);
            running += total;
        }
        if (tid == 0) q.totals[c] = running;
    }
}

// ---- the children of a split ------------------------------------------------------------------------------------------------------
// The generator of sas_device.h keyed by (seed, parent, counter).
DEV float density_normal(unsigned seed, unsigned parent, int child, int axis)
{
    const unsigned base = mix32(mix32(seed ^ 0x9e3779b9u) + parent);
    return hashed_normal(base, 2u * (unsigned)(3 * child + axis));
}

// row `pos` of the new scene: Gaussian `i` (old slot j) with the mean and the scale given
DEV void density_emit(const SasDensity &q, long long pos, long long i, long long j, const float4 P, const float4 A, const float4 B,
                      const float *mean, const float *scale)
{
    if (!SAS_IN(pos, q.n_new, 1005)) return;
    q.means[3 * pos] = mean[0]; q.means[3 * pos + 1] = mean[1]; q.means[3 * pos + 2] = mean[2];
    q.opac[pos] = P.w;
    if (q.cov_mode) {
        float *c = q.cov6 + 6 * pos;
        c[0] = A.x; c[1] = A.y; c[2] = A.z; c[3] = A.w; c[4] = B.x; c[5] = B.y;
    } else {
        q.quats[4 * pos] = A.x; q.quats[4 * pos + 1] = A.y; q.quats[4 * pos + 2] = A.z; q.quats[4 * pos + 3] = A.w;
        q.scales[3 * pos] = scale[0]; q.scales[3 * pos + 1] = scale[1]; q.scales[3 * pos + 2] = scale[2];
    }
    float *dst = q.colors + (long long)q.coeff_floats * pos;
    for (int p = 0; p < q.planes; ++p) {
        const float4 C = q.col[(long long)p * q.n_pad + j];
        const float c[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * p + k < q.coeff_floats) dst[4 * p + k] = c[k];
    }
    if (q.gid) q.gid[pos] = q.gid8[j];
    q.parents[pos] = (int)i;
}

__global__ __launch_bounds__(kThreads) void k_density_scatter(const SasDensity q)
{
    __shared__ unsigned s_wave[3][kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    const unsigned c = i < q.n ? q.cls[i] : 0u;
    const unsigned long long mk = __ballot(c & kKept), mc = __ballot(c & kClone), ms = __ballot(c & kSplit);
    if ((tid & 63) == 0) {
        s_wave[0][wv] = (unsigned)__popcll(mk);
        s_wave[1][wv] = (unsigned)__popcll(mc);
        s_wave[2][wv] = (unsigned)__popcll(ms);
    }
    __syncthreads();
    const long long b = blockIdx.x;
    if (!(c & kKept) || !SAS_IN(b, q.nb, 1006)) return;
    long long before[3] = {q.blk_off[b], q.blk_off[q.nb + b], q.blk_off[2 * q.nb + b]};   // kept, clone candidates, split candidates before i
    for (int k = 0; k < wv; ++k) {
        before[0] += s_wave[0][k]; before[1] += s_wave[1][k]; before[2] += s_wave[2][k];
    }
    before[0] += mbcnt64(mk); before[1] += mbcnt64(mc); before[2] += mbcnt64(ms);
    const SasDensityPlan pl = sas_density_plan(q.totals[0], q.totals[1], q.totals[2], q.max_gaussians);
    const bool cloned = (c & kClone) && before[1] < pl.clones, split = (c & kSplit) && before[2] < pl.splits;

    const long long j = q.inv[i];
    if (!SAS_IN(j, q.n_pad, 1007)) return;
    const float4 P = q.g0[j], A = q.g1[j], B = q.g2[j];
    const float mean[3] = {P.x, P.y, P.z}, scale[3] = {B.x, B.y, B.z};
    if (!split) density_emit(q, before[0] - (before[2] < pl.splits ? before[2] : pl.splits), i, j, P, A, B, mean, scale);
    if (cloned) density_emit(q, pl.survivors + before[1], i, j, P, A, B, mean, scale);
    if (split) {
        // R(q / |q|), q = wxyz
        const float inorm = 1.0f / sqrtf((A.x * A.x + A.y * A.y) + (A.z * A.z + A.w * A.w));
        const float w = A.x * inorm, x = A.y * inorm, y = A.z * inorm, z = A.w * inorm;
        const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - w * z), 2.0f * (x * z + w * y),
                            2.0f * (x * y + w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - w * x),
                            2.0f * (x * z - w * y), 2.0f * (y * z + w * x), 1.0f - 2.0f * (x * x + y * y)};
        const float small[3] = {scale[0] / q.split_factor, scale[1] / q.split_factor, scale[2] / q.split_factor};
        for (int ch = 0; ch < 2; ++ch) {
            float d[3], m[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = scale[k] * density_normal(q.seed, (unsigned)i, ch, k);
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = mean[k] + ((R[3 * k] * d[0] + R[3 * k + 1] * d[1]) + R[3 * k + 2] * d[2]);
            density_emit(q, pl.survivors + pl.clones + 2 * before[2] + ch, i, j, P, A, B, m, small);
        }
    }
}

DEV float4 state_or_zero(const float4 *src, long long js, bool fresh) { return fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : src[js]; }

__global__ __launch_bounds__(kThreads) void k_density_state(const SasDensityState q)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // new slot
    if (j >= q.n_new) return;
    const long long i = q.perm_new[j];                                    // new caller's index
    if (!SAS_IN(i, q.n_new, 1011)) return;
    const bool fresh = i >= q.n_survivors;
    const long long p = q.parents[i];
    if (!SAS_IN(p, q.n_old, 1012)) return;
    const long long js = q.inv_old[p];                                    // the parent's old slot
    if (!SAS_IN(js, q.n_pad_old, 1013) || !SAS_IN(j, q.n_pad_new, 1014)) return;
    const SasAdamState &o = q.old_, &s = q.new_;
    if (s.means_m) { s.means_m[j] = state_or_zero(o.means_m, js, fresh); s.means_v[j] = state_or_zero(o.means_v, js, fresh); }
    if (s.quats_m) { s.quats_m[j] = state_or_zero(o.quats_m, js, fresh); s.quats_v[j] = state_or_zero(o.quats_v, js, fresh); }
    if (s.opac) s.opac[j] = fresh ? make_float4(0.0f, 0.0f, raw_opacity(q.g0_new[j].w), 0.0f) : o.opac[js];
    if (s.scales_m) {
        s.scales_m[j] = state_or_zero(o.scales_m, js, fresh);
        s.scales_v[j] = state_or_zero(o.scales_v, js, fresh);
        float4 r = fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : o.scales_raw[js];
        if (fresh) {
            const float4 G = q.g2_new[j];
            r.x = raw_scale(G.x); r.y = raw_scale(G.y); r.z = raw_scale(G.z);
        }
        s.scales_raw[j] = r;
    }
    if (s.sh_m)
        for (int pl = 0; pl < q.planes; ++pl) {
            const long long on = (long long)pl * q.n_pad_new + j, os = (long long)pl * q.n_pad_old + js;
            s.sh_m[on] = state_or_zero(o.sh_m, os, fresh);
            s.sh_v[on] = state_or_zero(o.sh_v, os, fresh);
        }
}

// Behind k_density_state run with n_survivors = n_new (every row takes its parent's state): the rows `mask` marks start anew -- zero
// moments, raw values from the new planes (sas_scene_mcmc_refine: its fresh rows lie among the others).
__global__ __launch_bounds__(kThreads) void k_density_state_fresh(const SasDensityState q, const uint8_t *mask)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // new slot
    if (j >= q.n_new) return;
    const long long i = q.perm_new[j];                                    // new caller's index
    if (!SAS_IN(i, q.n_new, 1015) || !SAS_IN(j, q.n_pad_new, 1016) || !mask[i]) return;
    const SasAdamState &s = q.new_;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (s.means_m) { s.means_m[j] = zero; s.means_v[j] = zero; }
    if (s.quats_m) { s.quats_m[j] = zero; s.quats_v[j] = zero; }
    if (s.opac) s.opac[j] = make_float4(0.0f, 0.0f, raw_opacity(q.g0_new[j].w), 0.0f);
    if (s.scales_m) {
        const float4 G = q.g2_new[j];
        s.scales_m[j] = zero;
        s.scales_v[j] = zero;
        s.scales_raw[j] = make_float4(raw_scale(G.x), raw_scale(G.y), raw_scale(G.z), 0.0f);
    }
    if (s.sh_m)
        for (int pl = 0; pl < q.planes; ++pl) {
            const long long on = (long long)pl * q.n_pad_new + j;
            s.sh_m[on] = zero;
            s.sh_v[on] = zero;
        }
}

__global__ __launch_bounds__(kThreads) void k_opacity_reset(long long n, float cap, float4 *g0, float4 *opac)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    float *o = reinterpret_cast<float *>(g0 + j) + 3;
    if (!(*o > cap)) return;   // (a NaN stays)
    *o = cap;
    if (opac) opac[j] = make_float4(0.0f, 0.0f, raw_opacity(cap), opac[j].w);
}

unsigned grid_of(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_density)

void sas_launch_density_accumulate(hipStream_t st, const SasDensityStats &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_density_accumulate, dim3(grid_of(q.n)), dim3(kThreads), 0, st, q);
}

void sas_launch_density_inverse(hipStream_t st, int64_t n, const int *perm, int *inv)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_density_inverse, dim3(grid_of(n)), dim3(kThreads), 0, st, (long long)n, perm, inv);
}

void sas_launch_density_classes(hipStream_t st, const SasDensity &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_density_inverse, dim3(grid_of(q.n)), dim3(kThreads), 0, st, (long long)q.n, q.perm, q.inv);
    hipLaunchKernelGGL(k_density_flag, dim3((unsigned)q.nb), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(k_density_scan, dim3(1), dim3(kThreads), 0, st, q);
}

void sas_launch_density_scatter(hipStream_t st, const SasDensity &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_density_scatter, dim3((unsigned)q.nb), dim3(kThreads), 0, st, q);
}

void sas_launch_density_state(hipStream_t st, const SasDensityState &q, const uint8_t *fresh)
{
    if (q.n_new <= 0) return;
    SasDensityState all = q;
    if (fresh) all.n_survivors = q.n_new;
    hipLaunchKernelGGL(k_density_state, dim3(grid_of(q.n_new)), dim3(kThreads), 0, st, all);
    if (fresh) hipLaunchKernelGGL(k_density_state_fresh, dim3(grid_of(q.n_new)), dim3(kThreads), 0, st, q, fresh);
}

void sas_launch_opacity_reset(hipStream_t st, int64_t n, float cap, float4 *g0, float4 *opac)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_opacity_reset, dim3(grid_of(n)), dim3(kThreads), 0, st, (long long)n, cap, g0, opac);
}
