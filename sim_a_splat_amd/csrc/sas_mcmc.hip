// sas_mcmc.hip -- MCMC density control on the resident scene (sas_scene_mcmc_noise, sas_scene_mcmc_refine; DESIGN.md 3, "MCMC density
// control"), hand-written for gfx950 (CDNA4, wave64).
//
//   k_mcmc_noise        one lane per storage slot: the mean moves by C (xi g scale), C the Gaussian's own covariance, g the opacity gate,
//                       xi three normals of the generator keyed by (seed, step, CALLER's index, axis).  The hot path: every step.
//   k_mcmc_weights      one lane per Gaussian of the caller's order, 256 per workgroup: the integer sampling weight, and the workgroup's
//                       alive count and weight sum.
//   k_mcmc_scan         ONE workgroup: the workgroup sums -> exclusive offsets (alive counts 32-bit, weights 64-bit), and the totals.
//   k_mcmc_prefix       the grid of k_mcmc_weights again: the inclusive 64-bit prefix of the weights in the caller's order.
//   k_mcmc_draw         one lane per draw: a 64-bit uniform -> target = mulhi(u, total) -> the Gaussian whose prefix interval holds it
//                       (binary search over the workgroup offsets, then inside the workgroup); copies[i] += 1 (an integer atomic: exact).
//   k_mcmc_alive_rows   the grid of k_mcmc_weights again: rank among the alive = offset + rank in workgroup (ballots); the relocated
//                       opacity and scale of a source (binary64), then its row of the new scene.
//   k_mcmc_child_rows   one lane per draw: the child's row, a copy of its source's new row.
//   k_mcmc_identity     parents[i] = i.
// The split between kernels is the one of sas_density.hip: no kernel waits for another workgroup, no look-back.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_); correctly rounded / and sqrt, libm expf / logf / cosf.  The
// relocation alone is binary64 (libm pow, correctly rounded sqrt), rounded once to binary32.
#include <cfloat>

#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kGolden = 0x9e3779b9u;

// C(n, k) for n, k < SAS_MCMC_MAX_N, by Pascal's rule: every entry is an integer below 2^53, exact in binary64
struct Binomials {
    double c[SAS_MCMC_MAX_N][SAS_MCMC_MAX_N];
};
constexpr Binomials pascal()
{
    Binomials b{};
    for (int n = 0; n < SAS_MCMC_MAX_N; ++n) {
        b.c[n][0] = 1.0;
        for (int k = 1; k <= n; ++k) b.c[n][k] = b.c[n - 1][k - 1] + (k < n ? b.c[n - 1][k] : 0.0);
    }
    return b;
}
__constant__ const Binomials kBinom = pascal();

// ---- noise on the means -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mcmc_noise(const SasMcmcNoise q)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // slot
    if (j >= q.n) return;
    const long long i = q.perm[j];                                        // caller's index: the key does not depend on the storage order
    if (!SAS_IN(i, q.n, 1101)) return;
    const float4 P = q.g0[j];
    // gsplat's op_sigmoid; expf overflows to +inf from an opacity of about 0.89 on: g is then exactly 0
    const float g = 1.0f / (1.0f + expf(-100.0f * ((1.0f - P.w) - 0.995f)));
    if (!(g > 0.0f)) return;   // (the mean keeps its bits, -0 included; a NaN opacity moves nothing either)
    const float4 A = q.g1[j], B = q.g2[j];
    float C[6];   // xx xy xz yy yz zz
    if (q.cov_mode) {
        C[0] = A.x; C[1] = A.y; C[2] = A.z; C[3] = A.w; C[4] = B.x; C[5] = B.y;
    } else {
        // R(q / |q|), q = wxyz; M = R diag(s); C = M M^T
        const float inorm = 1.0f / sqrtf((A.x * A.x + A.y * A.y) + (A.z * A.z + A.w * A.w));
        const float w = A.x * inorm, x = A.y * inorm, y = A.z * inorm, z = A.w * inorm;
        const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - w * z), 2.0f * (x * z + w * y),
                            2.0f * (x * y + w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - w * x),
                            2.0f * (x * z - w * y), 2.0f * (y * z + w * x), 1.0f - 2.0f * (x * x + y * y)};
        const float s[3] = {B.x, B.y, B.z};
        float M[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = R[k] * s[k % 3];
        int e = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) C[e++] = (M[3 * r] * M[3 * c] + M[3 * r + 1] * M[3 * c + 1]) + M[3 * r + 2] * M[3 * c + 2];
    }
    const unsigned base = mix32(mix32(mix32(q.seed ^ kGolden) + q.step) + (unsigned)i);
    float n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (hashed_normal(base, 2u * (unsigned)k) * g) * q.scale;
    // (one 16-byte store: w goes back with the bits it came with)
    q.g0[j] = make_float4(P.x + ((C[0] * n[0] + C[1] * n[1]) + C[2] * n[2]), P.y + ((C[1] * n[0] + C[3] * n[1]) + C[4] * n[2]),
                          P.z + ((C[2] * n[0] + C[4] * n[1]) + C[5] * n[2]), P.w);
}

// ---- refine: the alive set and the sampling weights -------------------------------------------------------------------------------
// inclusive prefix sum over the wave's 64 lanes, 64-bit (the refine kernels run on a schedule, not every step: plain shuffles)
DEV unsigned long long wave_inclusive_sum_u64(unsigned long long v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(v, d, 64);
        v += lane >= d ? t : 0ull;
    }
    return v;
}

// alive: o > min_opacity (a NaN is dead)
DEV bool mcmc_alive(const SasMcmc &q, long long i, float &o, long long &j)
{
    j = q.inv[i];
    if (!SAS_IN(j, q.n_pad, 1102)) return false;
    o = q.g0[j].w;
    return o > q.min_opacity;
}

__global__ __launch_bounds__(kThreads) void k_mcmc_weights(const SasMcmc q)
{
    __shared__ unsigned s_alive[kWaves];
    __shared__ unsigned long long s_weight[kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    float o = 0.0f;
    long long j = 0;
    const bool alive = i < q.n && mcmc_alive(q, i, o, j);
    // (a power of two: the product is exact; an opacity above 1 or +Inf is outside the contract and weighs as 1, so the conversion is defined)
    const unsigned w = alive ? (unsigned)(fminf(o, 1.0f) * 16777216.0f) : 0u;
    if (i < q.n) q.weight[i] = w;
    const unsigned long long ma = __ballot(alive);
    const unsigned long long incl = wave_inclusive_sum_u64(w);
    if ((tid & 63) == 63) {
        s_alive[wv] = (unsigned)__popcll(ma);
        s_weight[wv] = incl;
    }
    __syncthreads();
    const long long b = blockIdx.x;
    if (tid == 0 && SAS_IN(b, q.nb, 1103)) {
        q.blk_alive[b] = ((s_alive[0] + s_alive[1]) + s_alive[2]) + s_alive[3];
        q.blk_weight[b] = ((s_weight[0] + s_weight[1]) + s_weight[2]) + s_weight[3];
    }
}

// one workgroup: the exclusive offsets of blk_alive and blk_weight, totals <- (alive, weight)
__global__ __launch_bounds__(kThreads) void k_mcmc_scan(const SasMcmc q)
{
    __shared__ unsigned long long s_wave[2][2][kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    unsigned long long run_a = 0, run_w = 0;
    int slot = 0;
    for (long long b0 = 0; b0 < q.nb; b0 += kThreads, slot ^= 1) {
        const long long b = b0 + tid;
        const unsigned long long a = b < q.nb ? q.blk_alive[b] : 0u, w = b < q.nb ? q.blk_weight[b] : 0ull;
        const unsigned long long ia = wave_inclusive_sum_u64(a), iw = wave_inclusive_sum_u64(w);
        if ((tid & 63) == 63) {
            s_wave[slot][0][wv] = ia;
            s_wave[slot][1][wv] = iw;
        }
        __syncthreads();   // (the slots alternate: one barrier per round)
        unsigned long long before_a = 0, before_w = 0, total_a = 0, total_w = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            before_a += k < wv ? s_wave[slot][0][k] : 0ull;
            before_w += k < wv ? s_wave[slot][1][k] : 0ull;
            total_a += s_wave[slot][0][k];
            total_w += s_wave[slot][1][k];
        }
        if (b < q.nb) {
            q.blk_alive_off[b] = (unsigned)(run_a + before_a + (ia - a));
            q.blk_weight_off[b] = run_w + before_w + (iw - w);
        }
        run_a += total_a;
        run_w += total_w;
    }
    if (tid == 0) {
        q.totals[0] = run_a;
        q.totals[1] = run_w;
    }
}

__global__ __launch_bounds__(kThreads) void k_mcmc_prefix(const SasMcmc q)
{
    __shared__ unsigned long long s_weight[kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    const unsigned long long incl = wave_inclusive_sum_u64(i < q.n ? q.weight[i] : 0u);
    if ((tid & 63) == 63) s_weight[wv] = incl;
    __syncthreads();
    const long long b = blockIdx.x;
    if (i >= q.n || !SAS_IN(b, q.nb, 1104)) return;
    unsigned long long before = q.blk_weight_off[b];
    for (int k = 0; k < wv; ++k) before += s_weight[k];
    q.prefix[i] = before + incl;
}

// ---- refine: the draws ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_mcmc_draw(const SasMcmc q)
{
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (d >= q.draws) return;
    const unsigned base = mix32(mix32(q.seed ^ kGolden) + (unsigned)d);
    const unsigned long long u = ((unsigned long long)mix32(base ^ kGolden) << 32) | mix32(base ^ (2u * kGolden));
    const unsigned long long t = __umul64hi(u, q.total_weight);   // in [0, total)
    // the last workgroup whose offset is <= t (the empty ones behind it share the next one's offset) ...
    long long lo = 0, hi = q.nb - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (q.blk_weight_off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    // ... and in it the first Gaussian whose inclusive prefix is > t
    long long a = lo * kThreads, z = a + kThreads - 1 < q.n - 1 ? a + kThreads - 1 : q.n - 1;
    while (a < z) {
        const long long mid = (a + z) >> 1;
        if (q.prefix[mid] > t) z = mid;
        else a = mid + 1;
    }
    if (!SAS_IN(a, q.n, 1105)) return;
    q.source[d] = (int)a;
    atomicAdd(&q.copies[a], 1u);
}

// ---- refine: relocation and the rows of the new scene -----------------------------------------------------------------------------
// gsplat's compute_relocation for a source selected `copies` times: it becomes n = min(copies + 1, 51) Gaussians of opacity
// o' = 1 - (1 - o)^(1/n) and scale (o / denom) scale, denom = sum_{i=1..n} sum_{k<i} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1).  The
// alternating sum cancels: binary64, in this fixed order, rounded once.
DEV float4 mcmc_relocate(float o, unsigned copies, float min_opacity, const float4 B)
{
    const int n = (int)(copies < (unsigned)SAS_MCMC_MAX_N - 1u ? copies + 1u : (unsigned)SAS_MCMC_MAX_N);
    const double od = (double)o;
    const double on = 1.0 - pow(1.0 - od, 1.0 / (double)n);
    double denom = 0.0;
    for (int i = 1; i <= n; ++i) {
        double p = on;   // o'^(k+1)
        for (int k = 0; k < i; ++k) {
            denom += (kBinom.c[i - 1][k] * ((k & 1) ? -p : p)) / sqrt((double)(k + 1));
            p *= on;
        }
    }
    const float ratio = (float)(od / denom);
    return make_float4(fminf(fmaxf((float)on, min_opacity), 1.0f - FLT_EPSILON), ratio * B.x, ratio * B.y, ratio * B.z);
}

// row `pos` of the new scene: Gaussian `i` (old slot j), with the opacity and scale of X where it is a source or a child
DEV void mcmc_emit(const SasMcmc &q, long long pos, long long i, long long j, bool fresh, const float4 X)
{
    if (!SAS_IN(pos, q.n_new, 1106) || !SAS_IN(j, q.n_pad, 1107)) return;
    const float4 P = q.g0[j], A = q.g1[j], B = q.g2[j];
    q.means[3 * pos] = P.x; q.means[3 * pos + 1] = P.y; q.means[3 * pos + 2] = P.z;
    q.opac[pos] = fresh ? X.x : P.w;
    q.quats[4 * pos] = A.x; q.quats[4 * pos + 1] = A.y; q.quats[4 * pos + 2] = A.z; q.quats[4 * pos + 3] = A.w;
    q.scales[3 * pos] = fresh ? X.y : B.x; q.scales[3 * pos + 1] = fresh ? X.z : B.y; q.scales[3 * pos + 2] = fresh ? X.w : B.z;
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
    q.fresh[pos] = fresh ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_mcmc_alive_rows(const SasMcmc q)
{
    __shared__ unsigned s_alive[kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    float o = 0.0f;
    long long j = 0;
    const bool alive = i < q.n && mcmc_alive(q, i, o, j);
    const unsigned long long ma = __ballot(alive);
    if ((tid & 63) == 0) s_alive[wv] = (unsigned)__popcll(ma);
    __syncthreads();
    const long long b = blockIdx.x;
    if (!alive || !SAS_IN(b, q.nb, 1108)) return;
    long long pos = q.blk_alive_off[b];
    for (int k = 0; k < wv; ++k) pos += s_alive[k];
    pos += mbcnt64(ma);
    const unsigned copies = q.copies[i];
    float4 X = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (copies > 0u) {
        X = mcmc_relocate(o, copies, q.min_opacity, q.g2[j]);
        q.reloc[i] = X;
    }
    mcmc_emit(q, pos, i, j, copies > 0u, X);
}

__global__ __launch_bounds__(kThreads) void k_mcmc_child_rows(const SasMcmc q)
{
    const long long d = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (d >= q.draws) return;
    const long long i = q.source[d];
    if (!SAS_IN(i, q.n, 1109)) return;
    mcmc_emit(q, q.n_alive + d, i, q.inv[i], true, q.reloc[i]);
}

__global__ __launch_bounds__(kThreads) void k_mcmc_identity(long long n, int *parents)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) parents[i] = (int)i;
}

unsigned grid_of(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_mcmc)

void sas_launch_mcmc_noise(hipStream_t st, const SasMcmcNoise &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_mcmc_noise, dim3(grid_of(q.n)), dim3(kThreads), 0, st, q);
}

void sas_launch_mcmc_weights(hipStream_t st, const SasMcmc &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_mcmc_weights, dim3((unsigned)q.nb), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(k_mcmc_scan, dim3(1), dim3(kThreads), 0, st, q);
}

void sas_launch_mcmc_rows(hipStream_t st, const SasMcmc &q)
{
    if (q.n <= 0 || q.draws <= 0) return;
    hipLaunchKernelGGL(k_mcmc_prefix, dim3((unsigned)q.nb), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(k_mcmc_draw, dim3(grid_of(q.draws)), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(k_mcmc_alive_rows, dim3((unsigned)q.nb), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(k_mcmc_child_rows, dim3(grid_of(q.draws)), dim3(kThreads), 0, st, q);
}

void sas_launch_mcmc_identity(hipStream_t st, int64_t n, int *parents)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_mcmc_identity, dim3(grid_of(n)), dim3(kThreads), 0, st, (long long)n, parents);
}
