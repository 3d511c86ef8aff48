// sas_order.hip -- the storage order of a scene on the device (sas_storage_order, and the tail of sas_scene_upload, sas_scene_densify and
// sas_scene_mcmc_refine; DESIGN.md 3, "Storage order"), hand-written for gfx950 (CDNA4, wave64).  The result is the permutation
// storage_order() of sas_api.cpp gives on the host, bit for bit: slot -> caller's index, ordered by (group, 10-bit-per-axis Hilbert index
// of the mean, caller's index).
//
//   k_order_bounds       kOrderTile Gaussians per workgroup: the minimum and maximum of the finite coordinates per axis, and the smallest index
//                        whose group id is >= n_groups, as one partial record per workgroup (wave reductions, then the four waves in LDS).
//   k_order_bounds_tail  ONE workgroup: the partial records -> lo[3], hi[3], inv[3], and the first bad index with its id.
//   k_order_keys         one lane per Gaussian: the quantised mean, its Hilbert index (Skilling's transform), key = group << 32 | index.
//   k_order_hist         pass p of the sort: the histogram of digit p over each workgroup's tile of kOrderTile keys, table[digit][workgroup].
//   k_order_scan         ONE workgroup: the table, digit-major, -> exclusive offsets, kOrderScanRound entries per round.
//   k_order_scatter      the grid of k_order_hist again: a key goes to table offset + its rank among the keys of its digit in the tile, in
//                        input order (per-wave counts from ballots, as lds_radix_sort of sas_tile.hip).
// The sort is a least-significant-digit radix sort with 8-bit digits: four passes over the 30 Hilbert bits, a fifth over the group byte
// when the scene has groups.  Every pass is STABLE, so equal keys stay in ascending caller's index: the host comparator's third key.
// As in sas_density.hip: no kernel waits for another workgroup, no look-back, no global atomics; the LDS counters of k_order_hist are
// sums, whose final value does not depend on the order of arrival.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_), correctly rounded /: the host's expressions in the host's order.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = SAS_ORDER_TILE;              // keys per workgroup of a sort pass, Gaussians per workgroup of k_order_bounds
constexpr int kBatches = kTile / kThreads;         // 64-key batches per wave
constexpr int kScanRound = SAS_ORDER_SCAN_ROUND;   // table entries k_order_scan takes per round: four per lane
static_assert(kTile % kThreads == 0 && kScanRound == 4 * kThreads, "the tile is whole batches, a scan round four entries per lane");

DEV bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// a float as an int that orders the same way (its own inverse); -0 sorts below +0
DEV int ordered_i32(float v)
{
    const int b = (int)__float_as_uint(v);
    return b ^ ((b >> 31) & 0x7fffffff);
}
DEV float ordered_f32(int o) { return __uint_as_float((unsigned)(o ^ ((o >> 31) & 0x7fffffff))); }

// Minimum and maximum do not depend on the order of the reduction -- with one exception: of +0 and -0 either may come out, where the
// host keeps the one it met first.  The sign of a zero bound cannot change a key: v - lo and hi - lo differ by it only where they are
// zero, a zero product quantises to 0 whatever its sign, and hi > lo does not see it.
__global__ __launch_bounds__(kThreads) void k_order_bounds(const SasOrder q)
{
    __shared__ int s_part[kWaves][SAS_ORDER_PARTIAL];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0x7fffffff;
    const long long base = (long long)blockIdx.x * kTile;
#pragma unroll
    for (int b = 0; b < kBatches; ++b) {
        const long long i = base + b * kThreads + tid;
        if (i >= q.n) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = q.means[3 * i + k];
            if (finite_f32(v)) { lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); }
        }
        if (q.gid && (int)q.gid[i] >= q.n_groups && (int)i < bad) bad = (int)i;
    }
    int part[SAS_ORDER_PARTIAL];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        part[k] = wave_min_i32(ordered_i32(lo[k]));
        part[3 + k] = wave_max_i32(ordered_i32(hi[k]));
    }
    part[6] = wave_min_i32(bad);
    part[7] = 0;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < SAS_ORDER_PARTIAL; ++k) s_part[wv][k] = part[k];
    __syncthreads();
    if (tid < SAS_ORDER_PARTIAL && SAS_IN(blockIdx.x, q.n_tiles, 1301)) {
        int v = s_part[0][tid];
        const bool is_max = tid >= 3 && tid < 6;
        for (int w = 1; w < kWaves; ++w) v = is_max ? max(v, s_part[w][tid]) : min(v, s_part[w][tid]);
        q.partial[(long long)blockIdx.x * SAS_ORDER_PARTIAL + tid] = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_order_bounds_tail(const SasOrder q)
{
    __shared__ int s_part[kWaves][SAS_ORDER_PARTIAL];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int part[SAS_ORDER_PARTIAL];
#pragma unroll
    for (int k = 0; k < SAS_ORDER_PARTIAL; ++k) part[k] = (k >= 3 && k < 6) ? (int)0x80000000 : 0x7fffffff;
    for (long long t = tid; t < q.n_tiles; t += kThreads)
#pragma unroll
        for (int k = 0; k < SAS_ORDER_PARTIAL; ++k) {
            const int v = q.partial[t * SAS_ORDER_PARTIAL + k];
            part[k] = (k >= 3 && k < 6) ? max(part[k], v) : min(part[k], v);
        }
#pragma unroll
    for (int k = 0; k < SAS_ORDER_PARTIAL; ++k) part[k] = (k >= 3 && k < 6) ? wave_max_i32(part[k]) : wave_min_i32(part[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < SAS_ORDER_PARTIAL; ++k) s_part[wv][k] = part[k];
    __syncthreads();
    if (tid < 3) {
        int l = s_part[0][tid], h = s_part[0][3 + tid];
        for (int w = 1; w < kWaves; ++w) { l = min(l, s_part[w][tid]); h = max(h, s_part[w][3 + tid]); }
        const float lo = ordered_f32(l), hi = ordered_f32(h);
        q.rec->lo[tid] = lo;
        q.rec->hi[tid] = hi;
        q.rec->inv[tid] = hi > lo ? 1023.0f / (hi - lo) : 0.0f;
    }
    if (tid == 3) {
        int bad = s_part[0][6];
        for (int w = 1; w < kWaves; ++w) bad = min(bad, s_part[w][6]);
        const bool any = q.gid && bad < q.n;
        q.rec->bad_index = any ? bad : -1;
        q.rec->bad_id = any ? (int)q.gid[bad] : 0;
    }
}

// 3-D Hilbert index of 10 bits per axis: hilbert3 of sas_api.cpp, unrolled
DEV unsigned hilbert3_10(unsigned x, unsigned y, unsigned z)
{
    unsigned X[3] = {x, y, z};
#pragma unroll
    for (unsigned Q = 512u; Q > 1u; Q >>= 1) {
        const unsigned P = Q - 1u;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (X[i] & Q) X[0] ^= P;
            else { const unsigned t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    unsigned t = 0u;
#pragma unroll
    for (unsigned Q = 512u; Q > 1u; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1u;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] ^= t;
    unsigned code = 0u;
#pragma unroll
    for (int b = 9; b >= 0; --b)
#pragma unroll
        for (int i = 0; i < 3; ++i) code = (code << 1) | ((X[i] >> b) & 1u);
    return code;
}

__global__ __launch_bounds__(kThreads) void k_order_keys(const SasOrder q)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.n) return;
    unsigned c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = q.means[3 * i + k];
        const float u = finite_f32(v) ? (v - q.rec->lo[k]) * q.rec->inv[k] : 0.0f;
        // the host's min(max(u, 0), 1023), written so that a NaN (inf * 0 once hi - lo has overflowed) becomes 0 in front of the conversion
        c[k] = (unsigned)(u > 0.0f ? (u < 1023.0f ? u : 1023.0f) : 0.0f);
    }
    const unsigned long long g = q.gid ? q.gid[i] : 0u;
    q.key[0][i] = (g << 32) | hilbert3_10(c[0], c[1], c[2]);
}

DEV unsigned digit_of(unsigned long long key, int shift) { return (unsigned)(key >> shift) & 255u; }

__global__ __launch_bounds__(kThreads) void k_order_hist(const SasOrder q, const unsigned long long *key, int shift)
{
    __shared__ unsigned s_hist[256];
    const int tid = threadIdx.x;
    s_hist[tid] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kTile;
#pragma unroll
    for (int b = 0; b < kBatches; ++b) {
        const long long i = base + b * kThreads + tid;
        if (i < q.n) atomicAdd(&s_hist[digit_of(key[i], shift)], 1u);   // (LDS; a sum: the order of arrival does not reach it)
    }
    __syncthreads();
    if (SAS_IN(blockIdx.x, q.n_tiles, 1302)) q.table[(long long)tid * q.n_tiles + blockIdx.x] = s_hist[tid];
}

// one workgroup: table[256 n_tiles] <- its exclusive prefix sums, in place.  Lane t of a round takes entries 4 t .. 4 t + 3.
__global__ __launch_bounds__(kThreads) void k_order_scan(const SasOrder q)
{
    __shared__ unsigned s_wave[2][kWaves];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long m = 256ll * q.n_tiles;   // a multiple of 4, and the table 16-byte aligned: a lane's four entries are all inside or all outside
    unsigned running = 0;
    int slot = 0;
    for (long long e0 = 0; e0 < m; e0 += kScanRound, slot ^= 1) {
        const long long e = e0 + 4 * tid;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (e < m) v = *reinterpret_cast<const uint4 *>(q.table + e);
        const unsigned n = (v.x + v.y) + (v.z + v.w);
        const unsigned incl = wave_inclusive_sum_u32(n);
        if ((tid & 63) == 63) s_wave[slot][wv] = incl;
        __syncthreads();   // (the slots alternate: one barrier per round)
        unsigned before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            before += k < wv ? s_wave[slot][k] : 0u;
            total += s_wave[slot][k];
        }
        const unsigned x0 = running + before + (incl - n);
        if (e < m) *reinterpret_cast<uint4 *>(q.table + e) = make_uint4(x0, x0 + v.x, x0 + v.x + v.y, x0 + v.x + v.y + v.z);
        running += total;
    }
}

// Wave w of the workgroup takes the tile's keys [w kBatches 64, (w + 1) kBatches 64), batch by batch: input order is (wave, batch, lane).
// in_idx nullptr: the first pass, whose indices are the positions; out_key nullptr: the last, whose keys nobody reads.
__global__ __launch_bounds__(kThreads) void k_order_scatter(const SasOrder q, const unsigned long long *in_key, const int *in_idx,
                                                            unsigned long long *out_key, int *out_idx, int shift)
{
    __shared__ unsigned s_cnt[kWaves][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int d = lane; d < 256; d += 64) s_cnt[wv][d] = 0u;
    const long long base = (long long)blockIdx.x * kTile + (long long)wv * (kBatches * 64) + lane;
    unsigned long long key[kBatches];
    int idx[kBatches];
    unsigned rank[kBatches];
#pragma unroll
    for (int b = 0; b < kBatches; ++b) {
        const long long i = base + 64 * b;
        const bool act = i < q.n;
        key[b] = act ? in_key[i] : ~0ull;
        idx[b] = act ? (in_idx ? in_idx[i] : (int)i) : -1;
    }
#pragma unroll
    for (int b = 0; b < kBatches; ++b) {
        const bool act = base + 64 * b < q.n;
        const unsigned d = digit_of(key[b], shift);
        unsigned long long mm = __ballot(act);   // the lanes of this batch with this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long bm = __ballot(on);
            mm &= on ? bm : ~bm;
        }
        const unsigned below = mbcnt64(mm), total = (unsigned)__popcll(mm);
        const unsigned prev = act ? s_cnt[wv][d] : 0u;
        if (act && below == 0u) s_cnt[wv][d] = prev + total;   // (the wave's own row, in program order: no other wave touches it)
        rank[b] = prev + below;
    }
    __syncthreads();
    {   // the waves' counts of digit `tid` -> what the waves before hold of it
        unsigned run = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { const unsigned c = s_cnt[w][tid]; s_cnt[w][tid] = run; run += c; }
    }
    __syncthreads();
    if (!SAS_IN(blockIdx.x, q.n_tiles, 1303)) return;
#pragma unroll
    for (int b = 0; b < kBatches; ++b) {
        if (base + 64 * b >= q.n) continue;
        const unsigned d = digit_of(key[b], shift);
        const long long pos = (long long)q.table[(long long)d * q.n_tiles + blockIdx.x] + s_cnt[wv][d] + rank[b];
        if (!SAS_IN(pos, q.n, 1304) || pos >= q.n) continue;   // (the offsets are a partition of [0, n): checked in the product build too, nothing is written beyond it)
        if (out_key) out_key[pos] = key[b];
        out_idx[pos] = idx[b];
    }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_order)

// the bounds alone: q.rec <- lo, hi, inv and the first bad group id (sas_knn.hip lays its grid over them)
void sas_launch_order_bounds(hipStream_t st, const SasOrder &q)
{
    if (q.n <= 0) return;
    const dim3 tiles((unsigned)q.n_tiles), wg(kThreads);
    hipLaunchKernelGGL(k_order_bounds, tiles, wg, 0, st, q);
    hipLaunchKernelGGL(k_order_bounds_tail, dim3(1), wg, 0, st, q);
}

void sas_launch_order(hipStream_t st, const SasOrder &q)
{
    if (q.n <= 0) return;
    const dim3 tiles((unsigned)q.n_tiles), wg(kThreads);
    sas_launch_order_bounds(st, q);
    hipLaunchKernelGGL(k_order_keys, dim3((unsigned)((q.n + kThreads - 1) / kThreads)), wg, 0, st, q);
    const int passes = q.gid ? 5 : 4;   // bytes 0 .. 3 hold the 30 Hilbert bits, byte 4 the group
    for (int p = 0; p < passes; ++p) {
        const bool last = p == passes - 1;
        const unsigned long long *in_key = q.key[p & 1];
        hipLaunchKernelGGL(k_order_hist, tiles, wg, 0, st, q, in_key, 8 * p);
        hipLaunchKernelGGL(k_order_scan, dim3(1), wg, 0, st, q);
        hipLaunchKernelGGL(k_order_scatter, tiles, wg, 0, st, q, in_key, p == 0 ? (const int *)nullptr : (const int *)q.idx[p & 1],
                           last ? (unsigned long long *)nullptr : q.key[(p + 1) & 1], last ? q.perm : q.idx[(p + 1) & 1], 8 * p);
    }
}
