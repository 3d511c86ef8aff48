// sas_knn.hip -- for every point of one cloud its k nearest OTHER points of the same cloud, exactly (sas_knn_points; DESIGN.md 3, "Scene from
// points"), hand-written for gfx950 (CDNA4, wave64).  It is the one step of the published scene initialisation that is not elementwise: the
// isotropic scale of a new Gaussian is the RMS distance to its three nearest neighbours.
//
// The contract (tests/tools/knn_ref.py restates it): d2 = (dx dx + dy dy) + dz dz in IEEE binary32, nothing fused, d = q - p for the candidate q
// of the point p; candidates are compared by the key bits(d2) << 32 | j and the k smallest keys win, in ascending order; the point itself is
// left out BY INDEX; a candidate whose d2 is NaN or +inf never counts (so neither does one with a non-finite coordinate, and a point with a
// non-finite coordinate of its own has no neighbours); a missing neighbour reads dist2 = +inf, index = -1.
//
//   k_knn_occupancy  one lane per point: its bit in a 32^3 occupancy mask over the bounds sas_launch_order_bounds found (integer OR).
//   k_knn_grid       ONE workgroup: occupied coarse cells at 32^3 and 16^3 -> the grid's cell edge and dimensions (the rule: below), under the
//                    table budget; the record every later kernel reads.
//   k_knn_count      one lane per point: table[cell] += 1 (integer atomics: sums); the non-finite points count in cell n_cells.
//   k_knn_scan_a/b/c block sums, ONE workgroup over the block sums, starts per cell: three launches, no kernel waits for another workgroup.
//   k_knn_scatter    one lane per point: pts[table[cell]++] = (x, y, z, bits(index)).  The order inside a cell is the order of arrival -- it
//                    reaches no result, because a result is the k smallest KEYS of a set.  Afterwards table[c] is the END of cell c.
//   k_knn_search<K>  one lane per point IN CELL ORDER, so that the lanes of a wave walk the same cells: Chebyshev rings r = 0, 1, .. of cells
//                    around its own, the K best keys in registers, and the stop rule below.  A lane still searching behind ring
//                    SAS_KNN_RING_LIMIT appends itself to the leftover list (one integer atomic per wave).
//   k_knn_brute<K>   grid (blocks of 256 leftover points, slices of the cloud), k_match_slice's form: the candidates pass through LDS in chunks
//                    and every lane reads the same address.  Far outliers, grossly non-uniform clouds and SAS_KNN_GRID=1 take this path; it
//                    is right at any leftover count, the whole cloud included.
//   k_knn_merge<K>   one lane per leftover point: the K smallest keys over its slices, and the rows of the result.
// K is 3 (k <= 3) or 8: the first k of the K smallest keys ARE the k smallest, and a stop rule on the K-th key is only more careful.
//
// THE STOP RULE.  cell(v) = min((int)fl(fl(v - lo) inv), n - 1) per axis, with at most SAS_KNN_MAX_AXIS cells.  Behind ring r a lane whose
// point p lies in cell c has seen every point of the cells [c - r, c + r]^3.  Let q be a point outside that box: on some axis its cell is
// m >= c + r + 1 or m <= c - r - 1.  With u = 2^-24 and h = 1 / inv (the real reciprocal of the float inv):
//   upper side: fl(fl(q - lo) inv) >= m  =>  fl(q - lo) inv >= m (1 - u)  =>  q - lo >= m h (1 - u) / (1 + u) >= m h (1 - 2 u);
//               fl(fl(p - lo) inv) < c + 1 =>  fl(p - lo) inv < c + 1 (rounding is monotone, c + 1 a float) => p - lo < (c + 1) h (1 + 2.01 u);
//               q - p > h (r - 4.01 u (c + r + 1)),
//   lower side: the same with the roles exchanged, q - p < -h (r - 4.01 u c)   (the clamp to n - 1 only moves p's cell DOWN to c: fl(..) >= c holds).
// Cell indices stay below 1024, so 4.01 u 1024 < 2^-10 and |q - p| > (r - 2^-10) h in real numbers.  The kernel's bound is the float
//   b = fl((r - 2^-10) h_lo),  h_lo = fl(hf (1 - 2^-20)),  inv = fl(1 / hf):
// inv = (1 + e) / hf with |e| <= u (a correctly rounded division), so h >= hf (1 - 1.01 u), while h_lo <= hf (1 - 2^-20)(1 + u) and b picks up
// one more (1 + u): b <= (r - 2^-10) hf (1 - 16 u)(1 + u)^2 < (r - 2^-10) h.  r - 2^-10 is exact in binary32 (r <= 64).
// From a float b <= |q_k - p_k| to the kernel's d2, by monotonicity alone (no error terms, denormals included): rounding is monotone and b is a
// float, so |fl(q_k - p_k)| >= b; then fl(d_k d_k) >= fl(b b); and adding non-negative floats never rounds below an addend, so
// d2 >= fl(d_k d_k) >= fl(b b).  A lane stops behind ring r when its K-th d2 is STRICTLY below fl(b b): every unseen point then has a larger key
// whatever its index.  (Equal would not do: an unseen point at the same d2 may have the lower index.)  r = 0 never stops.
//
// THE GRID RULE (k_knn_grid).  Cubic cells of edge h = E / g over the finite bounds, E their largest extent.  A depth camera's cloud is a
// surface, so N / g^3 says nothing about how full a cell is.  The rule measures instead: M32 and M16, the occupied cells of a 32^3 and a 16^3
// grid over the bounds, give the cloud's box dimension d = log2(M32 / M16) (clamped to [1, 3]: 2 for a surface, 3 for a volume), so a grid of
// g cells per axis has about M32 (g / 32)^d occupied cells, and g = 32 (N / (T M32))^(1/d) leaves T = 3 points per occupied cell.  g is
// clamped to [1, 1024]; while the cells outnumber the table budget (min(2^21, max(4096, 2 N))) h grows by 1.26.  None of this is exact
// arithmetic and none of it has to be: no result depends on the grid.
// Arithmetic of the results: IEEE binary32, nothing fused (-ffp-contract=off, no fma_).
// The keys' helpers (kKnnNone, keep_key, finite3) live in sas_device.h: sas_skin.hip's k_knn_cross extends this contract to a second cloud.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlock = SAS_KNN_SCAN_BLOCK;
constexpr int kCoarse = SAS_KNN_COARSE;
constexpr float kTargetPerCell = 3.0f;
static_assert(kBlock == 8 * kThreads && SAS_KNN_CHUNK == kThreads && kCoarse == 32, "eight table entries per lane, one candidate per thread of a chunk, one word per coarse row");
static_assert(SAS_KNN_RING_LIMIT <= 64 && SAS_KNN_MAX_AXIS <= 1024, "the stop bound's margin is derived for these");

// the cell of a finite coordinate on an axis of n cells (monotone in v: the stop rule rests on it)
DEV int cell_axis(float v, float lo, float inv, int n)
{
    const float t = (v - lo) * inv;
    const int c = (int)(t > 0.0f ? (t < (float)(SAS_KNN_MAX_AXIS - 1) ? t : (float)(SAS_KNN_MAX_AXIS - 1)) : 0.0f);   // (a NaN becomes 0)
    return c < n - 1 ? c : n - 1;
}
DEV long long cell_of(const SasKnnGrid &G, float x, float y, float z)
{
    const int cx = cell_axis(x, G.lo[0], G.inv, G.n[0]), cy = cell_axis(y, G.lo[1], G.inv, G.n[1]), cz = cell_axis(z, G.lo[2], G.inv, G.n[2]);
    return ((long long)cz * G.n[1] + cy) * G.n[0] + cx;
}

__global__ __launch_bounds__(kThreads) void k_knn_occupancy(const SasKnn q)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.n) return;
    const float x = q.points[3 * i], y = q.points[3 * i + 1], z = q.points[3 * i + 2];
    if (!finite3(x, y, z)) return;
    const float *lo = q.bounds->lo, *hi = q.bounds->hi;
    const float e = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    const float inv = (e > 0.0f && e < INFINITY) ? (float)kCoarse / e : 0.0f;
    const int cx = cell_axis(x, lo[0], inv, kCoarse), cy = cell_axis(y, lo[1], inv, kCoarse), cz = cell_axis(z, lo[2], inv, kCoarse);
    const int w = cz * kCoarse + cy;
    const unsigned bit = 1u << cx;
    // (the plain read may be stale: then the OR is repeated, nothing else)
    if (SAS_IN(w, kCoarse * kCoarse, 1401) && !(q.occ[w] & bit)) atomicOr(&q.occ[w], bit);
}

__global__ __launch_bounds__(kThreads) void k_knn_grid(const SasKnn q)
{
    __shared__ int s_m[2];
    const int tid = threadIdx.x;
    if (tid < 2) s_m[tid] = 0;
    __syncthreads();
    {   // thread (Z, Y) of 16 x 16: the four words of its 2 x 2 coarse rows
        const int Z = tid >> 4, Y = tid & 15;
        const unsigned w0 = q.occ[(2 * Z) * kCoarse + 2 * Y], w1 = q.occ[(2 * Z) * kCoarse + 2 * Y + 1];
        const unsigned w2 = q.occ[(2 * Z + 1) * kCoarse + 2 * Y], w3 = q.occ[(2 * Z + 1) * kCoarse + 2 * Y + 1];
        unsigned u = (w0 | w1) | (w2 | w3);
        u = (u | (u >> 1)) & 0x55555555u;
        atomicAdd(&s_m[0], __popc(w0) + __popc(w1) + __popc(w2) + __popc(w3));   // (LDS; integer sums)
        atomicAdd(&s_m[1], __popc(u));
    }
    __syncthreads();
    if (tid != 0) return;
    const float *lo = q.bounds->lo, *hi = q.bounds->hi;
    float ext[3], emax = 0.0f;
    bool ok = q.forced_g != 1;
    for (int k = 0; k < 3; ++k) {
        ok = ok && hi[k] >= lo[k];   // (false where no coordinate of the axis is finite)
        ext[k] = hi[k] - lo[k];
        emax = fmaxf(emax, ext[k]);
    }
    ok = ok && emax > 0.0f && emax < INFINITY;
    int n[3] = {1, 1, 1};
    float h = 1.0f, inv = 0.0f;
    if (ok) {
        float g;
        if (q.forced_g > 0) g = (float)q.forced_g;
        else {
            const float m32 = (float)max(s_m[0], 1), m16 = (float)max(s_m[1], 1);
            const float d = fminf(fmaxf(log2f(m32 / m16), 1.0f), 3.0f);
            g = (float)kCoarse * powf((float)q.n / (kTargetPerCell * m32), 1.0f / d);
        }
        g = fminf(fmaxf(g, 1.0f), (float)SAS_KNN_MAX_AXIS);
        h = emax / g;
        ok = false;
        for (int it = 0; it < 64 && !ok; ++it) {
            inv = 1.0f / h;
            if (h >= 1e-30f && inv > 0.0f && inv < INFINITY) {
                long long cells = 1;
                for (int k = 0; k < 3; ++k) {
                    n[k] = (int)fminf(ext[k] * inv, (float)(SAS_KNN_MAX_AXIS - 1)) + 1;
                    if (q.forced_g > 0) n[k] = min(n[k], q.forced_g);
                    cells *= n[k];
                }
                ok = cells <= q.cells_cap;
            }
            if (!ok) h = h * 1.26f;
        }
    }
    SasKnnGrid G;
    for (int k = 0; k < 3; ++k) {
        G.lo[k] = ok ? lo[k] : 0.0f;
        G.n[k] = ok ? n[k] : 1;
    }
    G.inv = ok ? inv : 0.0f;
    G.h_lo = ok ? h * (1.0f - 9.5367431640625e-7f) : 0.0f;   // (2^-20)
    G.n_cells = G.n[0] * G.n[1] * G.n[2];
    G.brute = (!ok || G.n_cells == 1) ? 1 : 0;
    G.left_count = 0u;
    G.occupied[0] = s_m[0];
    G.occupied[1] = s_m[1];
    *q.grid = G;
}

__global__ __launch_bounds__(kThreads) void k_knn_count(const SasKnn q)
{
    const SasKnnGrid &G = *q.grid;
    if (G.brute) return;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.n) return;
    const float x = q.points[3 * i], y = q.points[3 * i + 1], z = q.points[3 * i + 2];
    const long long c = finite3(x, y, z) ? cell_of(G, x, y, z) : (long long)G.n_cells;
    if (SAS_IN(c, q.cells_cap + 1, 1402) && c <= q.cells_cap) atomicAdd(&q.table[c], 1u);   // (a sum: the order of arrival does not reach it)
}

// the workgroup's exclusive prefix of v (one value per thread) and the workgroup's total; s_wave: kWaves words nobody else is using
DEV unsigned wg_exclusive_sum(unsigned v, unsigned *s_wave, int tid, unsigned &total)
{
    const unsigned incl = wave_inclusive_sum_u32(v);
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    unsigned before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        before += w < (tid >> 6) ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    return before + (incl - v);
}

DEV void load8(const unsigned *p, unsigned (&v)[8])
{
    const uint4 a = *reinterpret_cast<const uint4 *>(p), b = *reinterpret_cast<const uint4 *>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// blk[b] <- the sum of block b's kBlock table entries (the table is 16-byte aligned and whole blocks long)
__global__ __launch_bounds__(kThreads) void k_knn_scan_a(const SasKnn q)
{
    __shared__ unsigned s_wave[kWaves];
    const int tid = threadIdx.x;
    unsigned v[8];
    load8(q.table + (long long)blockIdx.x * kBlock + 8 * tid, v);
    unsigned total;
    (void)wg_exclusive_sum(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])), s_wave, tid, total);
    if (tid == 0 && SAS_IN(blockIdx.x, q.table_len / kBlock, 1403)) q.blk[blockIdx.x] = total;
}

// ONE workgroup: blk <- its exclusive prefix sums.  Lane t takes `per` consecutive entries.
__global__ __launch_bounds__(kThreads) void k_knn_scan_b(const SasKnn q)
{
    __shared__ unsigned s_wave[kWaves];
    const int tid = threadIdx.x;
    const long long nb = q.table_len / kBlock, per = (nb + kThreads - 1) / kThreads;
    const long long first = min((long long)tid * per, nb), last = min(first + per, nb);
    unsigned sum = 0u;
    for (long long b = first; b < last; ++b) sum += q.blk[b];
    unsigned total;
    unsigned run = wg_exclusive_sum(sum, s_wave, tid, total);
    for (long long b = first; b < last; ++b)
        if (SAS_IN(b, nb, 1404)) { const unsigned c = q.blk[b]; q.blk[b] = run; run += c; }
}

// table <- the start of every cell: the exclusive prefix inside the block plus the block's offset
__global__ __launch_bounds__(kThreads) void k_knn_scan_c(const SasKnn q)
{
    __shared__ unsigned s_wave[kWaves];
    const int tid = threadIdx.x;
    unsigned *p = q.table + (long long)blockIdx.x * kBlock + 8 * tid;
    unsigned v[8];
    load8(p, v);
    unsigned total;
    unsigned x = q.blk[blockIdx.x] + wg_exclusive_sum(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])), s_wave, tid, total);
    if (!SAS_IN((long long)blockIdx.x * kBlock + 8 * tid + 7, q.table_len, 1405)) return;
    unsigned o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { o[k] = x; x += v[k]; }
    *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4 *>(p + 4) = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ __launch_bounds__(kThreads) void k_knn_scatter(const SasKnn q)
{
    const SasKnnGrid &G = *q.grid;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.n) return;
    const float x = q.points[3 * i], y = q.points[3 * i + 1], z = q.points[3 * i + 2];
    long long pos = i;   // no grid: the caller's order
    if (!G.brute) {
        const long long c = finite3(x, y, z) ? cell_of(G, x, y, z) : (long long)G.n_cells;
        if (!SAS_IN(c, q.cells_cap + 1, 1406) || c > q.cells_cap) return;
        pos = (long long)atomicAdd(&q.table[c], 1u);   // (which of the cell's places: the order of arrival, which reaches no result)
    }
    if (SAS_IN(pos, q.n, 1407) && pos < q.n) q.pts[pos] = make_float4(x, y, z, __uint_as_float((unsigned)i));
}

// candidate c against the point (px, py, pz) of index i: the contract's d2 and key
template <int K>
DEV void meet(unsigned long long (&best)[K], const float4 c, float px, float py, float pz, unsigned i)
{
    const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const unsigned j = __float_as_uint(c.w);
    if (j != i && d2 < INFINITY) {   // (false for a NaN and for +inf)
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | j;
        if (key < best[K - 1]) keep_key<K>(best, key);
    }
}

template <int K>
DEV void write_rows(const SasKnn &q, unsigned i, const unsigned long long (&best)[K])
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j >= q.k) break;
        const long long o = (long long)i * q.k + j;
        if (!SAS_IN(o, q.n * q.k, 1408) || i >= (unsigned long long)q.n) continue;
        const bool none = (unsigned)(best[j] >> 32) == 0x7f800000u;
        q.dist2[o] = none ? INFINITY : __uint_as_float((unsigned)(best[j] >> 32));
        if (q.index) q.index[o] = none ? -1 : (int)(unsigned)(best[j] & 0xffffffffull);
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void k_knn_search(const SasKnn q)
{
    const SasKnnGrid &G = *q.grid;
    if (G.brute) return;   // (uniform)
    const long long s = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long n_finite = min((long long)q.table[G.n_cells - 1], q.n);   // the end of the last cell
    unsigned long long best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = kKnnNone;
    bool left = false;
    if (s < q.n) {
        const float4 p = q.pts[s];
        const unsigned i = __float_as_uint(p.w);
        if (s < n_finite) {
            const int n0 = G.n[0], n1 = G.n[1], n2 = G.n[2];
            const int c0 = cell_axis(p.x, G.lo[0], G.inv, n0), c1 = cell_axis(p.y, G.lo[1], G.inv, n1), c2 = cell_axis(p.z, G.lo[2], G.inv, n2);
            // the points of the cells [a, b] of one row (x fastest): table[c - 1] is where cell c starts, table[c] where it ends
            auto row = [&](long long a, long long b) {
                const long long e = min((long long)q.table[b], n_finite);
                for (long long t = q.table[a - 1]; t < e; ++t) meet<K>(best, q.pts[t], p.x, p.y, p.z, i);
            };
            for (int r = 0;; ++r) {
                for (int z = max(c2 - r, 0); z <= min(c2 + r, n2 - 1); ++z)
                    for (int y = max(c1 - r, 0); y <= min(c1 + r, n1 - 1); ++y) {
                        const long long base = ((long long)z * n1 + y) * n0;
                        if (abs(z - c2) == r || abs(y - c1) == r) row(base + max(c0 - r, 0), base + min(c0 + r, n0 - 1));
                        else {   // (r > 0 here) the ring's two cells of an inner row
                            if (c0 - r >= 0) row(base + c0 - r, base + c0 - r);
                            if (c0 + r < n0) row(base + c0 + r, base + c0 + r);
                        }
                    }
                const bool whole = c0 - r <= 0 && c0 + r >= n0 - 1 && c1 - r <= 0 && c1 + r >= n1 - 1 && c2 - r <= 0 && c2 + r >= n2 - 1;
                const float b = ((float)r - 9.765625e-4f) * G.h_lo;   // (r - 2^-10) h_lo: the stop rule at the head of the file
                const float bound2 = r > 0 ? b * b : 0.0f;
                if (whole || __uint_as_float((unsigned)(best[K - 1] >> 32)) < bound2) break;
                if (r == SAS_KNN_RING_LIMIT) { left = true; break; }
            }
        }
        if (!left) write_rows<K>(q, i, best);   // (a point with a non-finite coordinate: no neighbours)
    }
    // the leftover list: one atomic per wave, the lanes' places by their rank among the wave's leftover lanes
    const unsigned long long m = __ballot(left);
    if (left) {
        unsigned base = 0u;
        if (mbcnt64(m) == 0u) base = atomicAdd(&q.grid->left_count, (unsigned)__popcll(m));
        base = (unsigned)__shfl((int)base, __ffsll((long long)m) - 1, 64);
        const long long pos = (long long)base + mbcnt64(m);
        if (SAS_IN(pos, q.n, 1409) && pos < q.n) q.left[pos] = (int)s;
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void k_knn_brute(const SasKnn q)
{
    __shared__ float4 s_c[SAS_KNN_CHUNK];
    const SasKnnGrid &G = *q.grid;
    const long long count = G.brute ? q.n : min((long long)G.left_count, q.n);
    if ((long long)blockIdx.x * kThreads >= count) return;   // (uniform)
    const int tid = threadIdx.x, slice = blockIdx.y;
    const long long pos = (long long)blockIdx.x * kThreads + tid;
    const bool active = pos < count;
    long long s = 0;
    if (active) s = G.brute ? pos : (long long)q.left[pos];
    s = s < 0 ? 0 : (s < q.n ? s : q.n - 1);
    const float4 p = q.pts[s];
    const unsigned i = __float_as_uint(p.w);
    unsigned long long best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = kKnnNone;
    const long long first = (long long)slice * q.slice_points, last = min(first + q.slice_points, q.n);
    for (long long base = first; base < last; base += SAS_KNN_CHUNK) {
        const int nload = (int)min((long long)SAS_KNN_CHUNK, last - base);
        __syncthreads();   // the chunk before has been read
        if (tid < nload && SAS_IN(base + tid, q.n, 1410) && SAS_IN(tid, SAS_KNN_CHUNK, 1411)) s_c[tid] = q.pts[base + tid];
        __syncthreads();
        for (int t = 0; t < nload; ++t) meet<K>(best, s_c[t], p.x, p.y, p.z, i);
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const long long o = ((long long)slice * q.n + pos) * K + j;
        if (SAS_IN(o, (long long)q.slices * q.n * K, 1412)) q.keys[o] = best[j];
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void k_knn_merge(const SasKnn q)
{
    const SasKnnGrid &G = *q.grid;
    const long long count = G.brute ? q.n : min((long long)G.left_count, q.n);
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pos >= count) return;
    long long s = G.brute ? pos : (long long)q.left[pos];
    s = s < 0 ? 0 : (s < q.n ? s : q.n - 1);
    const unsigned i = __float_as_uint(q.pts[s].w);
    unsigned long long best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = kKnnNone;
    for (int sl = 0; sl < q.slices; ++sl)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const unsigned long long key = q.keys[((long long)sl * q.n + pos) * K + j];   // (a slice's keys are distinct from every other slice's)
            if (key < best[K - 1]) keep_key<K>(best, key);
        }
    write_rows<K>(q, i, best);
}

template <int K>
void launch_search(hipStream_t st, const SasKnn &q, unsigned blocks)
{
    const dim3 wg(kThreads);
    hipLaunchKernelGGL(k_knn_search<K>, dim3(blocks), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_brute<K>, dim3(blocks, (unsigned)q.slices), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_merge<K>, dim3(blocks), wg, 0, st, q);
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_knn)

// behind sas_launch_order_bounds into q.bounds, and with occ and table zeroed, on the same stream
void sas_launch_knn(hipStream_t st, const SasKnn &q)
{
    if (q.n <= 0) return;
    const dim3 wg(kThreads);
    const unsigned blocks = (unsigned)((q.n + kThreads - 1) / kThreads), scan_blocks = (unsigned)(q.table_len / kBlock);
    hipLaunchKernelGGL(k_knn_occupancy, dim3(blocks), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_grid, dim3(1), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_count, dim3(blocks), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_scan_a, dim3(scan_blocks), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_scan_b, dim3(1), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_scan_c, dim3(scan_blocks), wg, 0, st, q);
    hipLaunchKernelGGL(k_knn_scatter, dim3(blocks), wg, 0, st, q);
    if (q.k <= 3) launch_search<3>(st, q, blocks);
    else launch_search<8>(st, q, blocks);
}
