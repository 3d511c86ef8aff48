// sas_cloud.hip -- fixed-size point clouds from depth frames (sas_sample_points; DESIGN.md 3, "Point clouds"): the pixels of C same-sized
// views are unprojected, moved into the output frame, cropped, thinned on a voxel grid and cut to K points per cloud by farthest-point
// sampling, with colour and label.  It is the consumer behind a label frame (sas_render_batch_labels): depth, rgb8 and labels stay on
// the device.
//
//   k_cloud_mark     grid (blocks of 256 strided pixels, views), one strided pixel per lane: candidate test, camera point (the expression
//                    of k_depth_tail), output-frame point, crop, and atomicMin(p) into the cloud's voxel cell.  Every lane leaves a
//                    float4 (w, cell bits | none) behind: the later passes read the point, they do not compute it again.
//   k_cloud_compact  the same grid, twice: <0> counts each block's survivors (a candidate whose cell holds its own p; every candidate
//                    without a grid), k_cloud_scan (one workgroup per cloud) turns the counts of the cloud's blocks, in view and pixel
//                    order, into offsets, <1> writes the survivors' rows (w, bits(p)) at offset + rank in block: ordered by p.
//   k_cloud_fps      one workgroup of 1024 lanes per cloud.  <true>: up to SAS_CLOUD_RESIDENT survivors, lane l keeps ranks l, l + 1024,
//                    ... and their running distances in registers; <false>: more, rows and distances stream from global memory (L2), eight ranks
//                    of a lane in flight at a time.
//                    Per pick every lane updates its distances against the last pick and takes its best key, the wave reduces
//                    (distance bits, then ~rank) on the DPP network, the 16 waves meet through one of two LDS slots with ONE barrier, and
//                    every lane reads the winner's coordinates from the winning wave's LDS entry.  The picks' ranks go to `index`; when
//                    the picks are done the workgroup's lanes turn them into the output rows (and the padding rows) side by side.
// No float atomics, no spin waits, no cooperative launch: a cloud's result depends on its own views' pixels only.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_).
#include "sas_device.h"

namespace {

constexpr int kCloudThreads = 256;
constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsSlots = SAS_CLOUD_RESIDENT / kFpsThreads;   // ranks a lane keeps in registers
static_assert(SAS_CLOUD_RESIDENT % kFpsThreads == 0, "every lane of k_cloud_fps<true> keeps the same number of ranks");
constexpr int kFpsBatch = 8;   // ranks per lane k_cloud_fps<false> loads at a time
constexpr unsigned kNoCell = 0xffffffffu;

DEV bool finite_f(float v) { return fabsf(v) < INFINITY; }   // (false for a NaN)

// the strided pixel of this lane: false beyond the view
DEV bool cloud_pixel(const SasCloud &q, int &c, long long &ci, long long &p, int &u, int &v)
{
    c = blockIdx.y;
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    if (i >= q.S) return false;
    const int vs = (int)(i / q.Ws), us = (int)(i - (long long)vs * q.Ws);
    u = us * q.stride;
    v = vs * q.stride;
    ci = (long long)c * q.S + i;
    p = ((long long)c * q.H + v) * q.W + u;
    return SAS_IN(c, q.C, 601) && SAS_IN(ci, q.n_rows, 602) && SAS_IN(p, q.n_pix, 603);
}

__global__ __launch_bounds__(kCloudThreads) void k_cloud_mark(SasCloud q)
{
    int c, u, v;
    long long ci, p;
    if (!cloud_pixel(q, c, ci, p, u, v)) return;
    const SasCloudView V = q.view[c];
    const float d = q.depth[p];
    bool ok = d > 0.0f && d < INFINITY;
    if (ok && q.labels && q.keep) ok = q.keep[q.labels[p]] != 0;
    const float x = ((float)u - V.cam.cx) * d / V.cam.fx, y = ((float)v - V.cam.cy) * d / V.cam.fy, z = d;
    const float w0 = sas_affine_row<0>(V.cam, x, y, z);
    const float w1 = sas_affine_row<1>(V.cam, x, y, z);
    const float w2 = sas_affine_row<2>(V.cam, x, y, z);
    ok = ok && finite_f(w0) && finite_f(w1) && finite_f(w2);
    if (q.has_bounds)
        ok = ok && q.lo[0] <= w0 && w0 <= q.hi[0] && q.lo[1] <= w1 && w1 <= q.hi[1] && q.lo[2] <= w2 && w2 <= q.hi[2];
    unsigned cell = ok ? 0u : kNoCell;
    if (ok && q.voxel > 0.0f) {
        const float w[3] = {w0, w1, w2};
        int ik[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // min((int)floorf(...), n_k - 1), the minimum taken before the conversion: no float beyond int's range is converted
            const float f = floorf((w[k] - q.lo[k]) / q.voxel);
            ik[k] = f >= (float)(q.n[k] - 1) ? q.n[k] - 1 : (int)f;
        }
        cell = (unsigned)(((long long)ik[0] * q.n[1] + ik[1]) * q.n[2] + ik[2]);
        const long long g = (long long)V.cloud * q.cells + cell;
        if (SAS_IN(cell, q.cells, 604) && SAS_IN(g, q.n_grid, 605)) atomicMin(&q.grid[g], (unsigned)p);
    }
    q.cand[ci] = make_float4(w0, w1, w2, __uint_as_float(cell));
}

// does this lane's strided pixel survive?  (after k_cloud_mark)
DEV bool cloud_survives(const SasCloud &q, bool in_view, int c, long long ci, long long p, float4 &row)
{
    if (!in_view) return false;
    row = q.cand[ci];
    const unsigned cell = __float_as_uint(row.w);
    if (cell == kNoCell) return false;
    row.w = __uint_as_float((unsigned)p);
    if (!(q.voxel > 0.0f)) return true;
    const long long g = (long long)q.view[c].cloud * q.cells + cell;
    return SAS_IN(g, q.n_grid, 606) && q.grid[g] == (unsigned)p;
}

// PHASE 0: blk_count <- survivors of the block; PHASE 1: the survivors' rows to blk_off + rank in block
template <int PHASE>
__global__ __launch_bounds__(kCloudThreads) void k_cloud_compact(SasCloud q)
{
    __shared__ unsigned s_wave[kCloudThreads / 64];
    const int tid = threadIdx.x, wv = tid >> 6;
    int c, u, v;
    long long ci = 0, p = 0;
    const bool in_view = cloud_pixel(q, c, ci, p, u, v);
    float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool s = cloud_survives(q, in_view, c, ci, p, row);
    const unsigned long long mask = __ballot(s);
    if ((tid & 63) == 0) s_wave[wv] = (unsigned)__popcll(mask);
    __syncthreads();
    const long long b = (long long)blockIdx.y * q.bpv + blockIdx.x;
    if (!SAS_IN(b, q.n_blocks, 607)) return;   // (uniform)
    if (PHASE == 0) {
        if (tid == 0) q.blk_count[b] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        return;
    }
    unsigned before = 0;
    for (int k = 0; k < wv; ++k) before += s_wave[k];
    if (s) {
        const long long r = q.view[blockIdx.y].base + q.blk_off[b] + before + mbcnt64(mask);
        if (SAS_IN(r, q.n_rows, 608)) q.rows[r] = row;
    }
}

// one workgroup per cloud: offsets of the cloud's blocks in view and pixel order, and M
__global__ __launch_bounds__(kCloudThreads) void k_cloud_scan(SasCloud q)
{
    __shared__ unsigned s_wave[2][kCloudThreads / 64];
    const int tid = threadIdx.x, wv = tid >> 6, e = blockIdx.x;
    unsigned running = 0;
    int slot = 0;
    for (long long b0 = 0; b0 < q.n_blocks; b0 += kCloudThreads, slot ^= 1) {
        const long long b = b0 + tid;
        const bool mine = b < q.n_blocks && SAS_IN(b / q.bpv, q.C, 609) && q.view[b / q.bpv].cloud == e;
        const unsigned n = mine ? q.blk_count[b] : 0u;
        const unsigned incl = wave_inclusive_sum_u32(n);
        if ((tid & 63) == 63) s_wave[slot][wv] = incl;
        __syncthreads();   // (the slots alternate: one barrier per round)
        unsigned before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kCloudThreads / 64; ++k) {
            before += k < wv ? s_wave[slot][k] : 0u;
            total += s_wave[slot][k];
        }
        if (mine) q.blk_off[b] = running + before + (incl - n);
        running += total;
    }
    if (tid == 0 && SAS_IN(e, q.E, 610)) {
        q.m_count[e] = (int)running;
        if (q.count) q.count[e] = (int)running;
    }
}

// key order: the larger distance bits, then the larger ~rank (the lower rank); lo == 0: no key
DEV bool key_above(unsigned h, unsigned l, unsigned bh, unsigned bl) { return h > bh || (h == bh && l > bl); }

template <bool RES>
__global__ __launch_bounds__(kFpsThreads) void k_cloud_fps(SasCloud q)
{
    __shared__ uint2 s_key[2][kFpsWaves];
    __shared__ float4 s_xyz[2][kFpsWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, e = blockIdx.x;
    if (!SAS_IN(e, q.E, 611)) return;
    const int M = q.m_count[e];
    if (RES != (M <= SAS_CLOUD_RESIDENT)) return;   // (uniform) the other instantiation samples this cloud
    const long long base = q.cloud_base[e];
    if (M > 0 && !(SAS_IN(base, q.n_rows, 612) && SAS_IN(base + M - 1, q.n_rows, 613))) return;   // (uniform)
    const float4 *rows = q.rows + base;
    float *dist = q.dist + base;
    const int K = q.K, npick = min(K, M);
    int32_t *index = q.index + (long long)e * K;

    float px[kFpsSlots], py[kFpsSlots], pz[kFpsSlots], pd[kFpsSlots];
    if (RES) {
#pragma unroll
        for (int j = 0; j < kFpsSlots; ++j) {
            const int i = tid + kFpsThreads * j;
            px[j] = py[j] = pz[j] = 0.0f;
            pd[j] = INFINITY;
            if (i < M) {
                const float4 r = rows[i];
                px[j] = r.x; py[j] = r.y; pz[j] = r.z;
            }
        }
    } else {
        for (int i = tid; i < M; i += kFpsThreads) dist[i] = INFINITY;
    }
    unsigned win = 0;   // pick 0 is rank 0
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (npick > 0) {
        const float4 r = rows[0];
        sx = r.x; sy = r.y; sz = r.z;
    }
    for (int k = 0; k < npick; ++k) {
        if (tid == 0) index[k] = (int)win;   // the rank for now: the epilogue turns it into the row
        if (k + 1 == npick) break;
        // this lane's distances against the last pick, and its best key: a picked point keeps -1 and has no key
        unsigned bh = 0, bl = 0;
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        auto visit = [&](unsigned i, float x, float y, float z, float d) {
            const float dx = x - sx, dy = y - sy, dz = z - sz;
            d = i == win ? -1.0f : fminf(d, (dx * dx + dy * dy) + dz * dz);
            const unsigned h = __float_as_uint(d);
            if (d >= 0.0f && (bl == 0u || h > bh)) {   // (ranks ascend within a lane: an equal distance keeps the earlier one)
                bh = h; bl = ~i;
                bx = x; by = y; bz = z;
            }
            return d;
        };
        if (RES) {
#pragma unroll
            for (int j = 0; j < kFpsSlots; ++j) {
                if (kFpsThreads * j >= M) break;   // (uniform)
                const int i = tid + kFpsThreads * j;
                if (i < M) pd[j] = visit((unsigned)i, px[j], py[j], pz[j], pd[j]);
            }
        } else {
            // kFpsBatch ranks of the lane at a time: their loads are in flight together, then they are visited in rank order
            for (int i0 = tid; i0 < M; i0 += kFpsThreads * kFpsBatch) {
                float4 r[kFpsBatch];
                float d[kFpsBatch];
#pragma unroll
                for (int u = 0; u < kFpsBatch; ++u) {
                    const int i = i0 + kFpsThreads * u;
                    r[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    d[u] = -1.0f;
                    if (i < M) { r[u] = rows[i]; d[u] = dist[i]; }
                }
#pragma unroll
                for (int u = 0; u < kFpsBatch; ++u) {
                    const int i = i0 + kFpsThreads * u;
                    if (i < M) dist[i] = visit((unsigned)i, r[u].x, r[u].y, r[u].z, d[u]);
                }
            }
        }
        // the wave's best: the distance bits, then ~rank among the lanes that hold them
        const unsigned mh = wave_max_u32(bh);
        const unsigned ml = wave_max_u32(bh == mh ? bl : 0u);
        const int src = (int)(~ml & 63u);   // the lane that owns rank ~ml (ranks are lane + 1024 j)
        const float wx = lane_get(bx, src), wy = lane_get(by, src), wz = lane_get(bz, src);
        const int slot = k & 1;   // (two slots: pick k + 1 writes the other one while a slow wave still reads this one)
        if (lane == 0) {
            s_key[slot][wv] = make_uint2(mh, ml);
            s_xyz[slot][wv] = make_float4(wx, wy, wz, 0.0f);
        }
        __syncthreads();
        unsigned gh = 0, gl = 0;
        int gw = 0;
#pragma unroll
        for (int w = 0; w < kFpsWaves; ++w) {
            const uint2 kk = s_key[slot][w];
            if (key_above(kk.x, kk.y, gh, gl)) { gh = kk.x; gl = kk.y; gw = w; }
        }
        const float4 g = s_xyz[slot][gw];
        win = ~gl;   // (npick <= M: an unpicked survivor exists, gl != 0)
        sx = g.x; sy = g.y; sz = g.z;
    }
    __syncthreads();   // index[0 .. npick) is visible to the workgroup
    // the output rows in pick order, then the padding
    for (int k = tid; k < K; k += kFpsThreads) {
        const long long o = (long long)e * K + k;
        if (!SAS_IN(o, (long long)q.E * K, 614)) continue;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        long long p = -1;
        if (k < npick) {
            const int rank = index[k];
            if (!SAS_IN(rank, M, 615)) continue;
            r = rows[rank];
            p = (long long)__float_as_uint(r.w);
            if (!SAS_IN(p, q.n_pix, 616)) continue;
        }
        index[k] = (int)p;
        if (q.points) { q.points[3 * o] = r.x; q.points[3 * o + 1] = r.y; q.points[3 * o + 2] = r.z; }
        if (q.colors)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) q.colors[3 * o + ch] = p >= 0 ? q.rgb8[3 * p + ch] : (uint8_t)0;
        if (q.labels_out) q.labels_out[o] = p >= 0 ? q.labels[p] : (uint8_t)255;
    }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_cloud)

void sas_launch_cloud(hipStream_t st, const SasCloud &q, hipEvent_t *ev)
{
    if (ev) (void)hipEventRecord(ev[0], st);
    if (q.n_blocks > 0) hipLaunchKernelGGL(k_cloud_mark, dim3((unsigned)q.bpv, (unsigned)q.C), dim3(kCloudThreads), 0, st, q);
    if (ev) (void)hipEventRecord(ev[1], st);
    if (q.n_blocks > 0) hipLaunchKernelGGL(k_cloud_compact<0>, dim3((unsigned)q.bpv, (unsigned)q.C), dim3(kCloudThreads), 0, st, q);
    hipLaunchKernelGGL(k_cloud_scan, dim3((unsigned)q.E), dim3(kCloudThreads), 0, st, q);
    if (q.n_blocks > 0) hipLaunchKernelGGL(k_cloud_compact<1>, dim3((unsigned)q.bpv, (unsigned)q.C), dim3(kCloudThreads), 0, st, q);
    if (ev) (void)hipEventRecord(ev[2], st);
    hipLaunchKernelGGL(k_cloud_fps<true>, dim3((unsigned)q.E), dim3(kFpsThreads), 0, st, q);
    hipLaunchKernelGGL(k_cloud_fps<false>, dim3((unsigned)q.E), dim3(kFpsThreads), 0, st, q);
    if (ev) (void)hipEventRecord(ev[3], st);
}
