// sas_match.hip -- nearest-neighbour matching of two point clouds (sas_match_points; DESIGN.md 3, "Point matching"): for every source
// point, moved by a 3x4 affine map, the nearest target point within max_distance, and the moments of the held matches a closed-form
// similarity fit needs.  It is the hot path of the ICP registration (register.py; the reference's match_splat.py:208-223 through
// open3d's registration_icp): 20 000 sampled robot points against the cropped centres of a splat, up to 30 times.
//
//   k_match_slice  grid (source blocks of 256, target slices), one source point per lane.  The slice's targets pass through LDS as
//                  float4 in chunks of SAS_MATCH_CHUNK and every lane reads the same address (the broadcast ds_read_b128 of
//                  k_query_eval): per target three subtractions, three products, two sums and a strict `<` against the running
//                  minimum, in target order -- the lowest index wins among equal d2.  Each lane writes its slice minimum as the key
//                  (bits(d2) << 32 | j) to keys[slice][i].  Slices exist because 20 000 source points are 79 workgroups on 256 CUs.
//   k_match_merge  one thread per source point: the minimum key over the slices (the bits of a non-negative float order as the float
//                  does, so the minimum key is the minimum d2 and, among equals, the lowest j), the max_distance rule, index / dist2,
//                  and the 18 float64 moments of the workgroup in a fixed tree (wave shuffles, then LDS across the four waves): one
//                  partial row per workgroup.
//   k_match_sum    one wave: lane l adds the partial rows l, l + 64, ... in order, then the same wave tree.
// No float atomics; no result depends on the slice count or on the other points of the call.
// Arithmetic: IEEE binary32 (moments: binary64 of the widened binary32 values), nothing fused (-ffp-contract=off, no fma_).
#include "sas_device.h"

namespace {

constexpr int kMatchThreads = 256;
static_assert(SAS_MATCH_CHUNK == kMatchThreads, "every thread of k_match_slice stages one target of a chunk");
constexpr unsigned long long kNoMatch = (0x7f800000ull << 32) | 0xffffffffull;   // d2 = +inf: above the key of every match

// p' = A p + t (sas_affine_row)
DEV void move_source(const SasMatch &m, long long i, float &px, float &py, float &pz)
{
    const float x = m.source[3 * i], y = m.source[3 * i + 1], z = m.source[3 * i + 2];
    px = sas_affine_row<0>(m, x, y, z);
    py = sas_affine_row<1>(m, x, y, z);
    pz = sas_affine_row<2>(m, x, y, z);
}

__global__ __launch_bounds__(kMatchThreads) void k_match_slice(SasMatch m)
{
    __shared__ float4 s_q[SAS_MATCH_CHUNK];
    const int tid = threadIdx.x, slice = blockIdx.y;
    const long long i = (long long)blockIdx.x * kMatchThreads + tid;
    const bool active = i < m.n_source && SAS_IN(i, m.n_source, 501);
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (active) move_source(m, i, px, py, pz);
    float best = INFINITY;
    unsigned best_j = 0xffffffffu;
    const long long first = (long long)slice * m.slice_targets;
    const long long last = min(first + m.slice_targets, m.n_target);
    for (long long base = first; base < last; base += SAS_MATCH_CHUNK) {
        const int nload = (int)min((long long)SAS_MATCH_CHUNK, last - base);
        __syncthreads();   // the chunk before has been read
        if (tid < nload && SAS_IN(base + tid, m.n_target, 502) && SAS_IN(tid, SAS_MATCH_CHUNK, 503)) {
            const float *src = m.target + 3 * (base + tid);
            s_q[tid] = make_float4(src[0], src[1], src[2], 0.0f);
        }
        __syncthreads();
        for (int k = 0; k < nload; ++k) {
            const float4 q = s_q[k];
            const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) {   // (false for a NaN and for +inf: such a target never matches; strict: the lowest index keeps a tie)
                best = d2;
                best_j = (unsigned)(base + k);
            }
        }
    }
    if (active && SAS_IN((long long)slice * m.n_source + i, (long long)m.slices * m.n_source, 504))
        m.keys[(long long)slice * m.n_source + i] = ((unsigned long long)__float_as_uint(best) << 32) | best_j;
}

// the sum over the wave's lanes in a fixed tree, in lane 0
DEV double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kMatchThreads) void k_match_merge(SasMatch m)
{
    __shared__ double s_part[kMatchThreads / 64][SAS_MATCH_MOMENTS];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMatchThreads + tid;
    const bool active = i < m.n_source && SAS_IN(i, m.n_source, 505);
    unsigned long long key = kNoMatch;
    if (active)
        for (int s = 0; s < m.slices; ++s)
            if (SAS_IN((long long)s * m.n_source + i, (long long)m.slices * m.n_source, 506)) {
                const unsigned long long k = m.keys[(long long)s * m.n_source + i];
                key = k < key ? k : key;
            }
    const float d2 = __uint_as_float((unsigned)(key >> 32));
    long long j = (long long)(key & 0xffffffffull);
    const bool held = active && d2 < INFINITY && d2 <= m.md2 && SAS_IN(j, m.n_target, 507);
    if (active) {
        if (m.index) m.index[i] = held ? (int)j : -1;
        if (m.dist2) m.dist2[i] = held ? d2 : INFINITY;
    }
    if (!m.partial) return;   // (uniform)
    double v[SAS_MATCH_MOMENTS];
#pragma unroll
    for (int k = 0; k < SAS_MATCH_MOMENTS; ++k) v[k] = 0.0;
    if (held) {
        float fx, fy, fz;
        move_source(m, i, fx, fy, fz);   // (the same operations as in k_match_slice: the same bits)
        const double p[3] = {(double)fx, (double)fy, (double)fz};
        const double q[3] = {(double)m.target[3 * j], (double)m.target[3 * j + 1], (double)m.target[3 * j + 2]};
        v[0] = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[1 + a] = p[a];
            v[4 + a] = q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] = q[a] * p[b];
        }
        v[16] = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        v[17] = (double)d2;
    }
#pragma unroll
    for (int k = 0; k < SAS_MATCH_MOMENTS; ++k) {
        const double w = wave_sum_f64(v[k]);
        if ((tid & 63) == 0) s_part[tid >> 6][k] = w;
    }
    __syncthreads();
    if (tid < SAS_MATCH_MOMENTS && SAS_IN((long long)blockIdx.x * SAS_MATCH_MOMENTS + tid, m.n_blocks * SAS_MATCH_MOMENTS, 508))
        m.partial[(long long)blockIdx.x * SAS_MATCH_MOMENTS + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
}

__global__ __launch_bounds__(64) void k_match_sum(SasMatch m)
{
    const int lane = threadIdx.x;
    for (int k = 0; k < SAS_MATCH_MOMENTS; ++k) {
        double v = 0.0;
        for (long long b = lane; b < m.n_blocks; b += 64)
            if (SAS_IN(b * SAS_MATCH_MOMENTS + k, m.n_blocks * SAS_MATCH_MOMENTS, 509)) v = v + m.partial[b * SAS_MATCH_MOMENTS + k];
        v = wave_sum_f64(v);
        if (lane == 0) m.moments[k] = v;
    }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_match)

void sas_launch_match(hipStream_t st, const SasMatch &m)
{
    if (m.n_source <= 0) return;
    hipLaunchKernelGGL(k_match_slice, dim3((unsigned)m.n_blocks, (unsigned)m.slices), dim3(kMatchThreads), 0, st, m);
    hipLaunchKernelGGL(k_match_merge, dim3((unsigned)m.n_blocks), dim3(kMatchThreads), 0, st, m);
    if (m.partial) hipLaunchKernelGGL(k_match_sum, dim3(1), dim3(64), 0, st, m);
}
