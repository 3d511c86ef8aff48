// sas_skin.hip -- deformable splats (sas_knn_cross, sas_scene_skin, sas_scene_deform; DESIGN.md 3, "Deformation"), hand-written for gfx950
// (CDNA4, wave64): an embedded deformation graph.  Every Gaussian of the resident scene is bound to up to 8 of M control nodes with weights;
// the nodes move rigidly, the means follow by linear blend skinning and the orientations by a blended quaternion.
//
//   k_knn_cross<K>  one lane per query point: its k nearest NODES of a second cloud.  sas_knn.hip's contract bit for bit (the keys and the
//                   insert are its helpers, sas_device.h) with two differences: nothing is left out by index, and a candidate beyond md2 never
//                   counts.  Brute force -- M is small, a grid would cost more than it saves: the nodes pass through LDS in chunks of
//                   SAS_KNN_CHUNK and every lane of the workgroup reads the same address (k_knn_brute's form); the K best keys sit in registers.
//   k_skin_bind     one lane per slot: the caller's [N,k] indices and weights through perm into planes of int4 / float4 per slot, stride
//                   n_pad, padded to 4 or 8 entries with (-1, 0).
//   k_skin_read     the inverse: the planes back in the caller's order.
//   k_skin_nodes    one lane per node: R -> the unit quaternion wxyz, by the branch of the largest of (trace, R00, R11, R22); the node's
//                   64-byte record (SasSkinNode).
//   k_deform<LDS,KP> one lane per slot: the rest planes and the slot's skin planes -> g0, g1, g2.  The LIVE entries are those with
//                   0 <= index < m and weight > 0; every other entry is ignored, so no index reaches memory unchecked.
//                     no live entry: the three planes are the rest planes' bits
//                     mean:     m' = m + (sum_j w_j ((R_j m + t_j) - m)) / W,  W = sum_j w_j, in entry order; R m + t = ((r0 x + r1 y) + r2 z) + t
//                     rotation: q_b = normalize(sum_j s_j w_j q_j), s_j = -1 where dot(q_j, q_first) < 0 (q_first: the first live entry's); a sum
//                               of norm zero or not finite gives q_first
//                     quaternion scenes: g1 = q_b (x) q_rest (Hamilton, not renormalised: the projection normalises), scales untouched
//                     covariance scenes: Sigma' = R_b Sigma_rest R_b^T, R_b the matrix of q_b
//                   Opacity, the group-id bits and g2.z of a covariance scene are the rest planes' bits.  LDS: the node records are staged
//                   in LDS by every workgroup (m * 64 B within SAS_SKIN_LDS_BYTES); else each lane reads its records from global memory.  The
//                   arithmetic is the same text on the same values: both paths give the same bits.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_); tests/tools/skin_ref.py restates it.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
static_assert(SAS_KNN_CHUNK == kThreads, "one node per thread of a chunk");
static_assert(SAS_SKIN_LDS_BYTES % sizeof(SasSkinNode) == 0, "whole records");

// node c against the point (px, py, pz): the contract's d2 and key, and the cut at md2
template <int K>
DEV void meet_node(unsigned long long (&best)[K], const float4 c, float px, float py, float pz, float md2)
{
    const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < INFINITY && d2 <= md2) {   // (false for a NaN and for +inf)
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(c.w);
        if (key < best[K - 1]) keep_key<K>(best, key);
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void k_knn_cross(const SasKnnCross q)
{
    __shared__ float4 s_c[SAS_KNN_CHUNK];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    const bool active = i < q.n;
    const long long ic = active ? i : q.n - 1;   // (q.n > 0: the launcher)
    const float px = q.points[3 * ic], py = q.points[3 * ic + 1], pz = q.points[3 * ic + 2];
    unsigned long long best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = kKnnNone;
    for (int base = 0; base < q.m; base += SAS_KNN_CHUNK) {
        const int nload = min(SAS_KNN_CHUNK, q.m - base);
        __syncthreads();   // the chunk before has been read
        if (tid < nload && SAS_IN(base + tid, q.m, 1501) && SAS_IN(tid, SAS_KNN_CHUNK, 1502)) {
            const float *c = q.nodes + 3 * (long long)(base + tid);
            s_c[tid] = make_float4(c[0], c[1], c[2], __uint_as_float((unsigned)(base + tid)));
        }
        __syncthreads();
        for (int t = 0; t < nload; ++t) meet_node<K>(best, s_c[t], px, py, pz, q.md2);
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j >= q.k) break;
        const long long o = i * q.k + j;
        if (!SAS_IN(o, q.n * q.k, 1503)) continue;
        const bool none = (unsigned)(best[j] >> 32) == 0x7f800000u;
        q.dist2[o] = none ? INFINITY : __uint_as_float((unsigned)(best[j] >> 32));
        if (q.index) q.index[o] = none ? -1 : (int)(unsigned)(best[j] & 0xffffffffull);
    }
}

__global__ __launch_bounds__(kThreads) void k_skin_bind(const SasSkinBind q)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // slot
    if (j >= q.n_pad) return;
    long long i = j < q.n ? (long long)q.perm[j] : -1;                    // caller's index; the padding slots hold no entry
    if (i >= 0 && !SAS_IN(i, q.n, 1504)) i = -1;
    for (int p = 0; p < q.kp / 4; ++p) {
        int v[4];
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = 4 * p + e;
            const bool given = i >= 0 && col < q.k;
            v[e] = given ? q.indices[i * q.k + col] : -1;
            u[e] = given ? q.weights[i * q.k + col] : 0.0f;
        }
        const long long o = (long long)p * q.n_pad + j;
        if (!SAS_IN(o, (long long)(q.kp / 4) * q.n_pad, 1505)) continue;
        q.idx[o] = make_int4(v[0], v[1], v[2], v[3]);
        q.w[o] = make_float4(u[0], u[1], u[2], u[3]);
    }
}

__global__ __launch_bounds__(kThreads) void k_skin_read(const SasSkinRead q)
{
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= q.n) return;
    const long long i = q.perm[j];
    if (!SAS_IN(i, q.n, 1506)) return;
    for (int p = 0; 4 * p < q.k; ++p) {
        const int4 v = q.idx[(long long)p * q.n_pad + j];
        const float4 u = q.w[(long long)p * q.n_pad + j];
        const int vv[4] = {v.x, v.y, v.z, v.w};
        const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = 4 * p + e;
            if (col >= q.k) break;
            q.indices[i * q.k + col] = vv[e];
            q.weights[i * q.k + col] = uu[e];
        }
    }
}

// R -> wxyz.  Each branch's four terms are 4 c times the quaternion, c its largest component: no cancellation in the term that is squared.
__global__ __launch_bounds__(kThreads) void k_skin_nodes(const SasDeform q)
{
    const int a = blockIdx.x * kThreads + threadIdx.x;
    if (a >= q.m) return;
    const float *G = q.node_Rt + 12 * (long long)a;
    const float r00 = G[0], r01 = G[1], r02 = G[2], r10 = G[4], r11 = G[5], r12 = G[6], r20 = G[8], r21 = G[9], r22 = G[10];
    const float tr = (r00 + r11) + r22;
    float w, x, y, z;
    if (tr >= r00 && tr >= r11 && tr >= r22) {
        w = 1.0f + tr; x = r21 - r12; y = r02 - r20; z = r10 - r01;
    } else if (r00 >= r11 && r00 >= r22) {
        w = r21 - r12; x = ((1.0f + r00) - r11) - r22; y = r01 + r10; z = r02 + r20;
    } else if (r11 >= r22) {
        w = r02 - r20; x = r01 + r10; y = ((1.0f + r11) - r00) - r22; z = r12 + r21;
    } else {
        w = r10 - r01; x = r02 + r20; y = r12 + r21; z = ((1.0f + r22) - r00) - r11;
    }
    const float inv = 1.0f / sqrtf(((w * w + x * x) + y * y) + z * z);
    if (!SAS_IN(a, q.m, 1507)) return;
    float4 *rec = reinterpret_cast<float4 *>(q.nodes + a);
    rec[0] = make_float4(G[0], G[1], G[2], G[3]);
    rec[1] = make_float4(G[4], G[5], G[6], G[7]);
    rec[2] = make_float4(G[8], G[9], G[10], G[11]);
    rec[3] = make_float4(w * inv, x * inv, y * inv, z * inv);
}

template <bool LDS, int KP>
__global__ __launch_bounds__(kThreads) void k_deform(const SasDeform q)
{
    __shared__ float4 s_nodes[LDS ? SAS_SKIN_LDS_BYTES / 16 : 1];
    const float4 *g_nodes = reinterpret_cast<const float4 *>(q.nodes);
    if constexpr (LDS) {
        for (int t = threadIdx.x; t < 4 * q.m; t += kThreads)
            if (SAS_IN(t, SAS_SKIN_LDS_BYTES / 16, 1508)) s_nodes[t] = g_nodes[t];
        __syncthreads();
    }
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // slot
    if (j >= q.n || !SAS_IN(j, q.n_pad, 1509)) return;
    auto rec = [&](int node, int part) -> float4 {
        if constexpr (LDS) return s_nodes[4 * node + part];
        else return g_nodes[4 * (long long)node + part];
    };
    const float4 r0 = q.r0[j], r1 = q.r1[j], r2 = q.r2[j];
    int id[KP];
    float wt[KP];
#pragma unroll
    for (int p = 0; p < KP / 4; ++p) {
        const int4 v = q.idx[(long long)p * q.n_pad + j];
        const float4 u = q.w[(long long)p * q.n_pad + j];
        id[4 * p] = v.x; id[4 * p + 1] = v.y; id[4 * p + 2] = v.z; id[4 * p + 3] = v.w;
        wt[4 * p] = u.x; wt[4 * p + 1] = u.y; wt[4 * p + 2] = u.z; wt[4 * p + 3] = u.w;
    }
    float ax = 0.0f, ay = 0.0f, az = 0.0f, W = 0.0f;
    float4 f = make_float4(1.0f, 0.0f, 0.0f, 0.0f), aq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool any = false;
#pragma unroll
    for (int e = 0; e < KP; ++e) {
        const float we = wt[e];
        if (!(id[e] >= 0 && id[e] < q.m && we > 0.0f)) continue;   // not live
        const float4 a = rec(id[e], 0), b = rec(id[e], 1), c = rec(id[e], 2), qn = rec(id[e], 3);
        const float y0 = ((a.x * r0.x + a.y * r0.y) + a.z * r0.z) + a.w;
        const float y1 = ((b.x * r0.x + b.y * r0.y) + b.z * r0.z) + b.w;
        const float y2 = ((c.x * r0.x + c.y * r0.y) + c.z * r0.z) + c.w;
        ax = ax + we * (y0 - r0.x);
        ay = ay + we * (y1 - r0.y);
        az = az + we * (y2 - r0.z);
        W = W + we;
        if (!any) f = qn;
        any = true;
        const float dot = ((qn.x * f.x + qn.y * f.y) + qn.z * f.z) + qn.w * f.w;
        const float sw = dot < 0.0f ? -we : we;
        aq.x = aq.x + sw * qn.x;
        aq.y = aq.y + sw * qn.y;
        aq.z = aq.z + sw * qn.z;
        aq.w = aq.w + sw * qn.w;
    }
    float4 o0 = r0, o1 = r1, o2 = r2;
    if (any) {
        o0.x = r0.x + ax / W;
        o0.y = r0.y + ay / W;
        o0.z = r0.z + az / W;
        const float n2 = ((aq.x * aq.x + aq.y * aq.y) + aq.z * aq.z) + aq.w * aq.w;
        float bw = f.x, bx = f.y, by = f.z, bz = f.w;
        if (n2 > 0.0f && n2 < INFINITY) {
            const float inv = 1.0f / sqrtf(n2);
            bw = aq.x * inv; bx = aq.y * inv; by = aq.z * inv; bz = aq.w * inv;
        }
        if (!q.cov_mode) {   // q_b (x) q_rest
            o1.x = ((bw * r1.x - bx * r1.y) - by * r1.z) - bz * r1.w;
            o1.y = ((bw * r1.y + bx * r1.x) + by * r1.w) - bz * r1.z;
            o1.z = ((bw * r1.z - bx * r1.w) + by * r1.x) + bz * r1.y;
            o1.w = ((bw * r1.w + bx * r1.z) - by * r1.y) + bz * r1.x;
        } else {             // R_b Sigma R_b^T
            const float R[3][3] = {{1.0f - 2.0f * (by * by + bz * bz), 2.0f * (bx * by - bw * bz), 2.0f * (bx * bz + bw * by)},
                                   {2.0f * (bx * by + bw * bz), 1.0f - 2.0f * (bx * bx + bz * bz), 2.0f * (by * bz - bw * bx)},
                                   {2.0f * (bx * bz - bw * by), 2.0f * (by * bz + bw * bx), 1.0f - 2.0f * (bx * bx + by * by)}};
            const float S[3][3] = {{r1.x, r1.y, r1.z}, {r1.y, r1.w, r2.x}, {r1.z, r2.x, r2.y}};
            float T[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) T[i][k] = (R[i][0] * S[0][k] + R[i][1] * S[1][k]) + R[i][2] * S[2][k];
            auto out = [&](int i, int k) { return (T[i][0] * R[k][0] + T[i][1] * R[k][1]) + T[i][2] * R[k][2]; };
            o1 = make_float4(out(0, 0), out(0, 1), out(0, 2), out(1, 1));
            o2.x = out(1, 2);
            o2.y = out(2, 2);
        }
    }
    q.g0[j] = o0;
    q.g1[j] = o1;
    q.g2[j] = o2;
}

template <bool LDS>
void launch_deform(hipStream_t st, const SasDeform &q, unsigned blocks)
{
    if (q.kp <= 4) hipLaunchKernelGGL((k_deform<LDS, 4>), dim3(blocks), dim3(kThreads), 0, st, q);
    else hipLaunchKernelGGL((k_deform<LDS, 8>), dim3(blocks), dim3(kThreads), 0, st, q);
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_skin)

void sas_launch_knn_cross(hipStream_t st, const SasKnnCross &q)
{
    if (q.n <= 0) return;
    const unsigned blocks = (unsigned)((q.n + kThreads - 1) / kThreads);
    if (q.k <= 3) hipLaunchKernelGGL(k_knn_cross<3>, dim3(blocks), dim3(kThreads), 0, st, q);
    else hipLaunchKernelGGL(k_knn_cross<8>, dim3(blocks), dim3(kThreads), 0, st, q);
}

void sas_launch_skin_bind(hipStream_t st, const SasSkinBind &q)
{
    if (q.n_pad <= 0) return;
    hipLaunchKernelGGL(k_skin_bind, dim3((unsigned)((q.n_pad + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
}

void sas_launch_skin_read(hipStream_t st, const SasSkinRead &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_skin_read, dim3((unsigned)((q.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
}

// the node records, then the planes: two launches on st
void sas_launch_deform(hipStream_t st, const SasDeform &q)
{
    if (q.n <= 0 || q.m <= 0) return;
    hipLaunchKernelGGL(k_skin_nodes, dim3((unsigned)((q.m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
    const unsigned blocks = (unsigned)((q.n + kThreads - 1) / kThreads);
    if (q.lds && (size_t)q.m * sizeof(SasSkinNode) <= SAS_SKIN_LDS_BYTES) launch_deform<true>(st, q, blocks);
    else launch_deform<false>(st, q, blocks);
}
