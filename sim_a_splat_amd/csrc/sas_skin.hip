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
//
// The skin walk: what the forward (k_deform) and both adjoints (k_deform_grad, k_deform_rest_grad) decide alike.  Each rule stands ONCE, as a
// helper or the macro below, and the three kernels use it: an adjoint differentiates the forward as evaluated, every decision a constant, and
// it is the forward's decision because it is the same text.  Nothing is saved by the forward but the node records.  What stays in each
// kernel is the walk's control flow: the loop over the entries, `first live entry sets q_first`, and what the kernel adds.
//   node records    k_skin_nodes, one lane per node: the rows [R | t] as given and R -> the unit quaternion wxyz, by the branch of the largest
//                   of (trace, R00, R11, R22) (quat_branch); the 64-byte record (SasSkinNode).  NodeRecords<LDS> reads them: staged in LDS by
//                   every workgroup (m * 64 B within SAS_SKIN_LDS_BYTES), else from global memory -- the same values, so the same bits.
//   live entries    SkinEntries<KP>: a slot's KP = 4 or 8 entries from its skin planes.  LIVE (SKIN_LIVE) are those with 0 <= index < m and weight > 0;
//                   every other entry is ignored, so no index reaches memory unchecked.  W = sum_j w_j over the live entries, in entry order.
//   blend           QuatBlend: q_b = normalize(sum_j s_j w_j q_j) over the live entries in entry order, s_j = -1 where dot(q_j, q_first) < 0
//                   (q_first: the first live entry's).
//   fallback        a sum of norm zero or not finite gives q_b = q_first (QuatBlend::unit).
//   R_b             quat_matrix: the matrix of q_b.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_); tests/tools/skin_ref.py restates it.
//
//   k_deform<LDS,KP> one lane per slot: the rest planes and the slot's skin planes -> g0, g1, g2.
//                     no live entry: the three planes are the rest planes' bits
//                     mean:     m' = m + (sum_j w_j ((R_j m + t_j) - m)) / W, in entry order; R m + t = ((r0 x + r1 y) + r2 z) + t
//                     quaternion scenes: g1 = q_b (x) q_rest (Hamilton, not renormalised: the projection normalises), scales untouched
//                     covariance scenes: Sigma' = R_b Sigma_rest R_b^T
//                   Opacity, the group-id bits and g2.z of a covariance scene are the rest planes' bits.
//
// The adjoint (sas_scene_deform_backward): from per-Gaussian gradients of the deformed means and orientations to the gradient of every node's
// twelve entries [R | t], each an independent variable.
//   k_deform_grad<LDS,STAGED,KP>  one lane per slot, a persistent grid walking the slots with a stride; its LDS is the accumulator's, so the
//                   quaternions come from global memory, and without an orientation gradient they are not read at all.  On top of the walk
//                   (with the index of the first live entry) it forms one 16-float ROW per live entry: dt (3) = (w_j / W) g, the mean path's
//                   dR (9) = (w_j / W) g m_rest^T, dq_j (4) = s_j w_j da with da = (dq_b - q_b (q_b . dq_b)) / |a| (fallback: dq_b to the first
//                   live entry, nothing to the others).  dq_b: quaternion scenes, the product of h with q_rest that transposes q_b (x) q_rest;
//                   covariance scenes, dR_b = 2 G R_b Sigma (G the symmetric matrix of the six, off-diagonals halved) through the matrix of
//                   q_b.  The rows are summed per node into acc [m,16], zeroed on the stream by every call.
//   k_skin_nodes_grad  one lane per node: acc row -> the 12 outputs.  dt and dR as summed, plus du = (dq - q (q . dq)) / |u| through the transpose of
//                   the branch's linear map R -> u.  A node no live entry names reads a zero row and writes exact zeros.
// Sizing.  At a million Gaussians and k = 4 there are 4 M rows of 64 B: 256 MB of adds.  Straight to memory that is 0.2 ms at best at the chip-wide
// float-atomic rate of about 1.3 TB/s, and the shape is against it: one lane per row is the 64-rows-per-instruction shape (about 17x slower), and
// with M = 64 every add lands in 4 KB, the contended case.  So the rows are summed on chip first: while m * 64 B fits the budget (SAS_SKIN_GRAD_LDS
// bytes, SAS_SKIN_GRAD_LDS_BYTES by default; 0: never) every workgroup keeps acc in LDS, adds there with LDS float atomics and flushes ONCE with global float
// atomics over contiguous floats -- a wave-instruction covers 256 contiguous bytes, 4 node rows, the full-rate shape; zeros are not sent.  The grid
// is persistent, as many workgroups per CU as their LDS allows and 4 at most, so the flush costs blocks * m * 64 B and not N k * 64 B.  Above the
// budget the rows go to global memory.  STAGED: a workgroup's 256 rows of one entry pass through 16 KB of LDS and come out transposed, 16 lanes per
// row, so that an atomic instruction covers 4 whole 64-B rows; not STAGED: every lane adds its own 16 floats, 64 rows per instruction.  Both forms
// exist for both paths (SAS_SKIN_GRAD_STAGED=0/1 forces one).  Measured (profiles/deform_grad.txt; a million Gaussians, k = 4): on the global path
// the staged form is 5 to 7 times the other (m = 16384: 0.63 against 4.6 ms; 64-B segments reach 0.3 to 0.45 of the 1.3 TB/s), so it is what that
// path takes.  The LDS path beats it at every m that fits (m = 2048: 0.46 against 1.10 ms; m = 64: 0.39 against 8.6), so the budget's default is its
// ceiling, SAS_SKIN_GRAD_LDS_MAX.  Within the LDS path the staged form wins while the accumulator is small (m = 256: 0.39 against 0.47 ms: the LDS
// adds of a wave then land in 4 rows and not in 64) and loses once the 17 KB of stage cost workgroups per CU (m = 1024: 0.50 against 0.46): staged up
// to SAS_SKIN_GRAD_STAGED_LDS_BYTES.  Combining equal nodes within a wave in front of the LDS add was not built: at m = 64 the LDS path runs in the
// time it runs in at m = 2048, so the adds' conflicts do not bind.
// Residency: 60 to 70 VGPRs (7 or 8 waves per SIMD by registers, no spills); what bounds it is the LDS, all of it dynamic: 17 408 B of stage and
// m * 64 B of sums -- 4 workgroups per CU up to m = 368 staged, 2 at m = 1024 and 1 at m = 2048 with every lane adding its own row.
// Float atomics: the sums depend on arrival order and vary in their last bits from run to run; zero rows and zero upstream give exact zeros.
//
// The adjoint to the REST arrays (sas_scene_deform_backward_rest): the same gradients of the deformed arrays -> gradients of the Gaussians that are
// stored, ADDED to the caller's arrays (the deformation differs per time step: the sum over time steps is taken here).
//   k_deform_rest_grad<LDS,KP>  one lane per slot, k_deform's shape: the gradients are gathered at perm[slot] as k_adam_scene gathers them
//                   (load_row, as k_deform_grad gathers them) and the results are added at the same caller's index.  The forward is linear
//                   in each rest array, so no rest plane is read, and the mean path is computed only where d_means is given:
//                     mean:       d_m = g + (sum_j w_j ((R_j^T g) - g)) / W, in entry order; R^T g = (r0 gx + r1 gy) + r2 gz by columns
//                     quaternion: d_q_rest = conj(q_b) (x) h, the transpose of the left product by q_b
//                     covariance: dSigma = R_b^T G R_b, G the symmetric matrix of the six with the off-diagonals halved; an off-diagonal of
//                                 the result's six is the sum of its two entries (render_backward's convention for `covariances`)
//                     no live entry: the gradient is added as it is (SAS_DEFORM_REST_BOUND_ONLY: nothing is added)
//                   Each output depends on its own input alone, and a zero input adds zeros.  No atomics: a Gaussian has one lane, the same inputs
//                   give the same bits on every run and on both paths.
#include "sas_device.h"

#include <type_traits>

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

// ---- the skin walk's shared pieces (the header: each rule once) ---------------------------------------------------------------------------------
// R -> u = 4 c times the quaternion wxyz, c its largest component: no cancellation in the term that is squared.
// Returns the branch; inv = 1 / |u|.
DEV int quat_branch(const float (&R)[3][3], float4 &u, float &inv)
{
    const float r00 = R[0][0], r01 = R[0][1], r02 = R[0][2], r10 = R[1][0], r11 = R[1][1], r12 = R[1][2], r20 = R[2][0], r21 = R[2][1], r22 = R[2][2];
    const float tr = (r00 + r11) + r22;
    int branch;
    float w, x, y, z;
    if (tr >= r00 && tr >= r11 && tr >= r22) {
        branch = 0; w = 1.0f + tr; x = r21 - r12; y = r02 - r20; z = r10 - r01;
    } else if (r00 >= r11 && r00 >= r22) {
        branch = 1; w = r21 - r12; x = ((1.0f + r00) - r11) - r22; y = r01 + r10; z = r02 + r20;
    } else if (r11 >= r22) {
        branch = 2; w = r02 - r20; x = r01 + r10; y = ((1.0f + r11) - r00) - r22; z = r12 + r21;
    } else {
        branch = 3; w = r10 - r01; x = r02 + r20; y = r12 + r21; z = ((1.0f + r22) - r00) - r11;
    }
    inv = 1.0f / sqrtf(((w * w + x * x) + y * y) + z * z);
    u = make_float4(w, x, y, z);
    return branch;
}

// The ONE live test: entry (id, w) under m nodes.  A macro, not a function: a function is optimised on its own before it is inlined and hands
// the kernel one flag, and the kernels then branch once per entry where this text branches on the index first -- other kernels
// (profiles/skin_refactor_isa_gate.txt), measured slower.  For the same reason the helpers below hold no decision of the walk, only its
// straight-line pieces, and the loops over planes and entries stay in the kernels.
#define SKIN_LIVE(id, w, m) ((id) >= 0 && (id) < (m) && (w) > 0.0f)

// a slot's entries; a lane that loads nothing holds none that is live
template <int KP>
struct SkinEntries {
    int id[KP];
    float wt[KP];
    DEV SkinEntries()
    {
#pragma unroll
        for (int e = 0; e < KP; ++e) { id[e] = -1; wt[e] = 0.0f; }
    }
    // plane p of the skin planes: entries 4p .. 4p + 3 of slot j
    DEV void load(int p, const int4 *idx, const float4 *w, long long n_pad, long long j)
    {
        const int4 v = idx[(long long)p * n_pad + j];
        const float4 u = w[(long long)p * n_pad + j];
        id[4 * p] = v.x; id[4 * p + 1] = v.y; id[4 * p + 2] = v.z; id[4 * p + 3] = v.w;
        wt[4 * p] = u.x; wt[4 * p + 1] = u.y; wt[4 * p + 2] = u.z; wt[4 * p + 3] = u.w;
    }
};

// the node records as float4 parts (0..2: the rows [R | t], 3: the quaternion); LDS: staged by the whole workgroup in lds, SAS_IN under `code`
template <bool LDS>
struct NodeRecords {
    const float4 *g_nodes;
    float4 *s_nodes;
    DEV NodeRecords(const SasSkinNode *nodes, int m, float4 *lds = nullptr, int code = 0) : g_nodes(reinterpret_cast<const float4 *>(nodes)), s_nodes(lds)
    {
        if constexpr (LDS) {
            for (int t = threadIdx.x; t < 4 * m; t += kThreads)
                if (SAS_IN(t, SAS_SKIN_LDS_BYTES / 16, code)) s_nodes[t] = g_nodes[t];
            __syncthreads();
        }
    }
    DEV float4 rec(int node, int part) const
    {
        if constexpr (LDS) return s_nodes[4 * node + part];
        else return g_nodes[4 * (long long)node + part];
    }
};

// the sign-aligned quaternion sum over the live entries, in entry order
struct QuatBlend {
    float4 f = make_float4(1.0f, 0.0f, 0.0f, 0.0f), aq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // q_first, the sum
    // s_j w_j
    DEV float sign(const float4 qn, float we) const
    {
        const float dot = ((qn.x * f.x + qn.y * f.y) + qn.z * f.z) + qn.w * f.w;
        return dot < 0.0f ? -we : we;
    }
    DEV void add(const float4 qn, float we)
    {
        const float sw = sign(qn, we);
        aq.x = aq.x + sw * qn.x;
        aq.y = aq.y + sw * qn.y;
        aq.z = aq.z + sw * qn.z;
        aq.w = aq.w + sw * qn.w;
    }
    // q_b wxyz, normalised: true; or (the sum's norm zero or not finite) q_first as it stands: false.  inv = 1 / |sum|, or 1
    DEV bool unit(float4 &qb, float &inv) const
    {
        const float n2 = ((aq.x * aq.x + aq.y * aq.y) + aq.z * aq.z) + aq.w * aq.w;
        qb = f;
        inv = 1.0f;
        if (n2 > 0.0f && n2 < INFINITY) {
            inv = 1.0f / sqrtf(n2);
            qb = make_float4(aq.x * inv, aq.y * inv, aq.z * inv, aq.w * inv);
            return true;
        }
        return false;
    }
};

// the matrix of the unit quaternion (bw, bx, by, bz)
DEV void quat_matrix(float (&R)[3][3], float bw, float bx, float by, float bz)
{
    R[0][0] = 1.0f - 2.0f * (by * by + bz * bz); R[0][1] = 2.0f * (bx * by - bw * bz); R[0][2] = 2.0f * (bx * bz + bw * by);
    R[1][0] = 2.0f * (bx * by + bw * bz); R[1][1] = 1.0f - 2.0f * (bx * bx + bz * bz); R[1][2] = 2.0f * (by * bz - bw * bx);
    R[2][0] = 2.0f * (bx * bz - bw * by); R[2][1] = 2.0f * (by * bz + bw * bx); R[2][2] = 1.0f - 2.0f * (bx * bx + by * by);
}

// one caller's row read: v[c] = in[at + c] (the adjoints' gather of an upstream gradient at the caller's index)
template <int C>
DEV void load_row(const float *in, long long at, float *v)
{
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = in[at + c];
}

// launch(KP as an integral constant): the instantiation for kp entries per slot
template <typename F>
void with_kp(int kp, F &&launch)
{
    if (kp <= 4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 8>{});
}

// ---- the forward ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_skin_nodes(const SasDeform q)
{
    const int a = blockIdx.x * kThreads + threadIdx.x;
    if (a >= q.m) return;
    const float *G = q.node_Rt + 12 * (long long)a;
    const float R[3][3] = {{G[0], G[1], G[2]}, {G[4], G[5], G[6]}, {G[8], G[9], G[10]}};
    float4 u;
    float inv;
    quat_branch(R, u, inv);
    if (!SAS_IN(a, q.m, 1507)) return;
    float4 *rec = reinterpret_cast<float4 *>(q.nodes + a);
    rec[0] = make_float4(G[0], G[1], G[2], G[3]);
    rec[1] = make_float4(G[4], G[5], G[6], G[7]);
    rec[2] = make_float4(G[8], G[9], G[10], G[11]);
    rec[3] = make_float4(u.x * inv, u.y * inv, u.z * inv, u.w * inv);
}

template <bool LDS, int KP>
__global__ __launch_bounds__(kThreads) void k_deform(const SasDeform q)
{
    __shared__ float4 s_nodes[LDS ? SAS_SKIN_LDS_BYTES / 16 : 1];
    const NodeRecords<LDS> nodes(q.nodes, q.m, s_nodes, 1508);
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // slot
    if (j >= q.n || !SAS_IN(j, q.n_pad, 1509)) return;
    const float4 r0 = q.r0[j], r1 = q.r1[j], r2 = q.r2[j];
    SkinEntries<KP> en;
#pragma unroll
    for (int p = 0; p < KP / 4; ++p) en.load(p, q.idx, q.w, q.n_pad, j);
    float ax = 0.0f, ay = 0.0f, az = 0.0f, W = 0.0f;
    QuatBlend blend;
    bool any = false;
#pragma unroll
    for (int e = 0; e < KP; ++e) {
        const float we = en.wt[e];
        if (!SKIN_LIVE(en.id[e], we, q.m)) continue;
        const float4 a = nodes.rec(en.id[e], 0), b = nodes.rec(en.id[e], 1), c = nodes.rec(en.id[e], 2), qn = nodes.rec(en.id[e], 3);
        const float y0 = ((a.x * r0.x + a.y * r0.y) + a.z * r0.z) + a.w;
        const float y1 = ((b.x * r0.x + b.y * r0.y) + b.z * r0.z) + b.w;
        const float y2 = ((c.x * r0.x + c.y * r0.y) + c.z * r0.z) + c.w;
        ax = ax + we * (y0 - r0.x);
        ay = ay + we * (y1 - r0.y);
        az = az + we * (y2 - r0.z);
        W = W + we;
        if (!any) blend.f = qn;
        any = true;
        blend.add(qn, we);
    }
    float4 o0 = r0, o1 = r1, o2 = r2;
    if (any) {
        o0.x = r0.x + ax / W;
        o0.y = r0.y + ay / W;
        o0.z = r0.z + az / W;
        float4 qb;
        float inv;
        blend.unit(qb, inv);
        const float bw = qb.x, bx = qb.y, by = qb.z, bz = qb.w;
        if (!q.cov_mode) {   // q_b (x) q_rest
            o1.x = ((bw * r1.x - bx * r1.y) - by * r1.z) - bz * r1.w;
            o1.y = ((bw * r1.y + bx * r1.x) + by * r1.w) - bz * r1.z;
            o1.z = ((bw * r1.z - bx * r1.w) + by * r1.x) + bz * r1.y;
            o1.w = ((bw * r1.w + bx * r1.z) - by * r1.y) + bz * r1.x;
        } else {             // R_b Sigma R_b^T
            float R[3][3];
            quat_matrix(R, bw, bx, by, bz);
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

// ---- the adjoint ---------------------------------------------------------------------------------------------------------------------------
constexpr int kRow = SAS_SKIN_GRAD_ROW;                  // floats of a row: dt 3, dR 9, dq 4
constexpr int kStageFloats = kThreads * kRow;            // a workgroup's rows of one entry
static_assert(kRow == 16 && kThreads % kRow == 0, "16 lanes per row in the staged flush");

// one float into a row of acc: LDS or global, both no-return float atomics
DEV void add_to(float *acc, long long at, float v) { atomicAdd(acc + at, v); }

template <bool LDS, bool STAGED, int KP>
__global__ __launch_bounds__(kThreads) void k_deform_grad(const SasDeformGrad q)
{
    extern __shared__ float s_mem[];
    float *s_stage = s_mem;                                            // [256][16] (STAGED)
    int *s_node = reinterpret_cast<int *>(s_mem + kStageFloats);       // [256]     (STAGED)
    float *s_acc = s_mem + (STAGED ? kStageFloats + kThreads : 0);     // [m][16]   (LDS)
    const int tid = threadIdx.x;
    const int n_acc = q.m * kRow;
    if constexpr (LDS) {
        for (int t = tid; t < n_acc; t += kThreads) s_acc[t] = 0.0f;
        __syncthreads();
    }
    float *acc = LDS ? s_acc : q.acc;
    const NodeRecords<false> nodes(q.nodes, q.m);            // (the LDS is the accumulator's)
    const bool rot = q.d_quats != nullptr || q.d_cov6 != nullptr;
    const int n_col = rot ? kRow : 12;                                 // without an orientation gradient the dq columns are never touched
    // the walk is the same for every lane of the workgroup: the barriers of the staged form are met by all
    for (long long base = (long long)blockIdx.x * kThreads; base < q.n; base += (long long)gridDim.x * kThreads) {
        const long long j = base + tid;   // slot
        const bool active = j < q.n && SAS_IN(j, q.n_pad, 1510);
        SkinEntries<KP> en;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
        float g[3] = {0.0f, 0.0f, 0.0f};
        float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (active) {
            r0 = q.r0[j]; r1 = q.r1[j]; r2 = q.r2[j];
        #pragma unroll
    for (int p = 0; p < KP / 4; ++p) en.load(p, q.idx, q.w, q.n_pad, j);
            const long long i = q.perm[j];   // the caller's index
            if (SAS_IN(i, q.n, 1511)) {
                if (q.d_means) load_row<3>(q.d_means, 3 * i, g);
                if (q.d_quats) load_row<4>(q.d_quats, 4 * i, h);
                if (q.d_cov6) load_row<6>(q.d_cov6, 6 * i, h);
            }
        }
        // the forward's sums again: W, a, q_first
        float W = 0.0f;
        QuatBlend blend;
        bool any = false;
        int first = -1;
#pragma unroll
        for (int e = 0; e < KP; ++e) {
            const float we = en.wt[e];
            if (!SKIN_LIVE(en.id[e], we, q.m)) continue;
            W = W + we;
            if (!rot) { any = true; continue; }
            const float4 qn = nodes.rec(en.id[e], 3);
            if (!any) { blend.f = qn; first = e; }
            any = true;
            blend.add(qn, we);
        }
        // dq_b, then da (or, in the fallback, dq_first)
        float4 da = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool fallback = false;
        if (any && rot) {
            float4 qb;
            float inv;
            fallback = !blend.unit(qb, inv);
            const float bw = qb.x, bx = qb.y, by = qb.z, bz = qb.w;
            float dw, dx, dy, dz;
            if (!q.cov_mode) {   // q' = q_b (x) q_rest, bilinear: h times the conjugate of q_rest
                dw = ((h[0] * r1.x + h[1] * r1.y) + h[2] * r1.z) + h[3] * r1.w;
                dx = ((h[1] * r1.x - h[0] * r1.y) - h[2] * r1.w) + h[3] * r1.z;
                dy = ((h[2] * r1.x - h[0] * r1.z) + h[1] * r1.w) - h[3] * r1.y;
                dz = ((h[3] * r1.x - h[0] * r1.w) - h[1] * r1.z) + h[2] * r1.y;
            } else {             // Sigma' = R_b Sigma R_b^T: D = dR_b = 2 G (R_b Sigma), then the matrix of q_b
                float R[3][3];
                quat_matrix(R, bw, bx, by, bz);
                const float S[3][3] = {{r1.x, r1.y, r1.z}, {r1.y, r1.w, r2.x}, {r1.z, r2.x, r2.y}};
                const float G[3][3] = {{2.0f * h[0], h[1], h[2]}, {h[1], 2.0f * h[3], h[4]}, {h[2], h[4], 2.0f * h[5]}};   // 2 G
                float T[3][3], D[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int k = 0; k < 3; ++k) T[a][k] = (R[a][0] * S[0][k] + R[a][1] * S[1][k]) + R[a][2] * S[2][k];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int k = 0; k < 3; ++k) D[a][k] = (G[a][0] * T[0][k] + G[a][1] * T[1][k]) + G[a][2] * T[2][k];
                dw = 2.0f * (((bz * (D[1][0] - D[0][1]) + by * (D[0][2] - D[2][0])) + bx * (D[2][1] - D[1][2])));
                dx = 2.0f * ((((by * (D[0][1] + D[1][0]) + bz * (D[0][2] + D[2][0])) + bw * (D[2][1] - D[1][2])) - 2.0f * bx * (D[1][1] + D[2][2])));
                dy = 2.0f * ((((bx * (D[0][1] + D[1][0]) + bz * (D[1][2] + D[2][1])) + bw * (D[0][2] - D[2][0])) - 2.0f * by * (D[0][0] + D[2][2])));
                dz = 2.0f * ((((bx * (D[0][2] + D[2][0]) + by * (D[1][2] + D[2][1])) + bw * (D[1][0] - D[0][1])) - 2.0f * bz * (D[0][0] + D[1][1])));
            }
            if (fallback) {
                da = make_float4(dw, dx, dy, dz);
            } else {
                const float dot = ((bw * dw + bx * dx) + by * dy) + bz * dz;
                da = make_float4((dw - bw * dot) * inv, (dx - bx * dot) * inv, (dy - by * dot) * inv, (dz - bz * dot) * inv);
            }
        }
        // one row per live entry
#pragma unroll
        for (int e = 0; e < KP; ++e) {
            const float we = en.wt[e];
            const bool live = SKIN_LIVE(en.id[e], we, q.m);
            float row[kRow];
#pragma unroll
            for (int c = 0; c < kRow; ++c) row[c] = 0.0f;
            if (live) {
                const float cw = we / W;
                const float cg[3] = {cw * g[0], cw * g[1], cw * g[2]};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    row[a] = cg[a];
                    row[3 + 3 * a] = cg[a] * r0.x;
                    row[4 + 3 * a] = cg[a] * r0.y;
                    row[5 + 3 * a] = cg[a] * r0.z;
                }
                if (rot) {
                    float sw = e == first ? 1.0f : 0.0f;   // the fallback: q_b is q_first as it stands
                    if (!fallback) sw = blend.sign(nodes.rec(en.id[e], 3), we);
                    row[12] = sw * da.x; row[13] = sw * da.y; row[14] = sw * da.z; row[15] = sw * da.w;
                }
            }
            if constexpr (STAGED) {
                if (SAS_IN(tid, kThreads, 1512)) {
                    float4 *dst = reinterpret_cast<float4 *>(s_stage + tid * kRow);
#pragma unroll
                    for (int c = 0; c < kRow / 4; ++c) dst[c] = make_float4(row[4 * c], row[4 * c + 1], row[4 * c + 2], row[4 * c + 3]);
                    s_node[tid] = live ? en.id[e] : -1;
                }
                __syncthreads();
                const int col = tid % kRow;
#pragma unroll 4
                for (int r = tid / kRow; r < kThreads; r += kThreads / kRow) {   // a wave: 4 rows of 16 lanes
                    const int node = s_node[r];
                    if (node < 0 || col >= n_col) continue;
                    const float v = s_stage[r * kRow + col];
                    if (SAS_IN(node, q.m, 1513)) add_to(acc, (long long)node * kRow + col, v);
                }
                __syncthreads();   // the stage is free for the next entry
            } else {
                if (live && SAS_IN(en.id[e], q.m, 1514)) {
#pragma unroll
                    for (int c = 0; c < kRow; ++c)
                        if (c < n_col) add_to(acc, (long long)en.id[e] * kRow + c, row[c]);
                }
            }
        }
    }
    if constexpr (LDS) {   // one flush: contiguous floats, 4 node rows per wave-instruction; zeros stay at home
        __syncthreads();
        for (int t = tid; t < n_acc; t += kThreads) {
            const float v = s_acc[t];
            if (v != 0.0f && SAS_IN(t, n_acc, 1515)) atomicAdd(q.acc + t, v);
        }
    }
}

// acc row -> the node's 12 outputs: rows [dR | dt]
__global__ __launch_bounds__(kThreads) void k_skin_nodes_grad(const SasDeformGrad q)
{
    const int a = blockIdx.x * kThreads + threadIdx.x;
    if (a >= q.m || !SAS_IN(a, q.m, 1516)) return;
    const float4 *A = reinterpret_cast<const float4 *>(q.acc + (long long)a * kRow);
    const float4 a0 = A[0], a1 = A[1], a2 = A[2], dq = A[3];
    const float dt[3] = {a0.x, a0.y, a0.z};
    float dR[3][3] = {{a0.w, a1.x, a1.y}, {a1.z, a1.w, a2.x}, {a2.y, a2.z, a2.w}};
    if (q.d_quats != nullptr || q.d_cov6 != nullptr) {
        const float4 *rec = reinterpret_cast<const float4 *>(q.nodes + a);
        const float4 G0 = rec[0], G1 = rec[1], G2 = rec[2], qn = rec[3];
        const float R[3][3] = {{G0.x, G0.y, G0.z}, {G1.x, G1.y, G1.z}, {G2.x, G2.y, G2.z}};
        float4 u;
        float inv;
        const int branch = quat_branch(R, u, inv);
        const float dot = ((qn.x * dq.x + qn.y * dq.y) + qn.z * dq.z) + qn.w * dq.w;
        const float uw = (dq.x - qn.x * dot) * inv, ux = (dq.y - qn.y * dot) * inv, uy = (dq.z - qn.z * dot) * inv, uz = (dq.w - qn.w * dot) * inv;
        // the transpose of the branch's map R -> u
        if (branch == 0) {
            dR[0][0] += uw; dR[1][1] += uw; dR[2][2] += uw;
            dR[2][1] += ux; dR[1][2] -= ux; dR[0][2] += uy; dR[2][0] -= uy; dR[1][0] += uz; dR[0][1] -= uz;
        } else if (branch == 1) {
            dR[2][1] += uw; dR[1][2] -= uw;
            dR[0][0] += ux; dR[1][1] -= ux; dR[2][2] -= ux;
            dR[0][1] += uy; dR[1][0] += uy; dR[0][2] += uz; dR[2][0] += uz;
        } else if (branch == 2) {
            dR[0][2] += uw; dR[2][0] -= uw;
            dR[0][1] += ux; dR[1][0] += ux;
            dR[1][1] += uy; dR[0][0] -= uy; dR[2][2] -= uy;
            dR[1][2] += uz; dR[2][1] += uz;
        } else {
            dR[1][0] += uw; dR[0][1] -= uw;
            dR[0][2] += ux; dR[2][0] += ux; dR[1][2] += uy; dR[2][1] += uy;
            dR[2][2] += uz; dR[0][0] -= uz; dR[1][1] -= uz;
        }
    }
    float *o = q.out + 12 * (long long)a;   // (the caller's array: no alignment beyond a float's is asked of it)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[4 * i] = dR[i][0]; o[4 * i + 1] = dR[i][1]; o[4 * i + 2] = dR[i][2]; o[4 * i + 3] = dt[i];
    }
}

// ---- the adjoint to the rest arrays ---------------------------------------------------------------------------------------------------------
// one caller's row added to: out[at + c] += v[c] (the caller's arrays: no alignment beyond a float's is asked of them)
template <int C>
DEV void add_row(float *out, long long at, const float (&v)[C])
{
#pragma unroll
    for (int c = 0; c < C; ++c) out[at + c] = out[at + c] + v[c];
}

template <bool LDS, int KP>
__global__ __launch_bounds__(kThreads) void k_deform_rest_grad(const SasDeformRestGrad q)
{
    __shared__ float4 s_nodes[LDS ? SAS_SKIN_LDS_BYTES / 16 : 1];
    const NodeRecords<LDS> nodes(q.nodes, q.m, s_nodes, 1517);
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;   // slot
    if (j >= q.n || !SAS_IN(j, q.n_pad, 1518)) return;
    const long long i = q.perm[j];                                     // the caller's index
    if (!SAS_IN(i, q.n, 1519)) return;
    SkinEntries<KP> en;
#pragma unroll
    for (int p = 0; p < KP / 4; ++p) en.load(p, q.idx, q.w, q.n_pad, j);
    const bool rot = q.d_quats != nullptr || q.d_cov6 != nullptr;
    float g[3] = {0.0f, 0.0f, 0.0f};
    float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (q.d_means) load_row<3>(q.d_means, 3 * i, g);
    if (q.d_quats) load_row<4>(q.d_quats, 4 * i, h);
    if (q.d_cov6) load_row<6>(q.d_cov6, 6 * i, h);
    // the forward's walk over the live entries: W and a again, and the mean path's sum_j w_j ((R_j^T g) - g)
    float ax = 0.0f, ay = 0.0f, az = 0.0f, W = 0.0f;
    QuatBlend blend;
    bool any = false;
#pragma unroll
    for (int e = 0; e < KP; ++e) {
        const float we = en.wt[e];
        if (!SKIN_LIVE(en.id[e], we, q.m)) continue;
        W = W + we;
        if (q.d_means) {
            const float4 a = nodes.rec(en.id[e], 0), b = nodes.rec(en.id[e], 1), c = nodes.rec(en.id[e], 2);
            const float u0 = (a.x * g[0] + b.x * g[1]) + c.x * g[2];
            const float u1 = (a.y * g[0] + b.y * g[1]) + c.y * g[2];
            const float u2 = (a.z * g[0] + b.z * g[1]) + c.z * g[2];
            ax = ax + we * (u0 - g[0]);
            ay = ay + we * (u1 - g[1]);
            az = az + we * (u2 - g[2]);
        }
        if (rot) {
            const float4 qn = nodes.rec(en.id[e], 3);
            if (!any) blend.f = qn;
            blend.add(qn, we);
        }
        any = true;
    }
    if (!any) {   // the forward copied the rest bits: the gradient passes through as it is
        if (q.bound_only) return;
        if (q.d_means) add_row<3>(q.o_means, 3 * i, g);
        if (q.d_quats) add_row<4>(q.o_quats, 4 * i, {h[0], h[1], h[2], h[3]});
        if (q.d_cov6) add_row<6>(q.o_cov6, 6 * i, h);
        return;
    }
    if (q.d_means) add_row<3>(q.o_means, 3 * i, {g[0] + ax / W, g[1] + ay / W, g[2] + az / W});
    if (!rot) return;
    float4 qb;
    float inv;
    blend.unit(qb, inv);
    const float bw = qb.x, bx = qb.y, by = qb.z, bz = qb.w;
    if (q.d_quats) {   // q' = q_b (x) q_rest: the transpose of the left product, the conjugate of q_b times h
        add_row<4>(q.o_quats, 4 * i, {((bw * h[0] + bx * h[1]) + by * h[2]) + bz * h[3],
                                      ((bw * h[1] - bx * h[0]) + bz * h[2]) - by * h[3],
                                      ((bw * h[2] - by * h[0]) - bz * h[1]) + bx * h[3],
                                      ((bw * h[3] - bz * h[0]) + by * h[1]) - bx * h[2]});
    } else {              // Sigma' = R_b Sigma R_b^T: dSigma = R_b^T G R_b, G the symmetric matrix of the six with its off-diagonals halved
        float R[3][3];
        quat_matrix(R, bw, bx, by, bz);
        const float G[3][3] = {{h[0], 0.5f * h[1], 0.5f * h[2]}, {0.5f * h[1], h[3], 0.5f * h[4]}, {0.5f * h[2], 0.5f * h[4], h[5]}};
        float T[3][3];   // R_b^T G
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) T[a][k] = (R[0][a] * G[0][k] + R[1][a] * G[1][k]) + R[2][a] * G[2][k];
        auto out = [&](int a, int k) { return (T[a][0] * R[0][k] + T[a][1] * R[1][k]) + T[a][2] * R[2][k]; };
        // an off-diagonal of the six stands for two entries of Sigma: both halves' gradients add
        add_row<6>(q.o_cov6, 6 * i, {out(0, 0), out(0, 1) + out(1, 0), out(0, 2) + out(2, 0), out(1, 1), out(1, 2) + out(2, 1), out(2, 2)});
    }
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
    sas_launch_deform_planes(st, q);
}

// the planes alone, from the records q.nodes holds: one launch on st
void sas_launch_deform_planes(hipStream_t st, const SasDeform &q)
{
    if (q.n <= 0 || q.m <= 0) return;
    const dim3 blocks((unsigned)((q.n + kThreads - 1) / kThreads));
    const bool lds = q.lds && (size_t)q.m * sizeof(SasSkinNode) <= SAS_SKIN_LDS_BYTES;
    with_kp(q.kp, [&](auto KP) {
        if (lds) hipLaunchKernelGGL((k_deform<true, decltype(KP)::value>), blocks, dim3(kThreads), 0, st, q);
        else hipLaunchKernelGGL((k_deform<false, decltype(KP)::value>), blocks, dim3(kThreads), 0, st, q);
    });
}

// the rest arrays' gradients, added to: one launch on st
void sas_launch_deform_rest_grad(hipStream_t st, const SasDeformRestGrad &q)
{
    if (q.n <= 0 || q.m <= 0) return;
    const dim3 blocks((unsigned)((q.n + kThreads - 1) / kThreads));
    const bool lds = q.lds && (size_t)q.m * sizeof(SasSkinNode) <= SAS_SKIN_LDS_BYTES;
    with_kp(q.kp, [&](auto KP) {
        if (lds) hipLaunchKernelGGL((k_deform_rest_grad<true, decltype(KP)::value>), blocks, dim3(kThreads), 0, st, q);
        else hipLaunchKernelGGL((k_deform_rest_grad<false, decltype(KP)::value>), blocks, dim3(kThreads), 0, st, q);
    });
}

size_t sas_deform_grad_lds_bytes(int m, bool lds, bool staged)
{
    return (staged ? sizeof(float) * (size_t)(kStageFloats + kThreads) : 0) + (lds ? sizeof(float) * kRow * (size_t)m : 0);
}

// the rows into acc (zeroed by the caller on st), then the nodes: two launches on st
void sas_launch_deform_grad(hipStream_t st, const SasDeformGrad &q)
{
    if (q.n <= 0 || q.m <= 0 || q.blocks <= 0) return;
    const bool lds = q.lds && sizeof(float) * kRow * (size_t)q.m <= SAS_SKIN_GRAD_LDS_MAX;
    const size_t bytes = sas_deform_grad_lds_bytes(q.m, lds, q.staged != 0);
    auto go = [&](auto kernel) {
        // above 64 KiB a kernel has to ask for its dynamic LDS
        if (bytes > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        hipLaunchKernelGGL(kernel, dim3((unsigned)q.blocks), dim3(kThreads), bytes, st, q);
    };
    with_kp(q.kp, [&](auto KP) {
        constexpr int kp = decltype(KP)::value;
        if (lds && q.staged) go(k_deform_grad<true, true, kp>);
        else if (lds) go(k_deform_grad<true, false, kp>);
        else if (q.staged) go(k_deform_grad<false, true, kp>);
        else go(k_deform_grad<false, false, kp>);
    });
    hipLaunchKernelGGL(k_skin_nodes_grad, dim3((unsigned)((q.m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
}
