// sas_nodes.hip -- the node optimiser and the node driver of the deformable splats on the device (sas_nodes_rigidity, sas_nodes_twist_step,
// sas_nodes_fit_rigid; DESIGN.md 3, "Deformation": the node optimiser, the node driver), hand-written for gfx950 (CDNA4, wave64).  The state -- every node's rows [R | t], the two Adam moments of its
// twist, the rigidity gradient -- is BINARY64: a rotation that is left-multiplied hundreds of times in binary32 drifts away from R^T R = I, and
// sas_scene_deform does not check device arrays.  The float32 rows sas_scene_deform reads are the state rounded ONCE (sas_mcmc.hip's precedent).
// One lane per node, 256-lane workgroups, plain vector loads and stores, no atomics: the same inputs give the same bits.  M <= 65 536 lanes of
// binary64 arithmetic are a launch-bound amount of work (profiles/node_opt.txt), so nothing is staged in LDS but the value's tree sum.
//
//   k_nodes_rigidity   deform.rigidity in gather form: E = sum_i sum_{j in N(i)} |T_i(g_j) - T_j(g_j)|^2 / (m kn), T(x) = R x + t, and dE / d[R | t]
//                      of every node.  Lane i sums its OWN kn edges in slot order -- r = T_i(g_j) - T_j(g_j), d_i += (2 / (m kn)) r [g_j^T | 1] --
//                      and then its INCOMING edges in the reverse table's order (ascending edge number e = k kn + slot with nb[e] == i), every
//                      residual recomputed from T_k and T_i: r = T_k(g_i) - T_i(g_i), d_i -= (2 / (m kn)) r [g_i^T | 1].  Nothing is stored in
//                      between, so the order of every sum is fixed; a hub with in-degree m - 1 is one long lane.  An entry nb outside [0, m) is
//                      ignored, an edge number outside [0, m kn) too, and the reverse ranges are clipped to [0, m kn]: nothing reaches memory
//                      unchecked.  The lane's sum of |r|^2 over its own edges goes through a fixed tree: one partial per workgroup.
//   k_nodes_value      ONE workgroup adds the partials in a fixed order (sas_loss.hip's tail) and writes value = sum / (m kn).
//   k_nodes_twist_step deform._twist_step per node, its operations in its order: the pivot p = R g + t; the gradient G = double(d32) + weight d64;
//                      the twist gradient about p (sum_c A[:,c] x G[:,c] over the four columns, + G[:,3] x p); the two moments; hat = (m1 / c1) /
//                      (sqrt(m2 / c2) + eps); xi = -(lr_rot hat_w, lr_trans hat_v); E = exp(xi) with the series branch below |w| = 1e-8;
//                      R <- E_R R, t <- (E_R (t - p) + E_t) + p; Rt32 = float(Rt64).
//   k_nodes_fit_rigid  deform.transforms_from_positions per (step, node), without an SVD: the members (the node, then its table entries in slot
//                      order; an entry outside [0, m) or with a non-finite moved position is left out), their centroids, the cross-covariance
//                      S = sum (a - ca)(b - cb)^T in member order, Horn's symmetric 4x4 matrix of S, SAS_NODES_FIT_SWEEPS cyclic Jacobi sweeps
//                      for all four eigenpairs, and the quaternion = (1,0,0,0) projected onto the span of the eigenvectors whose eigenvalue
//                      is within SAS_NODES_FIT_GAP of the top one, normalised: the top eigenvector with q_w >= 0 for a neighbourhood of full
//                      rank, the LEAST rotation of all optimal ones for a collinear one, the identity for S = 0; a projection that vanishes
//                      (an exact half turn) takes the top eigenvector as it is.  Always a proper rotation: there is no determinant to correct.
//                      t = moved_i - R rest_i.  Every loop has a compile-time trip count and no branch depends on the data but the first
//                      (the node's own moved position is not finite: [I | 0]), so a poisoned input costs what a clean one costs.
// Arithmetic: IEEE binary64, nothing fused, correctly rounded / and sqrt; sin and cos are the device library's (k_nodes_fit_rigid uses
// neither).  tests/tools/node_opt_ref.py restates the optimiser's kernels, tests/tools/node_fit_ref.py the driver's.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
static_assert(SAS_NODES_MAX_PARTIALS * kThreads >= SAS_KNN_CROSS_MAX_NODES, "one partial per workgroup");

struct Rt64 {
    double v[12];   // rows [R | t]: v[4 a + b]
};

DEV Rt64 load_rt(const double *p, long long node)
{
    Rt64 T;
#pragma unroll
    for (int k = 0; k < 12; ++k) T.v[k] = p[12 * node + k];
    return T;
}

// T(g), row a: ((R[a][0] gx + R[a][1] gy) + R[a][2] gz) + t[a]
DEV double apply_row(const Rt64 &T, int a, double gx, double gy, double gz)
{
    return ((T.v[4 * a] * gx + T.v[4 * a + 1] * gy) + T.v[4 * a + 2] * gz) + T.v[4 * a + 3];
}

// the workgroup's sum of v over its 256 lanes, a fixed tree (lane t += lane t + s, s = 128 .. 1); valid in lane 0
DEV double tree_sum(double *red, int tid, double v)
{
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kThreads) void k_nodes_rigidity(const SasNodesRigidity q)
{
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * kThreads + tid;
    const long long n_edges = (long long)q.m * q.kn;
    const bool active = i < q.m && SAS_IN(i, q.m, 1601);
    double own = 0.0;
    if (active) {
        const Rt64 Ti = load_rt(q.Rt, i);
        const double scale2 = 2.0 * (1.0 / (double)n_edges);
        double d[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) d[k] = 0.0;
        for (int s = 0; s < q.kn; ++s) {                       // own edges i -> j, slot order
            if (!SAS_IN(i * q.kn + s, n_edges, 1602)) break;
            const int j = q.nb[i * q.kn + s];
            if (j < 0 || j >= q.m) continue;
            const double gx = (double)q.nodes[3 * (long long)j], gy = (double)q.nodes[3 * (long long)j + 1], gz = (double)q.nodes[3 * (long long)j + 2];
            const Rt64 Tj = load_rt(q.Rt, j);
            double r[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = apply_row(Ti, a, gx, gy, gz) - apply_row(Tj, a, gx, gy, gz);
            own = own + ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double dr = scale2 * r[a];
                d[4 * a] = d[4 * a] + dr * gx;
                d[4 * a + 1] = d[4 * a + 1] + dr * gy;
                d[4 * a + 2] = d[4 * a + 2] + dr * gz;
                d[4 * a + 3] = d[4 * a + 3] + dr;
            }
        }
        if (q.kn > 0) {                                        // incoming edges k -> i, table order
            const double gx = (double)q.nodes[3 * i], gy = (double)q.nodes[3 * i + 1], gz = (double)q.nodes[3 * i + 2];
            long long lo = q.rev_start[i], hi = q.rev_start[i + 1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > n_edges ? n_edges : hi;
            for (long long p = lo; p < hi; ++p) {
                if (!SAS_IN(p, n_edges, 1603)) break;
                const int e = q.rev_edge[p];
                if (e < 0 || e >= n_edges) continue;
                const int k = e / q.kn;
                const Rt64 Tk = load_rt(q.Rt, k);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double dr = scale2 * (apply_row(Tk, a, gx, gy, gz) - apply_row(Ti, a, gx, gy, gz));
                    d[4 * a] = d[4 * a] - dr * gx;
                    d[4 * a + 1] = d[4 * a + 1] - dr * gy;
                    d[4 * a + 2] = d[4 * a + 2] - dr * gz;
                    d[4 * a + 3] = d[4 * a + 3] - dr;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) q.d_Rt[12 * i + k] = d[k];
    }
    const double total = tree_sum(red, tid, own);
    if (tid == 0 && SAS_IN(blockIdx.x, SAS_NODES_MAX_PARTIALS, 1604)) q.partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_nodes_value(const SasNodesRigidity q)
{
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int blocks = (q.m + kThreads - 1) / kThreads;
    double s = 0.0;
    for (int b = tid; b < blocks; b += kThreads) {
        if (!SAS_IN(b, SAS_NODES_MAX_PARTIALS, 1605)) break;
        s = s + q.partial[b];
    }
    const double total = tree_sum(red, tid, s);
    if (tid == 0) q.value[0] = q.kn > 0 ? total * (1.0 / ((double)q.m * q.kn)) : 0.0;
}

__global__ __launch_bounds__(kThreads) void k_nodes_twist_step(const SasNodesStep q)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= q.m || !SAS_IN(i, q.m, 1606)) return;
    const Rt64 T = load_rt(q.Rt, i);
    const double gx = (double)q.nodes[3 * i], gy = (double)q.nodes[3 * i + 1], gz = (double)q.nodes[3 * i + 2];
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = apply_row(T, a, gx, gy, gz);
    double G[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (q.d32 && q.d64) G[k] = (double)q.d32[12 * i + k] + q.weight * q.d64[12 * i + k];
        else if (q.d32) G[k] = (double)q.d32[12 * i + k];
        else G[k] = q.weight * q.d64[12 * i + k];
    }
    // the twist gradient about p: sum over the four columns c of A[:,c] x G[:,c], then G[:,3] x p
    double tw[6] = {0.0, 0.0, 0.0, G[3], G[7], G[11]};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double a0 = T.v[c], a1 = T.v[4 + c], a2 = T.v[8 + c], b0 = G[c], b1 = G[4 + c], b2 = G[8 + c];
        const double x = a1 * b2 - a2 * b1, y = a2 * b0 - a0 * b2, z = a0 * b1 - a1 * b0;
        tw[0] = c == 0 ? x : tw[0] + x;
        tw[1] = c == 0 ? y : tw[1] + y;
        tw[2] = c == 0 ? z : tw[2] + z;
    }
    tw[0] = tw[0] + (tw[4] * p[2] - tw[5] * p[1]);
    tw[1] = tw[1] + (tw[5] * p[0] - tw[3] * p[2]);
    tw[2] = tw[2] + (tw[3] * p[1] - tw[4] * p[0]);
    double xi[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double m1 = q.beta1 * q.m1[6 * i + k] + q.gain1 * tw[k];
        const double m2 = q.beta2 * q.m2[6 * i + k] + (q.gain2 * tw[k]) * tw[k];
        q.m1[6 * i + k] = m1;
        q.m2[6 * i + k] = m2;
        const double hat = (m1 / q.c1) / (sqrt(m2 / q.c2) + q.eps);
        xi[k] = -((k < 3 ? q.lr_rot : q.lr_trans) * hat);
    }
    // exp of the twist (omega, v): E_R = I + A W + B W^2, E_t = (I + B W + C W^2) v
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th = sqrt((wx * wx + wy * wy) + wz * wz);
    double A, B, C;
    if (th < 1e-8) {
        A = 1.0 - th * th / 6.0;
        B = 0.5 - th * th / 24.0;
        C = 1.0 / 6.0 - th * th / 120.0;
    } else {
        const double sn = sin(th), cs = cos(th);
        A = sn / th;
        B = (1.0 - cs) / (th * th);
        C = (th - sn) / ((th * th) * th);
    }
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double W2[9], ER[9], Et[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) W2[3 * a + b] = (W[3 * a] * W[b] + W[3 * a + 1] * W[3 + b]) + W[3 * a + 2] * W[6 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double V[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double id = a == b ? 1.0 : 0.0;
            ER[3 * a + b] = (id + A * W[3 * a + b]) + B * W2[3 * a + b];
            V[b] = (id + B * W[3 * a + b]) + C * W2[3 * a + b];
        }
        Et[a] = (V[0] * xi[3] + V[1] * xi[4]) + V[2] * xi[5];
    }
    // about the pivot: x -> E (x - p) + p
    const double u[3] = {T.v[3] - p[0], T.v[7] - p[1], T.v[11] - p[2]};
    double out[12];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) out[4 * a + b] = (ER[3 * a] * T.v[b] + ER[3 * a + 1] * T.v[4 + b]) + ER[3 * a + 2] * T.v[8 + b];
        out[4 * a + 3] = ((((ER[3 * a] * u[0] + ER[3 * a + 1] * u[1]) + ER[3 * a + 2] * u[2]) + Et[a]) + p[a]);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        q.Rt[12 * i + k] = out[k];
        q.Rt32[12 * i + k] = (float)out[k];
    }
}

DEV bool finite3(float x, float y, float z)
{
    const float big = 3.402823466e38f;
    return fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big;   // (false for NaN and for either infinity)
}

// One Jacobi rotation of the symmetric A about the pivot (P, Q), accumulated into the columns of V; node_fit_ref.jacobi's operations.
template <int P, int Q>
DEV void jacobi_turn(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q], app = A[P][P], aqq = A[Q][Q];
    const double theta = (aqq - app) / (2.0 * apq);
    const double sgn = theta >= 0.0 ? 1.0 : -1.0;
    double t = sgn / (fabs(theta) + sqrt(theta * theta + 1.0));   // (a theta that overflowed: t = 0 by itself)
    t = apq == 0.0 ? 0.0 : t;                                      // (an exactly zero pivot turns nothing)
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    A[P][P] = app - t * apq;
    A[Q][Q] = aqq + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        const double arp = A[r][P], arq = A[r][Q];
        A[r][P] = A[P][r] = c * arp - s * arq;
        A[r][Q] = A[Q][r] = s * arp + c * arq;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

__global__ __launch_bounds__(kThreads) void k_nodes_fit_rigid(const SasNodesFit q)
{
    const long long lanes = (long long)q.steps * q.m;
    const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (lane >= lanes || !SAS_IN(lane, lanes, 1607)) return;
    const long long i = lane % q.m, base = lane - i;   // base: the step's first row of `moved`
    const float *mv = q.moved + 3 * base;
    const float px = mv[3 * i], py = mv[3 * i + 1], pz = mv[3 * i + 2];
    double out[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (finite3(px, py, pz)) {
        const double gx = (double)q.nodes[3 * i], gy = (double)q.nodes[3 * i + 1], gz = (double)q.nodes[3 * i + 2];
        // the members: the node itself, then its table entries in slot order
        int member[SAS_NODES_MAX_K];
        double cnt = 1.0, ca[3] = {0.0 + gx, 0.0 + gy, 0.0 + gz}, cb[3] = {0.0 + (double)px, 0.0 + (double)py, 0.0 + (double)pz};   // (sums that begin at +0)
#pragma unroll
        for (int slot = 0; slot < SAS_NODES_MAX_K; ++slot) {
            int j = -1;
            if (slot < q.kn && SAS_IN(i * q.kn + slot, (long long)q.m * q.kn, 1608)) j = q.nb[i * q.kn + slot];
            bool on = j >= 0 && j < q.m && SAS_IN(base + j, lanes, 1609);
            const long long jj = on ? j : i;
            const float bx = mv[3 * jj], by = mv[3 * jj + 1], bz = mv[3 * jj + 2];
            on = on && finite3(bx, by, bz);
            member[slot] = on ? j : -1;
            cnt = cnt + (on ? 1.0 : 0.0);
            ca[0] = ca[0] + (on ? (double)q.nodes[3 * jj] : 0.0);
            ca[1] = ca[1] + (on ? (double)q.nodes[3 * jj + 1] : 0.0);
            ca[2] = ca[2] + (on ? (double)q.nodes[3 * jj + 2] : 0.0);
            cb[0] = cb[0] + (on ? (double)bx : 0.0);
            cb[1] = cb[1] + (on ? (double)by : 0.0);
            cb[2] = cb[2] + (on ? (double)bz : 0.0);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            ca[u] = ca[u] / cnt;
            cb[u] = cb[u] / cnt;
        }
        // S[u][v] = sum (a - ca)_u (b - cb)_v, in member order
        double S[3][3];
        {
            const double da[3] = {gx - ca[0], gy - ca[1], gz - ca[2]}, db[3] = {(double)px - cb[0], (double)py - cb[1], (double)pz - cb[2]};
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int v = 0; v < 3; ++v) S[u][v] = 0.0 + da[u] * db[v];
        }
#pragma unroll
        for (int slot = 0; slot < SAS_NODES_MAX_K; ++slot) {
            const bool on = member[slot] >= 0;
            const long long jj = on ? member[slot] : i;
            const double da[3] = {(double)q.nodes[3 * jj] - ca[0], (double)q.nodes[3 * jj + 1] - ca[1], (double)q.nodes[3 * jj + 2] - ca[2]};
            const double db[3] = {(double)mv[3 * jj] - cb[0], (double)mv[3 * jj + 1] - cb[1], (double)mv[3 * jj + 2] - cb[2]};
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int v = 0; v < 3; ++v) S[u][v] = S[u][v] + (on ? da[u] * db[v] : 0.0);
        }
        // Horn's matrix: its top eigenvector is the quaternion (w, x, y, z) of the best rotation
        double A[4][4], V[4][4];
        A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
        A[0][1] = S[1][2] - S[2][1];
        A[0][2] = S[2][0] - S[0][2];
        A[0][3] = S[0][1] - S[1][0];
        A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
        A[1][2] = S[0][1] + S[1][0];
        A[1][3] = S[2][0] + S[0][2];
        A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
        A[2][3] = S[1][2] + S[2][1];
        A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b < a) A[a][b] = A[b][a];
                V[a][b] = a == b ? 1.0 : 0.0;
            }
#pragma unroll 1
        for (int sweep = 0; sweep < SAS_NODES_FIT_SWEEPS; ++sweep) {
            jacobi_turn<0, 1>(A, V);
            jacobi_turn<0, 2>(A, V);
            jacobi_turn<0, 3>(A, V);
            jacobi_turn<1, 2>(A, V);
            jacobi_turn<1, 3>(A, V);
            jacobi_turn<2, 3>(A, V);
        }
        // (1,0,0,0) projected onto the span of the top eigenvectors
        const double l[4] = {A[0][0], A[1][1], A[2][2], A[3][3]};
        const double t01 = l[0] > l[1] ? l[0] : l[1], t23 = l[2] > l[3] ? l[2] : l[3];
        const double top = t01 > t23 ? t01 : t23;
        const double s01 = fabs(l[0]) > fabs(l[1]) ? fabs(l[0]) : fabs(l[1]), s23 = fabs(l[2]) > fabs(l[3]) ? fabs(l[2]) : fabs(l[3]);
        const double reach = SAS_NODES_FIT_GAP * (s01 > s23 ? s01 : s23);
        double qt[4] = {0.0, 0.0, 0.0, 0.0}, first[4] = {0.0, 0.0, 0.0, 0.0};
        bool taken = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double w = (top - l[k]) <= reach ? V[0][k] : 0.0;
            const bool pick = l[k] == top && !taken;
            taken = taken || pick;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                qt[r] = qt[r] + w * V[r][k];
                first[r] = pick ? V[r][k] : first[r];
            }
        }
        double n2 = ((qt[0] * qt[0] + qt[1] * qt[1]) + qt[2] * qt[2]) + qt[3] * qt[3];
        const bool half = n2 < SAS_NODES_FIT_HALF_TURN;
#pragma unroll
        for (int r = 0; r < 4; ++r) qt[r] = half ? first[r] : qt[r];
        n2 = ((qt[0] * qt[0] + qt[1] * qt[1]) + qt[2] * qt[2]) + qt[3] * qt[3];
        const double norm = sqrt(n2);
        const double w = qt[0] / norm, x = qt[1] / norm, y = qt[2] / norm, z = qt[3] / norm;
        out[0] = 1.0 - 2.0 * (y * y + z * z);
        out[1] = 2.0 * (x * y - w * z);
        out[2] = 2.0 * (x * z + w * y);
        out[4] = 2.0 * (x * y + w * z);
        out[5] = 1.0 - 2.0 * (x * x + z * z);
        out[6] = 2.0 * (y * z - w * x);
        out[8] = 2.0 * (x * z - w * y);
        out[9] = 2.0 * (y * z + w * x);
        out[10] = 1.0 - 2.0 * (x * x + y * y);
        const double p[3] = {(double)px, (double)py, (double)pz};
#pragma unroll
        for (int a = 0; a < 3; ++a) out[4 * a + 3] = p[a] - ((out[4 * a] * gx + out[4 * a + 1] * gy) + out[4 * a + 2] * gz);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (q.Rt64) q.Rt64[12 * lane + k] = out[k];
        q.Rt32[12 * lane + k] = (float)out[k];
    }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_nodes)

void sas_launch_nodes_rigidity(hipStream_t st, const SasNodesRigidity &q)
{
    const int blocks = (q.m + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_nodes_rigidity, dim3(blocks), dim3(kThreads), 0, st, q);
    hipLaunchKernelGGL(k_nodes_value, dim3(1), dim3(kThreads), 0, st, q);
}

void sas_launch_nodes_step(hipStream_t st, const SasNodesStep &q)
{
    const int blocks = (q.m + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_nodes_twist_step, dim3(blocks), dim3(kThreads), 0, st, q);
}

void sas_launch_nodes_fit(hipStream_t st, const SasNodesFit &q)
{
    const long long lanes = (long long)q.steps * q.m;
    hipLaunchKernelGGL(k_nodes_fit_rigid, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, q);
}
