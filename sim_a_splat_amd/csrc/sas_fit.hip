// sas_fit.hip -- the optimiser step on the resident scene (sas_scene_adam_step; DESIGN.md 3, "Optimiser step") and the scene's way back to
// the caller (sas_scene_read), hand-written for gfx950 (CDNA4, wave64).
//
//   k_adam_scene    one lane per storage slot, 256 per workgroup, ONE launch for every variable group that is stepped: the lane gathers
//                   its Gaussian's gradients at perm[slot] (the caller's order, AoS, as sas_render_backward writes them), chains them
//                   through the activations, advances Adam on the moments kept in slot order, and writes the new values back into the
//                   planes k_relayout laid out.  A pure HBM stream: 16-byte plane and state accesses, one contiguous 1 KiB per wave
//                   instruction; the state is read and written once (non-temporal), the gathered gradients are loaded plainly (a lane comes back
//                   to its cache lines) and the planes are stored plainly -- the next frame's projection reads them.  Never written: g2.w (the group bits), the zero padding of the last colour plane, the lanes
//                   n .. n_pad of any plane.
//   k_adam_init     the raw values log(scale) and logit(opacity) of a group that is stepped for the first time, from the resident
//                   values (raw_scale, raw_opacity); NaN marks a value outside the domain of its inverse activation: that variable stays fixed.
//   k_scene_gather  the inverse of k_relayout: planes -> the caller's AoS arrays through perm.
// No LDS, no atomics, no wait between workgroups: a Gaussian's step depends on its own slot only.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_); correctly rounded / and sqrt, libm expf / logf.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

DEV void nt_store(float4 *p, const float4 v)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4 *>(p));
}

// One element's Adam step on the raw variable x with gradient g.  A non-finite g leaves m, v and x as they are (false).
DEV bool adam_elem(const SasAdam &A, float g, float lr, float &m, float &v, float &x)
{
    if (!(fabsf(g) < INFINITY)) return false;   // (a NaN fails too)
    m = A.beta1 * m + A.omb1 * g;
    v = A.beta2 * v + A.omb2 * (g * g);
    const float mh = m / A.bc1, vh = v / A.bc2;
    x = x - (lr * mh) / (sqrtf(vh) + A.eps);
    return true;
}

// floats [4p, 4p + 4) of a Gaussian's coefficient gradient, zero beyond coeff_floats
DEV void load_sh_grad(const SasAdam &A, const float *gs, int base, int cnt, float *g)
{
    if (A.sh_aligned) {   // coeff_floats a multiple of 4 and a 16-byte aligned array: cnt == 4
        // (a plain load: the lane's next three loads fall into the same 128-byte lines.  Non-temporal here cost 11 % of the step at a
        // million Gaussians: profiles/scene_fit.txt)
        const float4 G = *reinterpret_cast<const float4 *>(gs + base);
        g[0] = G.x; g[1] = G.y; g[2] = G.z; g[3] = G.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = k < cnt ? gs[base + k] : 0.0f;
    }
}

constexpr int kBatch = 4;   // colour planes k_adam_scene has in flight per lane

__global__ __launch_bounds__(256) void k_adam_scene(const SasAdam A)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;   // slot
    if (j >= A.n) return;
    const long long i = A.perm[j];                                   // caller's index
    if (!SAS_IN(j, A.n_pad, 901) || !SAS_IN(i, A.n, 902)) return;
    const float *gs = A.d_sh ? A.d_sh + (long long)A.coeff_floats * i : nullptr;
    // the colour planes that hold a stepped coefficient: the DC triple lives in plane 0
    const int sh_planes = A.d_sh ? (A.lr_sh_rest != 0.0f ? A.planes : 1) : 0;

    if (A.visible_only) {   // a Gaussian whose gradient is an exact zero in every stepped array is skipped whole
        bool any = false;
        if (A.d_means) any = any || A.d_means[3 * i] != 0.0f || A.d_means[3 * i + 1] != 0.0f || A.d_means[3 * i + 2] != 0.0f;
        if (A.d_opac) any = any || A.d_opac[i] != 0.0f;
        if (A.d_quats) any = any || A.d_quats[4 * i] != 0.0f || A.d_quats[4 * i + 1] != 0.0f || A.d_quats[4 * i + 2] != 0.0f || A.d_quats[4 * i + 3] != 0.0f;
        if (A.d_scales) any = any || A.d_scales[3 * i] != 0.0f || A.d_scales[3 * i + 1] != 0.0f || A.d_scales[3 * i + 2] != 0.0f;
        if (gs)
            for (int e = 0; e < A.coeff_floats; ++e) any = any || gs[e] != 0.0f;
        if (!any) return;
    }

    if (A.d_means || A.d_opac) {   // g0 = (mean, opacity)
        float4 P = A.g0[j];
        if (A.d_means) {
            float4 M = nt_load(A.s.means_m + j), V = nt_load(A.s.means_v + j);
            adam_elem(A, A.d_means[3 * i + 0], A.lr_means, M.x, V.x, P.x);
            adam_elem(A, A.d_means[3 * i + 1], A.lr_means, M.y, V.y, P.y);
            adam_elem(A, A.d_means[3 * i + 2], A.lr_means, M.z, V.z, P.z);
            nt_store(A.s.means_m + j, M);
            nt_store(A.s.means_v + j, V);
        }
        if (A.d_opac) {
            float4 S = nt_load(A.s.opac + j);   // (m, v, logit, -)
            if (S.z == S.z) {                 // (NaN: the resident opacity was outside (0, 1) -- fixed)
                const float g = A.d_opac[i] * (P.w * (1.0f - P.w));
                if (adam_elem(A, g, A.lr_opac, S.x, S.y, S.z)) {
                    P.w = 1.0f / (1.0f + expf(-S.z));
                    nt_store(A.s.opac + j, S);
                }
            }
        }
        A.g0[j] = P;
    }
    if (A.d_quats) {   // g1 = the quaternion as uploaded
        float4 Q = A.g1[j], M = nt_load(A.s.quats_m + j), V = nt_load(A.s.quats_v + j);
        adam_elem(A, A.d_quats[4 * i + 0], A.lr_quats, M.x, V.x, Q.x);
        adam_elem(A, A.d_quats[4 * i + 1], A.lr_quats, M.y, V.y, Q.y);
        adam_elem(A, A.d_quats[4 * i + 2], A.lr_quats, M.z, V.z, Q.z);
        adam_elem(A, A.d_quats[4 * i + 3], A.lr_quats, M.w, V.w, Q.w);
        nt_store(A.s.quats_m + j, M);
        nt_store(A.s.quats_v + j, V);
        A.g1[j] = Q;
    }
    if (A.d_scales) {   // g2 = (scale, group bits): the bits are neither changed nor stored
        const float4 G = A.g2[j];
        const float4 M = nt_load(A.s.scales_m + j), V = nt_load(A.s.scales_v + j), R = nt_load(A.s.scales_raw + j);
        float s[3] = {G.x, G.y, G.z}, m[3] = {M.x, M.y, M.z}, v[3] = {V.x, V.y, V.z}, raw[3] = {R.x, R.y, R.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(raw[k] == raw[k])) continue;   // (NaN: the resident scale was not a positive finite number -- fixed)
            const float g = A.d_scales[3 * i + k] * s[k];
            if (adam_elem(A, g, A.lr_scales, m[k], v[k], raw[k])) s[k] = expf(raw[k]);
        }
        nt_store(A.s.scales_m + j, make_float4(m[0], m[1], m[2], M.w));
        nt_store(A.s.scales_v + j, make_float4(v[0], v[1], v[2], V.w));
        nt_store(A.s.scales_raw + j, make_float4(raw[0], raw[1], raw[2], R.w));
        float *dst = reinterpret_cast<float *>(A.g2 + j);
        dst[0] = s[0]; dst[1] = s[1]; dst[2] = s[2];
    }
    // col = the SH planes (or the plain colour), kBatch planes at a time: their twelve plane loads and the gradients are issued before
    // the first is used (stores in between would fence them: nothing tells the compiler that the state and the planes do not alias)
    for (int p0 = 0; p0 < sh_planes; p0 += kBatch) {
        float4 C[kBatch], M[kBatch], V[kBatch];
        float g[kBatch][4];
        bool live[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int p = p0 + b, base = 4 * p;
            const int cnt = A.coeff_floats - base < 4 ? A.coeff_floats - base : 4;
            const long long o = (long long)p * A.n_pad + j;
            live[b] = p < sh_planes && SAS_IN(o, (long long)A.planes * A.n_pad, 903) && SAS_IN(base + cnt - 1, A.coeff_floats, 904);
            if (!live[b]) continue;
            C[b] = A.col[o];
            M[b] = nt_load(A.s.sh_m + o);
            V[b] = nt_load(A.s.sh_v + o);
            load_sh_grad(A, gs, base, cnt, g[b]);
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            if (!live[b]) continue;
            const int p = p0 + b, base = 4 * p;
            const int cnt = A.coeff_floats - base < 4 ? A.coeff_floats - base : 4;
            const long long o = (long long)p * A.n_pad + j;
            float c[4] = {C[b].x, C[b].y, C[b].z, C[b].w}, m[4] = {M[b].x, M[b].y, M[b].z, M[b].w}, v[4] = {V[b].x, V[b].y, V[b].z, V[b].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lr = base + k < 3 ? A.lr_sh_dc : A.lr_sh_rest;
                if (k < cnt && lr != 0.0f) adam_elem(A, g[b][k], lr, m[k], v[k], c[k]);
            }
            nt_store(A.s.sh_m + o, make_float4(m[0], m[1], m[2], m[3]));
            nt_store(A.s.sh_v + o, make_float4(v[0], v[1], v[2], v[3]));
            if (cnt == 4) {
                A.col[o] = make_float4(c[0], c[1], c[2], c[3]);
            } else {   // the last plane of a block that is no multiple of four floats: its zero padding is not stored
                float *dst = reinterpret_cast<float *>(A.col + o);
                for (int k = 0; k < cnt; ++k) dst[k] = c[k];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_adam_init(long long n, const float4 *g0, const float4 *g2, float4 *opac, float4 *scales_raw)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (opac) {
        const float o = g0[j].w;
        opac[j] = make_float4(0.0f, 0.0f, raw_opacity(o), 0.0f);
    }
    if (scales_raw) {
        const float4 G = g2[j];
        scales_raw[j] = make_float4(raw_scale(G.x), raw_scale(G.y), raw_scale(G.z), 0.0f);
    }
}

__global__ __launch_bounds__(256) void k_scene_gather(const SasGather Q)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;   // slot
    if (j >= Q.n) return;
    const long long i = Q.perm[j];                                   // caller's index
    if (!SAS_IN(j, Q.n_pad, 911) || !SAS_IN(i, Q.n, 912)) return;
    const float4 P = Q.g0[j];
    if (Q.means) { Q.means[3 * i] = P.x; Q.means[3 * i + 1] = P.y; Q.means[3 * i + 2] = P.z; }
    if (Q.opac) Q.opac[i] = P.w;
    if (Q.quats || Q.scales || Q.cov6) {
        const float4 A = Q.g1[j], B = Q.g2[j];
        if (Q.quats) { Q.quats[4 * i] = A.x; Q.quats[4 * i + 1] = A.y; Q.quats[4 * i + 2] = A.z; Q.quats[4 * i + 3] = A.w; }
        if (Q.scales) { Q.scales[3 * i] = B.x; Q.scales[3 * i + 1] = B.y; Q.scales[3 * i + 2] = B.z; }
        if (Q.cov6) {
            float *c = Q.cov6 + 6 * i;
            c[0] = A.x; c[1] = A.y; c[2] = A.z; c[3] = A.w; c[4] = B.x; c[5] = B.y;
        }
    }
    if (Q.colors) {
        float *dst = Q.colors + (long long)Q.coeff_floats * i;
        for (int p = 0; p < Q.planes; ++p) {
            const float4 C = Q.col[(long long)p * Q.n_pad + j];
            const float c[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * p + k < Q.coeff_floats) dst[4 * p + k] = c[k];
        }
    }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_fit)

void sas_launch_adam_init(hipStream_t st, int64_t n, const float4 *g0, const float4 *g2, const SasAdamState &fresh)
{
    if (n <= 0 || (!fresh.opac && !fresh.scales_raw)) return;
    hipLaunchKernelGGL(k_adam_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, g0, g2, fresh.opac, fresh.scales_raw);
}

void sas_launch_adam_scene(hipStream_t st, const SasAdam &a)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_adam_scene, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
}

void sas_launch_scene_gather(hipStream_t st, const SasGather &q)
{
    if (q.n <= 0) return;
    hipLaunchKernelGGL(k_scene_gather, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, st, q);
}
