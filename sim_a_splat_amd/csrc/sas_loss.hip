// sas_loss.hip -- the photometric loss of 3DGS training, (1 - lambda) L1 + lambda (1 - SSIM), and its gradient with respect to the frame
// (sas_photometric_loss; DESIGN.md 3, "Photometric loss"), hand-written for gfx950 (CDNA4, wave64).
//
//   k_loss_stats<true>   one 256-lane workgroup per 16x16 pixel tile, one channel at a time: the 26x26 halo of the frame x and the target y
//                        goes to LDS (zeros outside the image), the five windowed sums g*x, g*y, g*x^2, g*y^2, g*xy are taken separably
//                        (rows into LDS, then columns), the lane forms its pixel's SSIM and the three partials d/dmu_x, d/dsigma_x^2,
//                        d/dsigma_xy (times the mask) and stores them as planes for the second stencil.  The lane's w |x - y|, w ssim,
//                        w (x - y)^2 and w are summed over the workgroup in a fixed tree: one partial row per workgroup.
//   k_loss_tail          ONE workgroup adds the partial rows in a fixed order (lane t takes rows t, t + 256, ... in index order, in double;
//                        then a fixed tree) and writes terms = (loss, l1, ssim, mse) and D = max(3 sum w, 1) for the gradient kernel:
//                        nobody waits for the host.
//   k_loss_grad<true>    same tiling: the halo of the three partial planes, three separable sums, composed with x, y and the L1 term,
//                        divided by D, gated where the frame's clamp binds, 12 contiguous bytes per pixel as sas_render_backward reads.
//   <false>              lambda == 0: no stencil, no planes, no LDS but the reduction's.
// No atomics anywhere: the same inputs give the same bits.  A lane outside the image computes on zeros and stores nothing.
// LDS: halo rows have a stride of 48 floats -- the four 16-lane rows of a wave then fall into four disjoint 16-bank groups for every
// window offset; the row sums are [26][16], read down the columns as 64 consecutive floats per wave.
// Arithmetic: IEEE binary32, nothing fused, correctly rounded /; a windowed sum is w[0] v[0], then + w[k] v[k] for k = 1 .. 10.
#include "sas_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 16, kRad = 5, kWin = 2 * kRad + 1, kHalo = kTile + 2 * kRad, kStride = 48;
constexpr int kHaloFloats = kHalo * kStride, kRowFloats = kHalo * kTile;
constexpr float kC1 = 0.0001f, kC2 = 0.0009f;

DEV float sign_of(float d) { return d != d ? d : (float)(d > 0.0f) - (float)(d < 0.0f); }

// the workgroup's sum of v over its 256 lanes, a fixed tree (lane t += lane t + s, s = 128 .. 1); valid in lane 0
DEV float tree_sum(float *red, int tid, float v)
{
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// plane[(oy + r) W + ox + c] of the 26x26 halo into dst (stride kStride), zeros outside the image
DEV void stage_halo(const SasLoss &q, const float *plane, long long stride, long long limit, int ox, int oy, int tid, float *dst, int code)
{
    for (int i = tid; i < kHalo * kHalo; i += 256) {
        const int r = i / kHalo, c = i - r * kHalo;
        const int px = ox + c, py = oy + r;
        float v = 0.0f;
        if (px >= 0 && px < q.W && py >= 0 && py < q.H) {
            const long long at = ((long long)py * q.W + px) * stride;
            if (SAS_IN(at, limit, code)) v = plane[at];
        }
        dst[r * kStride + c] = v;
    }
}

template <bool SSIM>
__global__ __launch_bounds__(256) void k_loss_stats(const SasLoss q)
{
    __shared__ float sx[SSIM ? kHaloFloats : 1], sy[SSIM ? kHaloFloats : 1], h[SSIM ? 5 * kRowFloats : 1], red[256];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int px = blockIdx.x * kTile + tx, py = blockIdx.y * kTile + ty;
    const bool in = px < q.W && py < q.H;
    const long long n_pix = (long long)q.W * q.H, p = (long long)py * q.W + px;
    float w = 0.0f;
    if (in && SAS_IN(p, n_pix, 931)) w = q.mask ? (q.mask[p] != 0 ? 1.0f : 0.0f) : 1.0f;
    float s_l1 = 0.0f, s_ss = 0.0f, s_l2 = 0.0f;
    for (int c = 0; c < 3; ++c) {
        float x = 0.0f, y = 0.0f;
        if (in && SAS_IN(3 * p + c, 3 * n_pix, 932)) { x = q.x[3 * p + c]; y = q.y[3 * p + c]; }
        const float d = x - y;
        s_l1 = s_l1 + w * fabsf(d);
        s_l2 = s_l2 + w * (d * d);
        if (!SSIM) continue;
        stage_halo(q, q.x + c, 3, 3 * n_pix - c, blockIdx.x * kTile - kRad, blockIdx.y * kTile - kRad, tid, sx, 933);
        stage_halo(q, q.y + c, 3, 3 * n_pix - c, blockIdx.x * kTile - kRad, blockIdx.y * kTile - kRad, tid, sy, 934);
        __syncthreads();
        for (int i = tid; i < kRowFloats; i += 256) {   // rows: 26 x 16 sums of each of the five
            const int r = i >> 4, j = i & 15;
            const float *rx = sx + r * kStride + j, *ry = sy + r * kStride + j;
            float a[5];
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float u = rx[k], v = ry[k], g = q.win[k];
                const float t[5] = {g * u, g * v, g * (u * u), g * (v * v), g * (u * v)};
#pragma unroll
                for (int m = 0; m < 5; ++m) a[m] = k == 0 ? t[m] : a[m] + t[m];
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) h[m * kRowFloats + i] = a[m];
        }
        __syncthreads();
        float a[5];
#pragma unroll
        for (int k = 0; k < kWin; ++k) {               // columns
            const float g = q.win[k];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const float t = g * h[m * kRowFloats + (ty + k) * kTile + tx];
                a[m] = k == 0 ? t : a[m] + t;
            }
        }
        const float mx = a[0], my = a[1];
        const float mx2 = mx * mx, my2 = my * my, mxy = mx * my;
        const float vx = a[2] - mx2, vy = a[3] - my2, cxy = a[4] - mxy;
        const float A1 = 2.0f * mxy + kC1, A2 = 2.0f * cxy + kC2, B1 = (mx2 + my2) + kC1, B2 = (vx + vy) + kC2;
        const float den = B1 * B2, ssim = (A1 * A2) / den;
        s_ss = s_ss + w * ssim;
        if (q.maps && in) {
            const float d_vx = -(ssim / B2), d_cxy = (2.0f * A1) / den;
            const float t = my * B1 - A1 * mx;
            const float d_mu = (((2.0f * t) * A2) / (B1 * den) - (2.0f * mx) * d_vx) - my * d_cxy;
            const long long at = (long long)c * n_pix + p, plane = 3 * n_pix;
            if (SAS_IN(at + 2 * plane, 9 * n_pix, 935)) {
                q.maps[at] = w * d_mu;
                q.maps[at + plane] = w * d_vx;
                q.maps[at + 2 * plane] = w * d_cxy;
            }
        }
        // (no barrier here: the next channel's staging overwrites sx / sy, which nothing reads behind the row pass's barrier, and its
        // row pass writes h only behind the barrier after staging, which every lane reaches after these column reads)
    }
    const float t_l1 = tree_sum(red, tid, s_l1), t_ss = SSIM ? tree_sum(red, tid, s_ss) : 0.0f, t_l2 = tree_sum(red, tid, s_l2),
                t_w = tree_sum(red, tid, w);
    if (tid == 0) {
        const long long b = (long long)blockIdx.y * q.tiles_x + blockIdx.x;
        if (SAS_IN(4 * b + 3, 4ll * q.tiles_x * q.tiles_y, 936)) {
            q.partial[4 * b + 0] = t_l1;
            q.partial[4 * b + 1] = t_ss;
            q.partial[4 * b + 2] = t_l2;
            q.partial[4 * b + 3] = t_w;
        }
    }
}

__global__ __launch_bounds__(256) void k_loss_tail(const SasLoss q)
{
    __shared__ double red[4][256];
    const int tid = threadIdx.x;
    const long long rows = (long long)q.tiles_x * q.tiles_y;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long b = tid; b < rows; b += 256) {
        if (!SAS_IN(4 * b + 3, 4 * rows, 937)) break;
#pragma unroll
        for (int m = 0; m < 4; ++m) s[m] = s[m] + (double)q.partial[4 * b + m];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) red[m][tid] = s[m];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int m = 0; m < 4; ++m) red[m][tid] = red[m][tid] + red[m][tid + st];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const float D = fmaxf(3.0f * (float)red[3][0], 1.0f);
    const float l1 = (float)red[0][0] / D, mse = (float)red[2][0] / D;
    if (q.lambda == 0.0f) {
        q.terms[0] = l1; q.terms[1] = l1; q.terms[2] = NAN; q.terms[3] = mse;
    } else {
        const float ssim = (float)red[1][0] / D;
        q.terms[0] = (1.0f - q.lambda) * l1 + q.lambda * (1.0f - ssim);
        q.terms[1] = l1; q.terms[2] = ssim; q.terms[3] = mse;
    }
    q.norm[0] = D;
}

template <bool SSIM>
__global__ __launch_bounds__(256) void k_loss_grad(const SasLoss q)
{
    __shared__ float sm[SSIM ? 3 * kHaloFloats : 1], h[SSIM ? 3 * kRowFloats : 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int px = blockIdx.x * kTile + tx, py = blockIdx.y * kTile + ty;
    const bool in = px < q.W && py < q.H;
    const long long n_pix = (long long)q.W * q.H, p = (long long)py * q.W + px;
    const float D = q.norm[0], oml = 1.0f - q.lambda;
    float w = 0.0f;
    if (in && SAS_IN(p, n_pix, 941)) w = q.mask ? (q.mask[p] != 0 ? 1.0f : 0.0f) : 1.0f;
    float g[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < 3; ++c) {
        float x = 0.0f, y = 0.0f;
        if (in && SAS_IN(3 * p + c, 3 * n_pix, 942)) { x = q.x[3 * p + c]; y = q.y[3 * p + c]; }
        float v = ((oml * w) * sign_of(x - y)) / D;
        if (SSIM) {
            // (no barrier in front: the row pass below writes h only behind the barrier after staging, which every lane reaches after
            // its column pass of the channel before)
#pragma unroll
            for (int m = 0; m < 3; ++m)
                stage_halo(q, q.maps + (long long)(3 * m + c) * n_pix, 1, n_pix, blockIdx.x * kTile - kRad, blockIdx.y * kTile - kRad, tid,
                           sm + m * kHaloFloats, 943 + m);
            __syncthreads();
            for (int i = tid; i < kRowFloats; i += 256) {
                const int r = i >> 4, j = i & 15;
                const float *row = sm + r * kStride + j;
                float a[3];
#pragma unroll
                for (int k = 0; k < kWin; ++k) {
                    const float gk = q.win[k];
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        const float t = gk * row[m * kHaloFloats + k];
                        a[m] = k == 0 ? t : a[m] + t;
                    }
                }
#pragma unroll
                for (int m = 0; m < 3; ++m) h[m * kRowFloats + i] = a[m];
            }
            __syncthreads();
            float a[3];
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float gk = q.win[k];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const float t = gk * h[m * kRowFloats + (ty + k) * kTile + tx];
                    a[m] = k == 0 ? t : a[m] + t;
                }
            }
            const float gs = (a[0] + (2.0f * x) * a[1]) + y * a[2];
            v = v - (q.lambda * gs) / D;
        }
        g[c] = (q.gate && !(x < 1.0f)) ? 0.0f : v;
    }
    if (!in) return;
    if (q.g_rgb && SAS_IN(3 * p + 2, 3 * n_pix, 946)) {
        q.g_rgb[3 * p + 0] = g[0];
        q.g_rgb[3 * p + 1] = g[1];
        q.g_rgb[3 * p + 2] = g[2];
    }
    if (q.g_alpha && SAS_IN(p, n_pix, 947)) q.g_alpha[p] = 0.0f - ((g[0] * q.bg[0] + g[1] * q.bg[1]) + g[2] * q.bg[2]);
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_loss)

void sas_launch_loss(hipStream_t st, const SasLoss &q)
{
    const dim3 grid((unsigned)q.tiles_x, (unsigned)q.tiles_y), block(256);
    const bool ssim = q.lambda != 0.0f, grad = q.g_rgb || q.g_alpha;
    if (ssim)
        hipLaunchKernelGGL(k_loss_stats<true>, grid, block, 0, st, q);
    else
        hipLaunchKernelGGL(k_loss_stats<false>, grid, block, 0, st, q);
    hipLaunchKernelGGL(k_loss_tail, dim3(1), block, 0, st, q);
    if (!grad) return;
    if (ssim)
        hipLaunchKernelGGL(k_loss_grad<true>, grid, block, 0, st, q);
    else
        hipLaunchKernelGGL(k_loss_grad<false>, grid, block, 0, st, q);
}
