// sas_fuse.hip -- TSDF fusion of depth frames into a caller-owned volume (sas_fuse_depth; DESIGN.md 3, "Depth fusion"): the consumer
// behind a label frame (sas_render_batch_labels) that turns depth, rgb8 and labels of C same-sized views into a signed-distance volume
// a surface can be extracted from.
//
//   k_fuse   one lane per voxel, flat index g = (k ny + j) nx + i along x: a wave reads and writes 256 contiguous bytes of tsdf and of
//            weight, and neighbouring lanes gather neighbouring pixels.  The lane reads its voxel once, walks the views in ascending
//            order with the voxel in registers, and writes it once -- only if some view updated it: a volume outside every frustum
//            costs one read.  The view's row {fx, fy, cx, cy, A|t} is indexed by the loop counter alone: wave-uniform loads.
// No LDS, no atomics, no wait between workgroups: a voxel's result depends on its own pixels only.
// Arithmetic: IEEE binary32, nothing fused (-ffp-contract=off, no fma_).
#include "sas_device.h"

namespace {

constexpr int kFuseThreads = SAS_FUSE_THREADS;

template <bool COLOR>
__global__ __launch_bounds__(kFuseThreads) void k_fuse(SasFuse q)
{
    const long long g = (long long)blockIdx.x * kFuseThreads + threadIdx.x;
    if (g >= q.n_vox) return;
    const int gi = (int)g;   // (n_vox <= 2^27)
    const int jk = gi / q.nx, i = gi - jk * q.nx, k = jk / q.ny, j = jk - k * q.ny;
    if (!SAS_IN(g, q.n_vox, 701) || !SAS_IN(k, q.nz, 702)) return;
    const float px = q.lo[0] + ((float)i + 0.5f) * q.voxel;
    const float py = q.lo[1] + ((float)j + 0.5f) * q.voxel;
    const float pz = q.lo[2] + ((float)k + 0.5f) * q.voxel;
    float tsdf = q.tsdf[g], w = q.weight[g];
    float col[3] = {0.0f, 0.0f, 0.0f};
    if (COLOR)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) col[ch] = q.color[3 * g + ch];
    const float Wf = (float)q.W, Hf = (float)q.H;
    bool updated = false, coloured = false;
    for (int c = 0; c < q.C; ++c) {
        if (!SAS_IN(c, q.n_rows, 703)) break;   // (uniform)
        const SasDepthView &V = q.view[c];
        const float qz = sas_affine_row<2>(V, px, py, pz);
        if (!(qz >= q.near_z)) continue;
        const float qx = sas_affine_row<0>(V, px, py, pz);
        const float qy = sas_affine_row<1>(V, px, py, pz);
        float uf = ((V.fx * (qx / qz)) + V.cx) - q.pixel_centre;
        float vf = ((V.fy * (qy / qz)) + V.cy) - q.pixel_centre;
        uf = uf + 0.5f;
        vf = vf + 0.5f;
        if (!(uf >= 0.0f && uf < Wf && vf >= 0.0f && vf < Hf)) continue;   // (a NaN fails; tested before the conversion)
        const int u = (int)floorf(uf), v = (int)floorf(vf);
        const long long p = ((long long)c * q.H + v) * q.W + u;
        if (!SAS_IN(u, q.W, 704) || !SAS_IN(v, q.H, 705) || !SAS_IN(p, q.n_pix, 706)) continue;
        const float d = q.depth[p];
        if (!(d > 0.0f && d < INFINITY)) continue;
        const float sdf = d - qz;
        const bool surface = !q.keep || q.keep[q.labels[p]] != 0;
        float val = 1.0f;
        if (surface) {
            if (sdf < -q.trunc) continue;
            val = fminf(1.0f, sdf / q.trunc);
        } else if (!(sdf >= q.trunc)) {
            continue;   // a carving pixel proves free space in front of itself only
        }
        const float w1 = w + 1.0f;
        tsdf = ((tsdf * w) + val) / w1;
        if (COLOR && surface) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) col[ch] = ((col[ch] * w) + (float)q.rgb8[3 * p + ch]) / w1;
            coloured = true;
        }
        w = fminf(w1, q.max_weight);
        updated = true;
    }
    if (!updated) return;
    q.tsdf[g] = tsdf;
    q.weight[g] = w;
    if (COLOR && coloured)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) q.color[3 * g + ch] = col[ch];
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_fuse)

void sas_launch_fuse(hipStream_t st, const SasFuse &q)
{
    if (q.n_vox <= 0 || q.C <= 0) return;
    const unsigned blocks = (unsigned)((q.n_vox + kFuseThreads - 1) / kFuseThreads);
    if (q.color) hipLaunchKernelGGL(k_fuse<true>, dim3(blocks), dim3(kFuseThreads), 0, st, q);
    else hipLaunchKernelGGL(k_fuse<false>, dim3(blocks), dim3(kFuseThreads), 0, st, q);
}
