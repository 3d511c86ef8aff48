// sas_mesh.hip -- triangle meshes of a frame (sas_scene_meshes; DESIGN.md 3, "Meshes"): setup, binning.
// The per-pixel resolution and the occlusion of the splats are k_blend_mesh's (sas_tile.hip).
#include "sas_device.h"

namespace {

constexpr int kMeshSetupThreads = 256;
constexpr int kMeshScanThreads = 1024;

struct Vc { double x, y, z; };   // a camera-frame vertex
constexpr double kMeshCullMargin = 1.0 / 64.0;   // px: far above the float32 edge error it has to cover (mesh_record)

// Screen-space record of one clipped triangle (camera-frame vertices, z >= kNear).  false: degenerate or off screen.
DEV bool mesh_record(const SasCam &c, const Vc *q, float4 *rec, int4 &rect)
{
    double u[3], v[3], w[3];
    for (int k = 0; k < 3; ++k) {
        w[k] = 1.0 / q[k].z;
        u[k] = (double)c.fx * q[k].x * w[k] + (double)c.cx;
        v[k] = (double)c.fy * q[k].y * w[k] + (double)c.cy;
    }
    double area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0]);
    if (!(fabs(area) > 0.0) || !isfinite(area)) return false;
    if (area < 0.0) {   // counter-clockwise in (u, v): inside is E > 0 on every edge
        double t;
        t = u[1]; u[1] = u[2]; u[2] = t;
        t = v[1]; v[1] = v[2]; v[2] = t;
        t = w[1]; w[1] = w[2]; w[2] = t;
        area = -area;
    }
    double umin = fmin(u[0], fmin(u[1], u[2])), umax = fmax(u[0], fmax(u[1], u[2]));
    double vmin = fmin(v[0], fmin(v[1], v[2])), vmax = fmax(v[0], fmax(v[1], v[2]));
    // pixel centres x + 0.5 in [umin, umax]
    if (umax < 0.5 || vmax < 0.5 || umin > (double)c.W - 0.5 || vmin > (double)c.H - 0.5) return false;
    // Planes in the frame of the image centre (xo, yo), edges normalised: E is the signed distance in pixels, and c the distance
    // of the centre from the edge's line -- small for every edge that passes the image, however far its ends project (a
    // triangle clipped at the near plane of a wrist camera), so float32 keeps E's error far below 1e-3 px on screen.
    const double xo = 0.5 * (double)c.W, yo = 0.5 * (double)c.H;
    float e[9];
    double elen[3];
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3;
        const double a0 = v[i] - v[j], b0 = u[j] - u[i];
        const double len = sqrt(a0 * a0 + b0 * b0);
        if (!(len > 0.0)) return false;
        elen[i] = len;
        const double a = a0 / len, b = b0 / len;
        // c from the edge's lexicographically smaller end: the same edge walked the other way (a neighbour) gets exactly -a, -b, -c,
        // so E is exactly negated and the tie rule gives a shared edge's pixel centre to one of the two
        const bool ifirst = u[i] < u[j] || (u[i] == u[j] && v[i] < v[j]);
        const double ue = ifirst ? u[i] : u[j], ve = ifirst ? v[i] : v[j];
        e[3 * i + 0] = (float)a;
        e[3 * i + 1] = (float)b;
        e[3 * i + 2] = (float)(-(a * (ue - xo) + b * (ve - yo)));
    }
    // A record that can hold NO pixel centre is dropped here (most triangles of a tessellated robot link are smaller than a pixel, and a
    // tile's list ran to thousands of them).  mesh_resolve's float32 E_i differs from the true signed distance by at most eps =
    // 2^-21 S_i at any pixel of the frame, S_i = |a| W/2 + |b| H/2 + |c| (three coefficients rounded to float32, two products, two
    // sums: below 8 * 2^-24 of the terms' magnitudes), so a centre it accepts has E_i >= -eps on all three edges: it lies in the
    // triangle grown by eps on every edge, the image of the triangle under the homothety about its incentre with ratio (r + eps) / r,
    // r = area / s the inradius -- within eps L / r of the triangle, L the longest edge (no vertex is farther from the incentre).  When
    // that distance is at most kMeshCullMargin and the bounding box widened by the margin holds no centre, no pixel can pass the test:
    // the record wins nowhere, and the minimum of keys over the others is what it was.  Slivers (eps L / r above the margin) are kept.
    {
        double smax = 0.0, lmax = 0.0;
        for (int i = 0; i < 3; ++i) {
            smax = fmax(smax, fabs((double)e[3 * i]) * xo + fabs((double)e[3 * i + 1]) * yo + fabs((double)e[3 * i + 2]));
            lmax = fmax(lmax, elen[i]);
        }
        const double eps = smax * (1.0 / 2097152.0);
        const double reach = eps * lmax * (elen[0] + elen[1] + elen[2]) / area;   // eps L / r, r = (area / 2) / ((l0 + l1 + l2) / 2)
        if (reach <= kMeshCullMargin) {
            const bool none_x = floor(umax + kMeshCullMargin - 0.5) < ceil(umin - kMeshCullMargin - 0.5);
            const bool none_y = floor(vmax + kMeshCullMargin - 0.5) < ceil(vmin - kMeshCullMargin - 0.5);
            if (none_x || none_y) return false;
        }
    }
    // 1/z = za (x - xo) + zb (y - yo) + zc through the three vertices (zc: 1/z at the image centre)
    const double za = ((w[1] - w[0]) * (v[2] - v[0]) - (w[2] - w[0]) * (v[1] - v[0])) / area;
    const double zb = ((u[1] - u[0]) * (w[2] - w[0]) - (u[2] - u[0]) * (w[1] - w[0])) / area;
    const double zc = w[0] + za * (xo - u[0]) + zb * (yo - v[0]);
    rec[0] = make_float4(e[0], e[1], e[2], e[3]);
    rec[1] = make_float4(e[4], e[5], e[6], e[7]);
    rec[2] = make_float4(e[8], (float)za, (float)zb, (float)zc);
    // tiles whose pixel centres the rectangle can hold
    const double lo_x = fmax(umin - 0.5, 0.0), hi_x = fmin(umax - 0.5, (double)c.W - 1.0);
    const double lo_y = fmax(vmin - 0.5, 0.0), hi_y = fmin(vmax - 0.5, (double)c.H - 1.0);
    rect = make_int4((int)floor(lo_x) / SAS_TILE, (int)floor(lo_y) / SAS_TILE, (int)ceil(hi_x) / SAS_TILE, (int)ceil(hi_y) / SAS_TILE);
    rect.z = min(rect.z, c.tw - 1);
    rect.w = min(rect.w, c.th - 1);
    return rect.x <= rect.z && rect.y <= rect.w;
}

// Attribute planes of a smooth triangle's record (rule 2b): per channel, shade / z is affine in the pixel, through the record's three
// corners (u, v, at / z) -- the plane of the unclipped triangle, whichever of its records this is.  Same frame and rounding as za, zb, zc.
DEV void mesh_planes(const SasCam &c, const Vc *q, const double (*at)[3], float4 *pl)
{
    double u[3], v[3], w[3];
    for (int k = 0; k < 3; ++k) {
        w[k] = 1.0 / q[k].z;
        u[k] = (double)c.fx * q[k].x * w[k] + (double)c.cx;
        v[k] = (double)c.fy * q[k].y * w[k] + (double)c.cy;
    }
    const double area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0]);   // (mesh_record has accepted it: not zero)
    const double xo = 0.5 * (double)c.W, yo = 0.5 * (double)c.H;
    float abc[3][3];
    for (int ch = 0; ch < 3; ++ch) {
        const double p0 = at[0][ch] * w[0], p1 = at[1][ch] * w[1], p2 = at[2][ch] * w[2];
        const double A = ((p1 - p0) * (v[2] - v[0]) - (p2 - p0) * (v[1] - v[0])) / area;
        const double B = ((u[1] - u[0]) * (p2 - p0) - (u[2] - u[0]) * (p1 - p0)) / area;
        abc[ch][0] = (float)A;
        abc[ch][1] = (float)B;
        abc[ch][2] = (float)(p0 + A * (xo - u[0]) + B * (yo - v[0]));
    }
    pl[0] = make_float4(abc[0][0], abc[0][1], abc[0][2], 1.0f);
    pl[1] = make_float4(abc[1][0], abc[1][1], abc[1][2], 0.0f);
    pl[2] = make_float4(abc[2][0], abc[2][1], abc[2][2], 0.0f);
}

// One thread per triangle: group pose and view (float, as the projection moves the Gaussians), shading, near clip, records
// 2 t and 2 t + 1, per-tile counts.  planes (a frame whose meshes carry vertex attributes, else nullptr): the records' attribute
// planes -- three vertex shades interpolated over a smooth triangle, the smooth flag zero on a flat one.
__global__ __launch_bounds__(kMeshSetupThreads) void k_mesh_setup(SasMeshScene m, SasParams P, SasFrame f, SasMeshFrame mf, float4 *planes)
{
    const int t = blockIdx.x * kMeshSetupThreads + threadIdx.x;
    if (t >= m.nt) return;
    const SasCam &c = P.cam;
    int4 none = make_int4(1, 0, 0, 0);
    mf.rect[2 * t] = none;
    mf.rect[2 * t + 1] = none;
    const int4 tr = m.tri[t];
    const int g = tr.w;
    const float *G = (f.group_Rt && g >= 0 && g < m.n_groups) ? f.group_Rt + 12 * g : nullptr;
    float wv[3][3];
    Vc q[3];
    bool ok = true;
    const int ids[3] = {tr.x, tr.y, tr.z};
    for (int k = 0; k < 3; ++k) {
        if (!SAS_IN(ids[k], m.nv, 301)) return;
        const float4 p = m.vert[ids[k]];
        float w[3] = {p.x, p.y, p.z}, cq[3];
        if (G) pose_point(G, w);
        wv[k][0] = w[0]; wv[k][1] = w[1]; wv[k][2] = w[2];
        to_camera(c, w, cq);
        q[k].x = cq[0]; q[k].y = cq[1]; q[k].z = cq[2];
        ok = ok && isfinite(q[k].x) && isfinite(q[k].y) && isfinite(q[k].z);
    }
    if (!ok) return;
    // shading: |n . v|, n the unit world-space face normal (two-sided), v the unit ray from the camera centre to the centroid
    // (the two edges that leave the vertex NEAREST the origin: from a finite vertex at 1e30, as the mesh fuzzer drew one, both edges
    // are that vertex's negative to sixteen digits, their cross product is exactly zero and the triangle was dropped as degenerate)
    int b0 = 0;
    float bmag = fabsf(wv[0][0]) + fabsf(wv[0][1]) + fabsf(wv[0][2]);
    for (int k = 1; k < 3; ++k) {
        const float mag = fabsf(wv[k][0]) + fabsf(wv[k][1]) + fabsf(wv[k][2]);
        if (mag < bmag) { bmag = mag; b0 = k; }
    }
    const int b1 = (b0 + 1) % 3, b2 = (b0 + 2) % 3;
    const double e1[3] = {(double)wv[b1][0] - wv[b0][0], (double)wv[b1][1] - wv[b0][1], (double)wv[b1][2] - wv[b0][2]};
    const double e2[3] = {(double)wv[b2][0] - wv[b0][0], (double)wv[b2][1] - wv[b0][1], (double)wv[b2][2] - wv[b0][2]};
    double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(nn > 0.0) || !isfinite(nn)) return;   // degenerate
    double d[3];
    for (int i = 0; i < 3; ++i) d[i] = ((double)wv[0][i] + (double)wv[1][i] + (double)wv[2][i]) / 3.0 - (double)c.campos[i];
    const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double ndv = dn > 0.0 ? fabs(n[0] * d[0] + n[1] * d[1] + n[2] * d[2]) / (nn * dn) : 1.0;
    const double shade = (double)m.ka + (double)m.kd * ndv;
    const float4 col = m.color[t];
    const float cr = (float)fmin(fmax((double)col.x * shade, 0.0), 1.0), cg = (float)fmin(fmax((double)col.y * shade, 0.0), 1.0),
                cb = (float)fmin(fmax((double)col.z * shade, 0.0), 1.0);
    // rule 2b: a triangle whose three vertices carry a normal is smooth -- per vertex clamp(c_k (ka + kd |n'_k . v_k|), 0, 1), n'_k the
    // normal under the 3x3 block of the triangle's pose row, renormalised, v_k the unit ray from the camera centre to the posed vertex
    double sv[3][3];
    bool smooth = planes != nullptr && m.vnormal != nullptr;
    for (int k = 0; k < 3 && smooth; ++k) {
        const float4 nk = m.vnormal[ids[k]];
        double nr[3] = {(double)nk.x, (double)nk.y, (double)nk.z};
        const double n_in = sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
        if (G) {
            const double x = nr[0], y = nr[1], z = nr[2];
            for (int i = 0; i < 3; ++i) nr[i] = (double)G[4 * i] * x + (double)G[4 * i + 1] * y + (double)G[4 * i + 2] * z;
        }
        const double nl = sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
        if (!(n_in > 0.0) || !(nl > 0.0) || !isfinite(nl)) { smooth = false; break; }   // no normal here: the triangle stays flat
        const double dv[3] = {(double)wv[k][0] - (double)c.campos[0], (double)wv[k][1] - (double)c.campos[1], (double)wv[k][2] - (double)c.campos[2]};
        const double dl = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
        const double nv = dl > 0.0 ? fabs(nr[0] * dv[0] + nr[1] * dv[1] + nr[2] * dv[2]) / (nl * dl) : 1.0;
        const double sh = (double)m.ka + (double)m.kd * nv;
        const float4 ck = m.vcolor ? m.vcolor[ids[k]] : col;
        sv[k][0] = fmin(fmax((double)ck.x * sh, 0.0), 1.0);
        sv[k][1] = fmin(fmax((double)ck.y * sh, 0.0), 1.0);
        sv[k][2] = fmin(fmax((double)ck.z * sh, 0.0), 1.0);
    }
    // near clip: the polygon's vertices in order, each edge that crosses z = kNear cut from its end NEARER the plane (a rule that
    // does not depend on the direction the edge is walked: a neighbour gets the same point).  Cut from an end at z = 1e30 -- a
    // finite vertex there, found by the mesh fuzzer -- the step back to the plane is the whole edge and i + s (o - i) cancels to
    // rounding noise of 1e13: the clipped corner landed at the principal point.
    // (a cut point's shades: the same step along the edge, in camera space)
    Vc poly[4];
    double pat[4][3];
    int np = 0;
    for (int k = 0; k < 3; ++k) {
        const int kb = (k + 1) % 3;
        const Vc &a = q[k], &b = q[kb];
        const bool ain = a.z >= (double)kNear, bin = b.z >= (double)kNear;
        if (ain) {
            if (smooth) for (int ch = 0; ch < 3; ++ch) pat[np][ch] = sv[k][ch];
            poly[np++] = a;
        }
        if (ain != bin) {
            const double da = fabs(a.z - (double)kNear), db = fabs(b.z - (double)kNear);
            const bool from_a = da < db || (da == db && ain);   // (a tie: the inside end, whichever way the edge is walked)
            const Vc &i = from_a ? a : b, &o = from_a ? b : a;
            const double s = ((double)kNear - i.z) / (o.z - i.z);
            if (smooth) {
                const double *si = from_a ? sv[k] : sv[kb], *so = from_a ? sv[kb] : sv[k];
                for (int ch = 0; ch < 3; ++ch) pat[np][ch] = si[ch] + s * (so[ch] - si[ch]);
            }
            poly[np++] = Vc{i.x + s * (o.x - i.x), i.y + s * (o.y - i.y), (double)kNear};
        }
    }
    for (int k = 0; k + 2 < np; ++k) {   // fan: one triangle, or two
        const Vc tri3[3] = {poly[0], poly[k + 1], poly[k + 2]};
        const int r = 2 * t + k;
        int4 rect;
        if (!mesh_record(c, tri3, mf.rec + 4 * r, rect)) continue;
        mf.rec[4 * r + 3] = make_float4(cr, cg, cb, 0.0f);
        if (planes) {
            float4 *pl = planes + SAS_MESH_PLANE_STRIDE * (long long)r;
            if (smooth) {
                const double at[3][3] = {{pat[0][0], pat[0][1], pat[0][2]}, {pat[k + 1][0], pat[k + 1][1], pat[k + 1][2]},
                                         {pat[k + 2][0], pat[k + 2][1], pat[k + 2][2]}};
                mesh_planes(c, tri3, at, pl);
            } else {
                pl[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        mf.rect[r] = rect;
        for (int ty = rect.y; ty <= rect.w; ++ty)
            for (int tx = rect.x; tx <= rect.z; ++tx) atomicAdd(&mf.tile_count[ty * c.tw + tx], 1);
    }
}

// One workgroup: exclusive scan of the tile counts into offsets and cursors; the total and the overflow flag to the host.
__global__ __launch_bounds__(kMeshScanThreads) void k_mesh_scan(SasMeshFrame mf, int tiles)
{
    __shared__ int s_w[kMeshScanThreads / 64];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int at = 0; at < tiles; at += kMeshScanThreads) {
        const int i = at + tid;
        const int v = i < tiles ? mf.tile_count[i] : 0;
        const int inc = (int)wave_inclusive_sum_u32((unsigned)v);
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        int before = s_base;
        for (int k = 0; k < wv; ++k) before += s_w[k];
        if (i < tiles) {
            mf.tile_offset[i] = before + inc - v;
            mf.tile_cursor[i] = before + inc - v;
        }
        __syncthreads();
        if (tid == kMeshScanThreads - 1) s_base = before + inc;
        __syncthreads();
    }
    if (tid == 0) {
        mf.tile_offset[tiles] = s_base;
        mf.status_host[0] = (unsigned)s_base;
        mf.status_host[1] = (long long)s_base > mf.cap ? 1u : 0u;
    }
}

// One thread per record: its index into the list of every tile of its rectangle (the order inside a list is free: k_blend_mesh
// keeps the minimum of (depth bits, triangle) whatever the order).
__global__ __launch_bounds__(kMeshSetupThreads) void k_mesh_scatter(SasMeshFrame mf, int n_rec, int tw)
{
    const int r = blockIdx.x * kMeshSetupThreads + threadIdx.x;
    if (r >= n_rec) return;
    const int4 rect = mf.rect[r];
    for (int ty = rect.y; ty <= rect.w; ++ty)
        for (int tx = rect.x; tx <= rect.z; ++tx) {
            const int pos = atomicAdd(&mf.tile_cursor[ty * tw + tx], 1);
            if (pos < mf.cap && SAS_IN(pos, mf.cap, 302)) mf.list[pos] = r;
        }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_mesh)

void sas_launch_mesh_bin(hipStream_t st, const SasMeshScene &m, const SasParams &P, const SasFrame &f, const SasMeshFrame &mf,
                         float4 *planes)
{
    const int tiles = P.cam.tw * P.cam.th;
    (void)hipMemsetAsync(mf.tile_count, 0, sizeof(int) * (size_t)tiles, st);
    const unsigned g1 = (unsigned)((m.nt + kMeshSetupThreads - 1) / kMeshSetupThreads);
    const unsigned g2 = (unsigned)((2 * m.nt + kMeshSetupThreads - 1) / kMeshSetupThreads);
    hipLaunchKernelGGL(k_mesh_setup, dim3(g1), dim3(kMeshSetupThreads), 0, st, m, P, f, mf, planes);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMeshScanThreads), 0, st, mf, tiles);
    hipLaunchKernelGGL(k_mesh_scatter, dim3(g2), dim3(kMeshSetupThreads), 0, st, mf, 2 * m.nt, P.cam.tw);
}
