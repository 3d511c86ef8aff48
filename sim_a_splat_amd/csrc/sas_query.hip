// sas_query.hip -- point-to-mesh queries (sas_query_meshes; DESIGN.md 3, "Mesh queries"): for every (mesh, point) pair the
// unsigned distance to the mesh and its generalised winding number at the point.  The segmentation step of the reference asks
// exactly this of every Gaussian centre and every robot link (match_splat.py:240-251, through open3d's RaycastingScene).
//
//   k_query_cull   one thread per (point, mesh): the point against the mesh's box inflated by max_distance.  Pairs outside read
//                  +inf / 0 at once; the others are compacted into the mesh's candidate list (one returning atomic per wave).  The
//                  order of a list is free: a candidate's result does not depend on the lane that computes it.
//   k_query_eval   one candidate per lane, 256 lanes, grid (candidate blocks, mesh).  The mesh's triangles pass through LDS in
//                  chunks of SAS_QUERY_CHUNK, three float4 each, and every lane reads the same address (a broadcast ds_read_b128):
//                  per triangle one closest-point evaluation, a running minimum of d^2 and a running sum of the solid angles, in
//                  triangle order -- a pair's result is the same bits whatever else the call holds.
// Arithmetic: IEEE binary32, nothing fused (the translation unit is built with -ffp-contract=off and writes no fma_).
#include "sas_device.h"

namespace {

constexpr int kQueryThreads = 256;
static_assert(SAS_QUERY_CHUNK == kQueryThreads, "every thread of k_query_eval stages one triangle of a chunk");

DEV float dot_(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// squared distance from the origin to the segment from a along e (a zero-length segment is its point)
DEV float segment_d2(float ax, float ay, float az, float ex, float ey, float ez)
{
    const float len2 = dot_(ex, ey, ez, ex, ey, ez);
    float t = len2 > 0.0f ? -dot_(ax, ay, az, ex, ey, ez) / len2 : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);   // (a NaN quotient -- overflowed dots -- clamps to 0)
    const float qx = ax + t * ex, qy = ay + t * ey, qz = az + t * ez;
    return dot_(qx, qy, qz, qx, qy, qz);
}

__global__ __launch_bounds__(kQueryThreads) void k_query_cull(SasQuery q)
{
    const int m = blockIdx.y;
    const long long i = (long long)blockIdx.x * kQueryThreads + threadIdx.x;
    const SasQueryMesh box = q.mesh[m];
    bool in = false;
    if (i < q.n) {
        const float px = q.points[3 * i], py = q.points[3 * i + 1], pz = q.points[3 * i + 2];
        const float md = q.max_distance;
        const bool finite = fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY;   // (false for a NaN)
        const bool outside = px < box.lo[0] - md || px > box.hi[0] + md || py < box.lo[1] - md || py > box.hi[1] + md ||
                             pz < box.lo[2] - md || pz > box.hi[2] + md;
        in = finite && box.count > 0 && !outside;
    }
    const unsigned long long vote = __ballot(in);   // (every lane of the wave is here: no lane has returned)
    if (vote != 0ull) {
        int base = 0;
        if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(vote)) base = atomicAdd(&q.count[m], (int)__popcll(vote));
        base = __builtin_amdgcn_readlane(base, __builtin_ctzll(vote));
        const long long pos = (long long)base + mbcnt64(vote);
        if (in && SAS_IN(pos, q.n, 401)) q.list[(long long)m * q.n + pos] = (int)i;
    }
    if (i < q.n && !in && SAS_IN((long long)m * q.n + i, (long long)q.n_meshes * q.n, 402)) {
        if (q.distance) q.distance[(long long)m * q.n + i] = INFINITY;
        if (q.winding) q.winding[(long long)m * q.n + i] = 0.0f;
    }
}

__global__ __launch_bounds__(kQueryThreads) void k_query_eval(SasQuery q)
{
    __shared__ float4 s_tri[3 * SAS_QUERY_CHUNK];
    const int m = blockIdx.y, tid = threadIdx.x;
    const int cand = q.count[m];
    if ((long long)blockIdx.x * kQueryThreads >= cand) return;   // (uniform: the whole workgroup leaves)
    const SasQueryMesh mesh = q.mesh[m];
    const long long k = (long long)blockIdx.x * kQueryThreads + tid;
    const bool active = k < cand && SAS_IN(k, q.n, 403);
    long long i = active ? q.list[(long long)m * q.n + k] : 0;
    if (!SAS_IN(i, q.n, 404)) i = 0;
    const float px = q.points[3 * i], py = q.points[3 * i + 1], pz = q.points[3 * i + 2];
    float best = INFINITY, sum = 0.0f;
    for (int base = 0; base < mesh.count; base += SAS_QUERY_CHUNK) {
        const int nload = min(SAS_QUERY_CHUNK, mesh.count - base);
        __syncthreads();   // the chunk before has been read
        if (tid < nload && SAS_IN(mesh.start + base + tid, q.n_tri, 405) && SAS_IN(3 * tid + 2, 3 * SAS_QUERY_CHUNK, 406)) {
            const float4 *src = q.tri + 3 * (long long)(mesh.start + base + tid);
            s_tri[3 * tid] = src[0];
            s_tri[3 * tid + 1] = src[1];
            s_tri[3 * tid + 2] = src[2];
        }
        __syncthreads();
        for (int t = 0; t < nload; ++t) {
            const float4 A = s_tri[3 * t], B = s_tri[3 * t + 1], C = s_tri[3 * t + 2];
            // the vertices seen from the point, and the edges from the vertices themselves
            const float ax = A.x - px, ay = A.y - py, az = A.z - pz;
            const float bx = B.x - px, by = B.y - py, bz = B.z - pz;
            const float cx = C.x - px, cy = C.y - py, cz = C.z - pz;
            const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;   // A -> B
            const float e2x = C.x - A.x, e2y = C.y - A.y, e2z = C.z - A.z;   // A -> C
            const float e3x = C.x - B.x, e3y = C.y - B.y, e3z = C.z - B.z;   // B -> C
            // distance: the nearest of the three edges, or the plane where the point projects into the triangle
            float d2 = fminf(fminf(segment_d2(ax, ay, az, e1x, e1y, e1z), segment_d2(bx, by, bz, e3x, e3y, e3z)),
                             segment_d2(ax, ay, az, e2x, e2y, e2z));
            const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const float nn = dot_(nx, ny, nz, nx, ny, nz);
            float omega = 0.0f;
            if (nn > 0.0f) {   // (a zero-area triangle: its edges, and no solid angle)
                const float s1 = dot_(nx, ny, nz, ay * e1z - az * e1y, az * e1x - ax * e1z, ax * e1y - ay * e1x);   // n . (a x e1)
                const float s2 = dot_(nx, ny, nz, by * e3z - bz * e3y, bz * e3x - bx * e3z, bx * e3y - by * e3x);   // n . (b x e3)
                const float s3 = dot_(nx, ny, nz, e2y * cz - e2z * cy, e2z * cx - e2x * cz, e2x * cy - e2y * cx);   // n . (e2 x c)
                if (s1 >= 0.0f && s2 >= 0.0f && s3 >= 0.0f) {
                    const float h = dot_(nx, ny, nz, ax, ay, az);
                    d2 = fminf(d2, h * h / nn);
                }
                const float la = sqrtf(dot_(ax, ay, az, ax, ay, az)), lb = sqrtf(dot_(bx, by, bz, bx, by, bz)),
                            lc = sqrtf(dot_(cx, cy, cz, cx, cy, cz));
                const float num = dot_(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);   // a . (b x c)
                const float den = la * lb * lc + dot_(ax, ay, az, bx, by, bz) * lc + dot_(bx, by, bz, cx, cy, cz) * la +
                                  dot_(cx, cy, cz, ax, ay, az) * lb;
                omega = atan2f(num, den);
                if (!(fabsf(omega) < INFINITY)) omega = 0.0f;   // (overflowed products: no NaN leaves the kernel)
            }
            best = fminf(best, d2);   // (fminf drops a NaN)
            sum = sum + omega;
        }
    }
    if (active && SAS_IN((long long)m * q.n + i, (long long)q.n_meshes * q.n, 407)) {
        if (q.distance) q.distance[(long long)m * q.n + i] = sqrtf(best);
        if (q.winding) q.winding[(long long)m * q.n + i] = sum * 0.15915494309189535f;   // sum of 2 atan2 over 4 pi
    }
}

}  // namespace

SAS_BOUNDS_ACCESSOR(sas_debug_bounds_query)

void sas_launch_query(hipStream_t st, const SasQuery &q)
{
    if (q.n <= 0) return;
    const dim3 grid((unsigned)((q.n + kQueryThreads - 1) / kQueryThreads), (unsigned)q.n_meshes);
    (void)hipMemsetAsync(q.count, 0, sizeof(int) * (size_t)q.n_meshes, st);
    hipLaunchKernelGGL(k_query_cull, grid, dim3(kQueryThreads), 0, st, q);
    // the candidate counts stay on the device: workgroups beyond a mesh's count leave at once
    hipLaunchKernelGGL(k_query_eval, grid, dim3(kQueryThreads), 0, st, q);
}
