/*
 * mesh_ref.c -- float64 reference of the mesh rules 1 and 2 of DESIGN.md 3 "Meshes" (coverage and depth), per pixel and
 * brute force over all triangles: no tiles, no rectangles, no records.  TEST INFRASTRUCTURE (see oracle/mesh_ref.py).
 *
 * Input: camera-frame vertices in float32 (sas_oracle_pose_points: the contract moves mesh vertices "in float, as the
 * projection moves the Gaussians"); everything below is float64.  A triangle is the set of camera rays that meet it at
 * z >= 0.01: it is clipped at the near plane into a convex polygon of 3 or 4 corners, and a pixel centre is inside when its
 * ray lies on the inner side of the plane through the camera centre and each edge (the projected edge function, see mr_setup).  Its depth comes from the triangle's PLANE
 * n . P = d in camera space: 1/z = n . ((u - cx)/fx, (v - cy)/fy, 1) / d, which is the "1/z linear in screen space" of the
 * contract without going through projected vertices.  The nearest covering triangle wins.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define MR_NEAR 0.01
#define MR_PROBE 1e-3   /* px: the winner must be the same at (+-1e-3, 0) and (0, +-1e-3) */

typedef struct {
    int ne;              /* 0: dropped */
    double a[4], b[4], c[4];   /* edge k: a x + b y + c >= 0 inside; (x, y) relative to the image centre */
    double za, zb, zc;   /* 1/z = za x + zb y + zc in the same frame */
} mr_tri;

static int mr_setup(const float *cv, const int32_t *t, const double K[4], double xo, double yo, mr_tri *o)
{
    o->ne = 0;
    double P[3][3];
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) {
            P[k][i] = (double)cv[3 * (int64_t)t[k] + i];
            if (!isfinite(P[k][i])) return 0;
        }
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    /* the plane's normal from the two edges that leave the corner NEAREST the camera centre, and d at that corner: with a corner
     * at 1e30 as the base both edges are that corner's negative to sixteen digits and their cross product is rounding noise */
    int b0 = 0;
    double best = INFINITY;
    for (int k = 0; k < 3; ++k) {
        const double m = fabs(P[k][0]) + fabs(P[k][1]) + fabs(P[k][2]);
        if (m < best) { best = m; b0 = k; }
    }
    const double *B0 = P[b0], *B1 = P[(b0 + 1) % 3], *B2 = P[(b0 + 2) % 3];
    double e1[3], e2[3];
    for (int i = 0; i < 3; ++i) { e1[i] = B1[i] - B0[i]; e2[i] = B2[i] - B0[i]; }
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(nn > 0.0) || !isfinite(nn)) return 0;                      /* degenerate */
    const double d = n[0] * B0[0] + n[1] * B0[1] + n[2] * B0[2];
    if (!(fabs(d) > 0.0) || !isfinite(d)) return 0;                  /* seen edge-on: its plane holds the camera centre */
    /* 1/z at pixel (u, v): (nx (u - cx)/fx + ny (v - cy)/fy + nz) / d; (u, v) = (x + xo, y + yo) */
    o->za = n[0] / (fx * d);
    o->zb = n[1] / (fy * d);
    o->zc = (n[0] * (xo - cx) / fx + n[1] * (yo - cy) / fy + n[2]) / d;
    /* near clip */
    double poly[4][3];
    int np = 0;
    for (int k = 0; k < 3; ++k) {
        const double *A = P[k], *B = P[(k + 1) % 3];
        const int ain = A[2] >= MR_NEAR, bin = B[2] >= MR_NEAR;
        if (ain) { poly[np][0] = A[0]; poly[np][1] = A[1]; poly[np][2] = A[2]; ++np; }
        if (ain != bin) {
            /* cut from the end NEARER the near plane: from an end at z = 1e30 the step back to the plane is the whole edge, and
             * the sum cancels to rounding noise of 1e13 */
            const double da = fabs(A[2] - MR_NEAR), db = fabs(B[2] - MR_NEAR);
            const int from_a = da < db || (da == db && ain);
            const double *I = from_a ? A : B, *O = from_a ? B : A;
            const double s = (MR_NEAR - I[2]) / (O[2] - I[2]);
            poly[np][0] = I[0] + s * (O[0] - I[0]); poly[np][1] = I[1] + s * (O[1] - I[1]); poly[np][2] = MR_NEAR;
            ++np;
        }
    }
    if (np < 3) return 0;
    /* Edge k of the clipped polygon, as a function of the pixel: the ray r = ((u - cx)/fx, (v - cy)/fy, 1) lies on the inner side
     * of the plane through the camera centre and the edge when r . (P_k x P_j) has the polygon's orientation, the sign of
     * P_2 . (P_0 x P_1).  This is the projected edge function times z_k z_j > 0, without the projection: a corner that
     * projects 1e30 px away (a vertex at 1e30, a corner clipped at the near plane) costs no digit of the edges that pass the image. */
    double N[4][3];
    for (int k = 0; k < np; ++k) {
        const double *A = poly[k], *B = poly[(k + 1) % np];
        N[k][0] = A[1] * B[2] - A[2] * B[1]; N[k][1] = A[2] * B[0] - A[0] * B[2]; N[k][2] = A[0] * B[1] - A[1] * B[0];
    }
    const double orient = poly[2][0] * N[0][0] + poly[2][1] * N[0][1] + poly[2][2] * N[0][2];
    if (!(fabs(orient) > 0.0) || !isfinite(orient)) return 0;
    const double sgn = orient > 0.0 ? 1.0 : -1.0;
    for (int k = 0; k < np; ++k) {
        o->a[k] = sgn * N[k][0] / fx;
        o->b[k] = sgn * N[k][1] / fy;
        o->c[k] = sgn * (N[k][0] * (xo - cx) / fx + N[k][1] * (yo - cy) / fy + N[k][2]);
        if (!isfinite(o->a[k]) || !isfinite(o->b[k]) || !isfinite(o->c[k])) return 0;
    }
    o->ne = np;
    return 1;
}

/*
 * cv [nv,3] camera-frame vertices, tris [nt,3], K4 = {fx, fy, cx, cy}.  Per pixel: winner (-1: none), z, kappa
 * = (|za x| + |zb y| + |zc|) / |za x + zb y + zc| of the winner in the image-centre frame, gap = (z2 - z) / z of the second
 * nearest covering triangle (+Inf: none) with kappa2 its own kappa, and probe_differs = 1 where the winner at one of the four
 * probes is another triangle (or none).  valid [nt] = 1 for the triangles that are not dropped.  Returns 0, -1 on allocation failure.
 */
int sas_mesh_ref(const float *cv, int64_t nv, const int32_t *tris, int64_t nt, const double K4[4], int W, int H,
                 int32_t *winner, double *z, double *kappa, double *gap, double *kappa2, uint8_t *probe_differs, uint8_t *valid)
{
    (void)nv;
    mr_tri *T = (mr_tri *)malloc(sizeof(mr_tri) * (size_t)(nt > 0 ? nt : 1));
    if (!T) return -1;
    const double xo = 0.5 * (double)W, yo = 0.5 * (double)H;
    for (int64_t t = 0; t < nt; ++t) {
        const int ok = mr_setup(cv, tris + 3 * t, K4, xo, yo, &T[t]);
        if (valid) valid[t] = (uint8_t)ok;
    }
    static const double PX[5] = {0.0, MR_PROBE, -MR_PROBE, 0.0, 0.0}, PY[5] = {0.0, 0.0, 0.0, MR_PROBE, -MR_PROBE};
#pragma omp parallel for schedule(dynamic, 4)
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const double x = (double)j + 0.5 - xo, y = (double)i + 0.5 - yo;
            double best[5], second = INFINITY, k1 = 0.0, k2 = 0.0;
            int32_t who[5];
            for (int q = 0; q < 5; ++q) { best[q] = INFINITY; who[q] = -1; }
            for (int64_t t = 0; t < nt; ++t) {
                const mr_tri *r = &T[t];
                int maybe = r->ne > 0;
                for (int k = 0; k < r->ne && maybe; ++k)
                    if (r->a[k] * x + r->b[k] * y + r->c[k] < -MR_PROBE * (fabs(r->a[k]) + fabs(r->b[k]))) maybe = 0;
                if (!maybe) continue;
                for (int q = 0; q < 5; ++q) {
                    const double xq = x + PX[q], yq = y + PY[q];
                    int in = 1;
                    for (int k = 0; k < r->ne; ++k)
                        if (!(r->a[k] * xq + r->b[k] * yq + r->c[k] >= 0.0)) in = 0;
                    if (!in) continue;
                    const double iz = r->za * xq + r->zb * yq + r->zc;
                    if (!(iz > 0.0)) continue;
                    const double zz = 1.0 / iz;
                    const double kk = (fabs(r->za * xq) + fabs(r->zb * yq) + fabs(r->zc)) / iz;
                    if (q == 0) {
                        if (zz < best[0]) { second = best[0]; k2 = k1; best[0] = zz; who[0] = (int32_t)t; k1 = kk; }
                        else if (zz < second) { second = zz; k2 = kk; }
                    } else if (zz < best[q]) { best[q] = zz; who[q] = (int32_t)t; }
                }
            }
            const int64_t p = (int64_t)i * W + j;
            winner[p] = who[0];
            z[p] = best[0];
            kappa[p] = who[0] >= 0 ? k1 : 0.0;
            gap[p] = (who[0] >= 0 && isfinite(second)) ? (second - best[0]) / best[0] : INFINITY;
            kappa2[p] = k2;
            probe_differs[p] = (uint8_t)(who[1] != who[0] || who[2] != who[0] || who[3] != who[0] || who[4] != who[0]);
        }
    free(T);
    return 0;
}
