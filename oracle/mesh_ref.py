"""Float64 reference of a frame's triangle meshes (DESIGN.md 3 "Meshes", rules 1, 2 and 2b) -- TEST INFRASTRUCTURE ONLY.

``reference`` answers, per pixel and brute force over all triangles (``mesh_ref.c``: no tiles, no rectangles, no records), which
triangle the pixel shows, at which camera depth and in which shaded colour.  The vertices are posed and moved to the camera
frame in float32 by the oracle's own fused chain (``oracle.pose_points``: the contract's "float, as the projection moves the
Gaussians"); near clip, projection, inside test, depth and shading are float64.

The colour is the triangle's flat one (rule 2) unless the mesh carries vertex normals (rule 2b).  Then:

* a triangle is smooth when its three vertices carry a finite, non-zero normal (and the pose leaves it one);
* vertex shade ``s_k = clamp(c_k (ka + kd |n'_k . v_k|), 0, 1)``: ``n'_k`` the float32 normal under the 3x3 block of the float32 pose row,
  in float64, renormalised; ``v_k`` the unit vector from the camera centre to the posed vertex (the float32 world corners the kernel
  has); ``c_k`` the float32 vertex colour, or the triangle's colour without vertex colours;
* pixel colour ``sum_k beta_k s_k``, ``beta`` the barycentric coordinates, in the unclipped camera-space triangle (the float32 camera
  corners), of the point where the ray through the pixel centre meets the triangle's plane.

Rule 2b knows no records, planes, tiles or clipping: the near clip changes nothing mathematically, so the reference has none.

``frame_inputs`` turns that into what ``oracle.render(zlim=, bgmap=)`` takes, and ``stability`` says on which pixels the HIP
kernels, which evaluate edges and depth in float32, must reproduce the resulting frame bit for bit:

(a) the winner is the same at the four probes (+-1e-3, 0), (0, +-1e-3) px (edge errors stay far below 1e-3 px);
(b) no second covering triangle lies within delta, relative, of the winner's depth;
(c) no Gaussian of the pixel's tile list has a depth (the oracle's, which are the GPU's bits) within delta, relative, of z(p).

delta(p) = 16 * 2^-24 * kappa(p), kappa(p) = (|za x| + |zb y| + |zc|) / |za x + zb y + zc| in the kernel's image-centre frame.
Derivation: the kernel evaluates 1/z = za x + zb y + zc from three coefficients rounded to float32 (each 2^-24 relative), with
two products and two sums, fused or not (each at most 2^-24 of a term bounded by the numerator of kappa), and takes one
reciprocal of at most 2.5 ulp: together below 10 * 2^-24 * kappa; 16 leaves margin.  For (b) the second triangle's own
kappa counts as well (its depth is evaluated with its own coefficients): the larger of the two is used.  delta is derived, not
measured, and is not widened to make a case pass: a disagreement on a stable pixel is a finding.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

import oracle

DELTA_ULPS = 16.0
EPS32 = 2.0 ** -24


def barycentric(winner, camera_vertices, K, W: int, H: int) -> np.ndarray:
    """``beta [H,W,3]`` float64 (0 where no triangle): ray through the pixel centre against the plane of the winner's unclipped
    camera-space triangle, then area ratios in that plane."""
    Km = np.asarray(K, np.float32).reshape(3, 3).astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    D = np.stack([((xs + 0.5) - Km[0, 2]) / Km[0, 0], ((ys + 0.5) - Km[1, 2]) / Km[1, 1], np.ones((H, W))], -1)
    hit = winner >= 0
    tri = camera_vertices.astype(np.float64)[winner[hit]]                # [P,3,3]
    A, B, C = tri[:, 0], tri[:, 1], tri[:, 2]
    N = np.cross(B - A, C - A)
    d = D[hit]
    X = d * ((N * A).sum(1) / (N * d).sum(1))[:, None]                   # the hit point
    nn = (N * N).sum(1)
    beta = np.zeros((H, W, 3))
    beta[hit] = np.stack([(N * np.cross(C - B, X - B)).sum(1), (N * np.cross(A - C, X - C)).sum(1), (N * np.cross(B - A, X - A)).sum(1)], 1) / nn[:, None]
    return beta


def vertex_shades(world, campos, t, g, col, group_Rt, ka, kd, vertex_normals, vertex_colors=None):
    """``(shade [T,3,3] float64 -- triangle, corner, channel --, smooth [T] bool)`` of rule 2b, from ``reference``'s posed corners
    ``world [T,3,3]`` (float64), triangles ``t``, groups ``g`` and colours ``col [T,3]`` (float64)."""
    n = np.asarray(vertex_normals, np.float32).reshape(-1, 3).astype(np.float64)
    n = np.where(np.isfinite(n).all(1, keepdims=True), n, 0.0)[t]       # [T,3,3]; non-finite counts as zero
    n_in = np.linalg.norm(n, axis=2)
    if group_Rt is not None:
        R = np.asarray(group_Rt, np.float32).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)[g]     # [T,3,3]
        n = np.einsum("tij,tkj->tki", R, n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nl = np.linalg.norm(n, axis=2)
        smooth = ((n_in > 0) & (nl > 0) & np.isfinite(nl)).all(1)
        d = world - campos.astype(np.float64)
        dl = np.linalg.norm(d, axis=2)
        ndv = np.where(dl > 0, np.abs((n * d).sum(2)) / (nl * dl), 1.0)
        sh = float(np.float32(ka)) + float(np.float32(kd)) * ndv       # [T,3]
        c = col[:, None, :].repeat(3, 1) if vertex_colors is None else np.asarray(vertex_colors, np.float32).reshape(-1, 3).astype(np.float64)[t]
        shade = np.clip(c * sh[..., None], 0.0, 1.0)
    return np.where(np.isfinite(shade), shade, 0.0), smooth


def reference(vertices, triangles, colors, groups, group_Rt, ka: float, kd: float, viewmat, K, W: int, H: int,
              vertex_normals=None, vertex_colors=None) -> Dict[str, np.ndarray]:
    """``vertices [V,3]``, ``triangles [T,3]``, ``colors [T,3]`` or ``[3]``, ``groups [T]`` or None, ``group_Rt [G,12]`` or None,
    ``vertex_normals`` / ``vertex_colors [V,3]`` or None.
    Returns ``winner [H,W]`` (int32, -1: none), ``z``, ``kappa``, ``delta`` (float64), ``color [H,W,3]`` (float32: the shaded
    colour as the kernel stores it; 0 where no triangle), ``tri_color [T,3]`` (the flat colours), ``valid [T]``, ``probe_differs``
    and ``near_second`` (bool: (a) and (b) above); of rule 2b ``smooth [T]``, ``smooth_pixel [H,W]`` (the winner is a smooth
    triangle), ``beta [H,W,3]`` and ``color64`` (the colour before rounding to float32) -- without normals all-false, zero, and
    ``color`` as float64."""
    L = oracle.lib()
    W, H = int(W), int(H)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = t.shape[0]
    col = np.broadcast_to(np.asarray(colors, np.float32).reshape(-1, 3), (T, 3)).astype(np.float64)
    # (triangles without a group take group 0, as Rasterizer.upload_meshes hands them over; a scene without groups: unposed)
    g = np.zeros(T, np.uint8) if groups is None else np.broadcast_to(np.asarray(groups, np.uint8).reshape(-1), (T,))
    corners = v[t.reshape(-1)] if T else np.zeros((0, 3), np.float32)
    world, camv, campos = oracle.pose_points(corners, viewmat, np.repeat(g, 3), group_Rt)
    tris = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    Km = np.asarray(K, np.float32).reshape(3, 3).astype(np.float64)
    K4 = np.array([Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]], np.float64)
    winner = np.empty((H, W), np.int32)
    z, kappa, gap, kappa2 = (np.empty((H, W), np.float64) for _ in range(4))
    probe = np.empty((H, W), np.uint8)
    valid = np.zeros(max(T, 1), np.uint8)
    camv = np.ascontiguousarray(camv)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    if L.sas_mesh_ref(p(camv), 3 * T, p(tris), T, p(K4), W, H, p(winner), p(z), p(kappa), p(gap), p(kappa2), p(probe), p(valid)) != 0:
        raise MemoryError("mesh reference allocation failed")
    # shading (rule 2): unit world-space face normal after the pose, unit ray from the camera centre to the centroid
    w = world.astype(np.float64).reshape(T, 3, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b0 = np.argmin(np.abs(w).sum(2), axis=1)       # the edges that leave the vertex nearest the origin: from a vertex at 1e30
        rows = np.arange(T)                             # both edges are its negative and their cross product is rounding noise
        o = w[rows, b0]
        n = np.cross(w[rows, (b0 + 1) % 3] - o, w[rows, (b0 + 2) % 3] - o)
        d = w.mean(1) - campos.astype(np.float64)
        nn, dn = np.linalg.norm(n, axis=1), np.linalg.norm(d, axis=1)
        ndv = np.where(dn > 0, np.abs((n * d).sum(1)) / (nn * dn), 1.0)
        shade = float(np.float32(ka)) + float(np.float32(kd)) * ndv
        tri_color = np.clip(col * shade[:, None], 0.0, 1.0)
    tri_color = np.where(np.isfinite(tri_color), tri_color, 0.0).astype(np.float32)
    color = np.zeros((H, W, 3), np.float32)
    hit = winner >= 0
    color[hit] = tri_color[winner[hit]]
    cam3 = camv.reshape(T, 3, 3)
    smooth, sp, beta, color64 = np.zeros(T, bool), np.zeros((H, W), bool), np.zeros((H, W, 3)), color.astype(np.float64)
    if vertex_normals is not None:
        vshade, smooth = vertex_shades(w, campos, t, g, col, group_Rt, ka, kd, vertex_normals, vertex_colors)
        beta = barycentric(winner, cam3, K, W, H)
        sp = hit & smooth[np.maximum(winner, 0)]
        color64[sp] = np.einsum("pk,pkc->pc", beta[sp], vshade[winner[sp]])
        color[sp] = color64[sp].astype(np.float32)
    delta = DELTA_ULPS * EPS32 * kappa
    near_second = hit & (gap <= DELTA_ULPS * EPS32 * np.maximum(kappa, kappa2))
    return dict(winner=winner, z=z, kappa=kappa, delta=delta, color=color, tri_color=tri_color, valid=valid[:T].astype(bool),
                probe_differs=probe.astype(bool), near_second=near_second, camera_vertices=cam3, smooth=smooth, smooth_pixel=sp,
                beta=beta, color64=color64)


def frame_inputs(ref: Dict[str, np.ndarray], background):
    """``(zlim [H,W], bgmap [H,W,3])`` for ``oracle.render``: float32(z), +Inf where no triangle; the shaded colour, the
    frame's background where no triangle."""
    hit = ref["winner"] >= 0
    zlim = np.where(hit, ref["z"], np.inf).astype(np.float32)
    bgmap = np.where(hit[..., None], ref["color"], np.asarray(background, np.float32).reshape(1, 1, 3)).astype(np.float32)
    return zlim, bgmap


def stability(ref: Dict[str, np.ndarray], dump: Optional[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """``dump``: an ``oracle.render(..., dump=True)`` of the same camera (None: a frame without Gaussians).  Returns ``stable
    [H,W]`` and, per pixel, ``length`` of its tile's list and ``cut``, the number of entries in front of the depth limit (the
    entries the pixel may composite; ``length`` where no triangle covers it)."""
    H, W = ref["winner"].shape
    hit = ref["winner"] >= 0
    stable = ~ref["probe_differs"] & ~ref["near_second"]
    length = np.zeros((H, W), np.int64)
    cut = np.zeros((H, W), np.int64)
    if dump is not None:
        tw, th = (W + 15) // 16, (H + 15) // 16
        off, ids, depths = dump["tile_offsets"], dump["sorted_ids"], dump["depths"]
        zl = np.where(hit, ref["z"], np.inf).astype(np.float32)
        for ty in range(th):
            for tx in range(tw):
                a, b = int(off[ty * tw + tx]), int(off[ty * tw + tx + 1])
                sl = (slice(16 * ty, min(16 * ty + 16, H)), slice(16 * tx, min(16 * tx + 16, W)))
                length[sl] = b - a
                if b == a:
                    continue
                dz = depths[ids[a:b]]                                  # ascending: the list's order
                cut[sl] = np.searchsorted(dz, zl[sl], side="left")     # entries with depth < zlim
                if not hit[sl].any():
                    continue
                zz = ref["z"][sl]
                d64 = dz.astype(np.float64)
                k = np.clip(np.searchsorted(d64, zz), 0, d64.size - 1)
                near = np.minimum(np.abs(d64[k] - zz), np.abs(d64[np.maximum(k - 1, 0)] - zz))
                with np.errstate(invalid="ignore"):
                    stable[sl] &= ~(hit[sl] & (near <= ref["delta"][sl] * zz))
    return dict(stable=stable, length=length, cut=cut)
