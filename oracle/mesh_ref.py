"""Float64 reference of a frame's triangle meshes (DESIGN.md 3 "Meshes", rules 1 and 2) -- TEST INFRASTRUCTURE ONLY.

``reference`` answers, per pixel and brute force over all triangles (``mesh_ref.c``: no tiles, no rectangles, no records), which
triangle the pixel shows, at which camera depth and in which shaded colour.  The vertices are posed and moved to the camera
frame in float32 by the oracle's own fused chain (``oracle.pose_points``: the contract's "float, as the projection moves the
Gaussians"); near clip, projection, inside test, depth and shading are float64.

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


def reference(vertices, triangles, colors, groups, group_Rt, ka: float, kd: float, viewmat, K, W: int, H: int) -> Dict[str, np.ndarray]:
    """``vertices [V,3]``, ``triangles [T,3]``, ``colors [T,3]`` or ``[3]``, ``groups [T]`` or None, ``group_Rt [G,12]`` or None.
    Returns ``winner [H,W]`` (int32, -1: none), ``z``, ``kappa``, ``delta`` (float64), ``color [H,W,3]`` (float32: the shaded
    colour as the kernel stores it; 0 where no triangle), ``tri_color [T,3]``, ``valid [T]``, ``probe_differs`` and
    ``near_second`` (bool: (a) and (b) above)."""
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
    delta = DELTA_ULPS * EPS32 * kappa
    near_second = hit & (gap <= DELTA_ULPS * EPS32 * np.maximum(kappa, kappa2))
    return dict(winner=winner, z=z, kappa=kappa, delta=delta, color=color, tri_color=tri_color, valid=valid[:T].astype(bool),
                probe_differs=probe.astype(bool), near_second=near_second, camera_vertices=camv.reshape(T, 3, 3))


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
