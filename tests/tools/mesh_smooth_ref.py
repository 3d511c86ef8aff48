"""Float64 reference of smooth-shaded meshes (DESIGN.md 3 "Meshes", rule 2b) -- TEST INFRASTRUCTURE ONLY.

``oracle.mesh_ref.reference`` stays what it is: which triangle a pixel shows, at which depth, in which FLAT colour.  This module
overwrites the colour where the winner is a smooth triangle:

* a triangle is smooth when its three vertices carry a finite, non-zero normal (and the pose leaves it one);
* vertex shade ``s_k = clamp(c_k (ka + kd |n'_k . v_k|), 0, 1)``: ``n'_k`` the float32 normal under the 3x3 block of the float32 pose row,
  in float64, renormalised; ``v_k`` the unit vector from the camera centre to the posed vertex (``oracle.pose_points``: the float32
  world corners the kernel has); ``c_k`` the float32 vertex colour, or the triangle's colour without vertex colours;
* pixel colour ``sum_k beta_k s_k``, ``beta`` the barycentric coordinates, in the unclipped camera-space triangle (the float32 camera
  corners ``mesh_ref`` returns), of the point where the ray through the pixel centre meets the triangle's plane.

Nothing here knows records, planes, tiles or clipping: the near clip changes nothing mathematically, so the reference has none.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Dict, Optional

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402
from oracle import mesh_ref  # noqa: E402


def barycentric(ref: Dict[str, np.ndarray], K, W: int, H: int) -> np.ndarray:
    """``beta [H,W,3]`` float64 (0 where no triangle): ray through the pixel centre against the plane of the winner's unclipped
    camera-space triangle, then area ratios in that plane."""
    Km = np.asarray(K, np.float32).reshape(3, 3).astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    D = np.stack([((xs + 0.5) - Km[0, 2]) / Km[0, 0], ((ys + 0.5) - Km[1, 2]) / Km[1, 1], np.ones((H, W))], -1)
    win = ref["winner"]
    hit = win >= 0
    tri = ref["camera_vertices"].astype(np.float64)[win[hit]]            # [P,3,3]
    A, B, C = tri[:, 0], tri[:, 1], tri[:, 2]
    N = np.cross(B - A, C - A)
    d = D[hit]
    X = d * ((N * A).sum(1) / (N * d).sum(1))[:, None]                   # the hit point
    nn = (N * N).sum(1)
    beta = np.zeros((H, W, 3))
    beta[hit] = np.stack([(N * np.cross(C - B, X - B)).sum(1), (N * np.cross(A - C, X - C)).sum(1), (N * np.cross(B - A, X - A)).sum(1)], 1) / nn[:, None]
    return beta


def vertex_shades(vertices, triangles, colors, groups, group_Rt, ka, kd, viewmat, vertex_normals, vertex_colors=None):
    """``(shade [T,3,3] float64 -- triangle, corner, channel --, smooth [T] bool)`` of rule 2b."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = t.shape[0]
    g = np.zeros(T, np.uint8) if groups is None else np.broadcast_to(np.asarray(groups, np.uint8).reshape(-1), (T,))
    world, _, campos = oracle.pose_points(v[t.reshape(-1)], viewmat, np.repeat(g, 3), group_Rt)
    world = world.astype(np.float64).reshape(T, 3, 3)
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
        if vertex_colors is not None:
            c = np.asarray(vertex_colors, np.float32).reshape(-1, 3).astype(np.float64)[t]
        else:
            c = np.broadcast_to(np.asarray(colors, np.float32).reshape(-1, 3), (T, 3)).astype(np.float64)[:, None, :].repeat(3, 1)
        shade = np.clip(c * sh[..., None], 0.0, 1.0)
    return np.where(np.isfinite(shade), shade, 0.0), smooth


def reference(vertices, triangles, colors, groups, group_Rt, ka: float, kd: float, viewmat, K, W: int, H: int,
              vertex_normals=None, vertex_colors=None) -> Dict[str, np.ndarray]:
    """``mesh_ref.reference`` with ``color`` overwritten on smooth winners; also ``smooth_pixel [H,W]`` (the winner is a smooth
    triangle), ``smooth [T]``, ``beta [H,W,3]`` and ``color64`` (the float64 colour before rounding to float32)."""
    ref = mesh_ref.reference(vertices, triangles, colors, groups, group_Rt, ka, kd, viewmat, K, W, H)
    T = np.asarray(triangles).reshape(-1, 3).shape[0]
    ref["smooth"] = np.zeros(T, bool)
    ref["smooth_pixel"] = np.zeros((H, W), bool)
    ref["color64"] = ref["color"].astype(np.float64)
    if vertex_normals is None:
        return ref
    shade, smooth = vertex_shades(vertices, triangles, colors, groups, group_Rt, ka, kd, viewmat, vertex_normals, vertex_colors)
    beta = barycentric(ref, K, W, H)
    win = ref["winner"]
    sp = (win >= 0) & smooth[np.maximum(win, 0)]
    col = np.einsum("pk,pkc->pc", beta[sp], shade[win[sp]])
    ref["color64"][sp] = col
    ref["color"] = ref["color"].copy()
    ref["color"][sp] = col.astype(np.float32)
    ref.update(smooth=smooth, smooth_pixel=sp, beta=beta)
    return ref


def expected(case, view=0, mc=None, depth_mode=0):
    """``mesh_cases.expected`` for a case whose mesh may carry ``normals`` / ``vcols``: the same stability, counts and caps (they do
    not depend on colours), the frame rendered with the smooth reference's colours."""
    import mesh_cases as mc_
    mc = mc or mc_
    e = mc.expected(case, view, depth_mode)
    m = case["mesh"]
    if m.get("normals") is None:
        e["ref"].update(smooth_pixel=np.zeros(e["ref"]["winner"].shape, bool))
        return e
    sc, cam = case["sc"], case["cams"][view]
    V, K, W, H = cam
    Rt = None if case.get("poses") is None else case["poses"][view]
    if Rt is None:
        Rt = sc["Rt"]
    ref = reference(m["verts"], m["tris"], m["cols"], m["groups"], Rt if sc["gid"] is not None else None, m["ka"], m["kd"], V, K, W, H,
                    vertex_normals=m["normals"], vertex_colors=m.get("vcols"))
    assert np.array_equal(ref["winner"], e["ref"]["winner"])
    zlim, bgmap = mesh_ref.frame_inputs(ref, case["bg"])
    e["flat_frame"] = e["frame"]
    e["frame"] = mc.oracle_frame(sc, cam, case["bg"], Rt=Rt, zlim=zlim, bgmap=bgmap, depth_mode=depth_mode)
    e["ref"] = ref
    return e
