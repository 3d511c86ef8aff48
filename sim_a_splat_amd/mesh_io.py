"""Triangle mesh readers (and an OBJ writer) for the meshes a scene composites (Rasterizer.upload_meshes; DESIGN.md 3, "Meshes").

They need neither trimesh nor open3d: the reference loads the pushT task object (an OBJ) and the URDF visuals (STL or OBJ)
through trimesh only to hand vertices and faces to viser (splat_handler.py:145-219).  Every reader returns
``(vertices [V,3] float64, faces [F,3] int64)``.  ``weld`` and ``vertex_normals`` prepare a loaded mesh for smooth shading (rule 2b): the
reference gets its vertex normals from open3d / trimesh.
"""
from __future__ import annotations

import struct
from pathlib import Path
from typing import Tuple, Union

import numpy as np

PathLike = Union[str, Path]


def load_obj(path: PathLike) -> Tuple[np.ndarray, np.ndarray]:
    """Wavefront OBJ: ``v`` records and ``f`` records in the forms ``v``, ``v/vt``, ``v//vn`` and ``v/vt/vn``; 1-based and
    negative (relative to the vertices read so far) indices; polygons triangulated as fans (0, k, k + 1)."""
    verts, faces = [], []
    for line in Path(path).read_text(errors="replace").splitlines():
        parts = line.split()
        if not parts:
            continue
        if parts[0] == "v":
            verts.append([float(x) for x in parts[1:4]])
        elif parts[0] == "f":
            idx = []
            for tok in parts[1:]:
                i = int(tok.split("/")[0])
                idx.append(i - 1 if i > 0 else len(verts) + i)
            for k in range(1, len(idx) - 1):
                faces.append([idx[0], idx[k], idx[k + 1]])
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index out of range")
    return v, f


def load_obj_colors(path: PathLike):
    """The per-vertex colours ``save_obj`` writes behind the coordinates (``v x y z r g b``, 0..1): ``[V,3]`` uint8, or None when any
    vertex has none."""
    cols = []
    for line in Path(path).read_text(errors="replace").splitlines():
        parts = line.split()
        if parts and parts[0] == "v":
            if len(parts) < 7:
                return None
            cols.append([float(x) for x in parts[4:7]])
    return np.clip(np.rint(np.asarray(cols, np.float64).reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)


def save_obj(path: PathLike, vertices, faces, colors=None) -> None:
    """Wavefront OBJ: one ``v x y z`` line per vertex (17 significant digits: ``load_obj`` reads the float64 back exactly), with
    ``colors [V,3]`` uint8 as ``r g b`` in 0..1 behind the coordinates (the common vertex-colour extension; k/255 in 6 decimals reads
    back as k), and one 1-based ``f`` line per triangle."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("save_obj: face index out of range")
    c = None
    if colors is not None:
        c = np.asarray(colors, np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"save_obj: {len(c)} colours for {len(v)} vertices")
    lines = []
    for k in range(len(v)):
        tail = "" if c is None else " " + " ".join(f"{x / 255.0:.6f}" for x in c[k])
        lines.append("v " + " ".join(repr(float(x)) for x in v[k]) + tail)
    lines += [f"f {a + 1} {b + 1} {d + 1}" for a, b, d in f.tolist()]
    Path(path).write_text("\n".join(lines) + "\n")


def _stl_is_binary(data: bytes) -> bool:
    if len(data) >= 84:
        n = struct.unpack_from("<I", data, 80)[0]
        if 84 + 50 * n == len(data):
            return True
    return not data.lstrip().startswith(b"solid")


def load_stl(path: PathLike) -> Tuple[np.ndarray, np.ndarray]:
    """STL, binary or ASCII.  Every facet keeps its own three vertices (faces [[0,1,2],[3,4,5],...]), as STL stores them."""
    data = Path(path).read_bytes()
    if _stl_is_binary(data):
        n = struct.unpack_from("<I", data, 80)[0]
        rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), count=n, offset=84)
        v = rec["v"].reshape(-1, 3).astype(np.float64)
    else:
        v = np.array([[float(x) for x in line.split()[1:4]] for line in data.decode(errors="replace").splitlines()
                      if line.strip().startswith("vertex")], np.float64).reshape(-1, 3)
        if len(v) % 3:
            raise ValueError(f"{path}: {len(v)} vertices is not a whole number of facets")
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)


def load_mesh(path: PathLike) -> Tuple[np.ndarray, np.ndarray]:
    """By suffix: ``.obj`` or ``.stl`` (any letter case)."""
    suf = Path(path).suffix.lower()
    if suf == ".obj":
        return load_obj(path)
    if suf == ".stl":
        return load_stl(path)
    raise ValueError(f"{path}: unsupported mesh format {suf!r} (OBJ and STL are read)")


def weld(vertices, faces) -> Tuple[np.ndarray, np.ndarray]:
    """Merge vertices whose float32 positions are bit-equal (``load_stl`` returns three private vertices per triangle, so that
    no vertex is shared and no normal can be averaged).  Returns ``(vertices [U,3] float64, faces [F,3] int64)``: the unique
    positions in order of first appearance, the faces re-indexed; +0 and -0 stay apart, as do NaNs of different bits."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(v) == 0:
        return v.copy(), f.copy()
    bits = np.ascontiguousarray(v.astype(np.float32)).view(np.uint32).reshape(-1, 3)
    key = bits.astype(np.uint64)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # unique rows by first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return v[first[order]].copy(), rank[np.asarray(inverse).reshape(-1)][f]


def vertex_normals(vertices, faces) -> np.ndarray:
    """Unit vertex normals ``[V,3]`` float64: the sum over a vertex's faces of the unit face normal weighted by the face's
    interior angle at that vertex, normalised.  Degenerate faces contribute nothing; a vertex without a usable face gets a
    zero normal ("no normal": its triangles stay flat)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros_like(v)
    if len(f) == 0:
        return out
    tri = v[f]                                               # [F,3,3]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fl = np.linalg.norm(fn, axis=1)
    ok = np.isfinite(fl) & (fl > 0)
    fn = np.where(ok[:, None], fn / np.where(ok, fl, 1.0)[:, None], 0.0)
    for k in range(3):
        a, b = tri[:, (k + 1) % 3] - tri[:, k], tri[:, (k + 2) % 3] - tri[:, k]
        la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            ang = np.arccos(np.clip((a * b).sum(1) / (la * lb), -1.0, 1.0))
        ang = np.where(ok & np.isfinite(ang), ang, 0.0)
        np.add.at(out, f[:, k], fn * ang[:, None])
    n = np.linalg.norm(out, axis=1)
    good = np.isfinite(n) & (n > 0)
    return np.where(good[:, None], out / np.where(good, n, 1.0)[:, None], 0.0)


def sample_surface(vertices, faces, n: int, seed: int = 0) -> np.ndarray:
    """``n`` points on the surface, ``[n,3]`` float64, area-weighted and stratified: point k takes the triangle that the cumulative
    triangle areas assign to ``u_k = (k + r_k) / n``, and a place in it by the square-root rule (``s = sqrt(r1)``:
    ``(1 - s) A + s (1 - r2) B + s r2 C``, uniform over the triangle).  ``r_k, r1, r2`` come from ``numpy.random.default_rng(seed)``:
    the same arguments give the same bits.  Triangles of zero or non-finite area carry no weight and receive no point; a triangle
    of area share ``a`` receives between ``n a - 2`` and ``n a + 2`` points.  ValueError when no triangle has an area.

    The reference samples its robot with open3d's ``sample_points_poisson_disk`` (match_splat.py:103), which draws more points than
    asked and eliminates the closest ones; that elimination is not reproduced here -- stratification spreads the points evenly over
    the area, not by mutual distance."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = int(n)
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    tri = v[f]                                               # [F,3,3]
    with np.errstate(invalid="ignore", over="ignore"):
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) if len(f) else np.zeros(0)
    area = np.where(np.isfinite(area) & np.isfinite(tri).all(axis=(1, 2)), area, 0.0)
    cum = np.cumsum(area)
    if len(cum) == 0 or not cum[-1] > 0.0 or not np.isfinite(cum[-1]):
        raise ValueError("sample_surface: the mesh has no triangle with a finite, positive area")
    r = np.random.default_rng(seed).random((n, 3))
    u = (np.arange(n) + r[:, 0]) / max(n, 1)
    t = np.minimum(np.searchsorted(cum, u * cum[-1], side="right"), int(np.flatnonzero(area > 0.0)[-1]))
    s = np.sqrt(r[:, 1])
    A, B, C = tri[t, 0], tri[t, 1], tri[t, 2]
    return (1.0 - s)[:, None] * A + (s * (1.0 - r[:, 2]))[:, None] * B + (s * r[:, 2])[:, None] * C
