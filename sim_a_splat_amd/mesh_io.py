"""Triangle mesh readers for the meshes a scene composites (Rasterizer.upload_meshes; DESIGN.md 3, "Meshes").

They need neither trimesh nor open3d: the reference loads the pushT task object (an OBJ) and the URDF visuals (STL or OBJ)
through trimesh only to hand vertices and faces to viser (splat_handler.py:145-219).  Every reader returns
``(vertices [V,3] float64, faces [F,3] int64)``.
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
