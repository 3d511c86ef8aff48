"""Meshes, points and tolerances shared by the mesh-query tests (tests/test_segment_cpu.py, tests/test_gpu_l_mesh_query.py,
tools/mesh_query_probe.py): the committed meshes, a box, the single-triangle cases, and the per-case tolerances the GPU is held to.
References are computed once per (case, dtype) and shared (``reference``)."""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import mesh_query_ref as ref  # noqa: E402

from sim_a_splat_amd import mesh_io  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def box_mesh(h=(0.5, 0.3, 0.2), centre=(0.0, 0.0, 0.0)):
    """Axis-aligned box of half extents ``h``: 8 vertices, 12 triangles, counter-clockwise seen from outside."""
    h, c = np.asarray(h, np.float64), np.asarray(centre, np.float64)
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h + c   # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x +x -y +y -z +z
    f = np.array([t for a, b, c_, d in quads for t in ((a, b, c_), (a, c_, d))], np.int64)
    return v, f


@functools.lru_cache(maxsize=None)
def base_mesh():
    """tests/golden/xarm6_base.stl welded: 1222 vertices, 2464 triangles, closed (mesh-local metres)."""
    return mesh_io.weld(*mesh_io.load_stl(GOLDEN / "xarm6_base.stl"))


@functools.lru_cache(maxsize=None)
def tblock_mesh():
    """tests/golden/tblock_paper.obj: 16 vertices, 28 triangles, closed."""
    return mesh_io.load_obj(GOLDEN / "tblock_paper.obj")


def tblock_inside(p):
    """Closed form: the T polygon (bar |x| <= 0.1, |y| <= 0.025; stem |x| <= 0.025, -0.175 <= y <= -0.025) times 0 <= z <= 0.04."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    bar = (np.abs(x) < 0.1) & (np.abs(y) < 0.025)
    stem = (np.abs(x) < 0.025) & (y > -0.175) & (y <= -0.025)
    return (bar | stem) & (z > 0) & (z < 0.04)


def unmatched_edges(faces) -> int:
    """Directed edges without their reverse: 0 for a closed, consistently oriented manifold."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = set(map(tuple, e))
    return sum((b, a) not in fwd for a, b in fwd)


def shipped_similarity():
    return np.load(GOLDEN / "scene_assets_xarm6_1.npz")["icp_transformation"].astype(np.float64)


def moved(mesh, T):
    v, f = mesh
    T = np.asarray(T, np.float64)
    return v @ T[:3, :3].T + T[:3, 3], f


# ---- the single triangle ---------------------------------------------------------------------------------------------------------------
TRIANGLE = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], np.int64))
# one point per closest-feature region, with the closed-form distance
SEVEN_REGIONS = {   # (coordinates that float32 holds exactly)
    "face": ((0.25, 0.25, 0.5), 0.5),
    "edge AB": ((0.5, -0.375, 0.5), 0.625),
    "edge BC": ((1.0, 1.0, 0.0), float(np.sqrt(0.5))),
    "edge CA": ((-0.375, 0.5, -0.5), 0.625),
    "vertex A": ((-0.375, -0.5, 0.0), 0.625),
    "vertex B": ((1.375, -0.5, 0.0), 0.625),
    "vertex C": ((-0.5, 1.375, 0.0), 0.625),
}
ZERO_AREA = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), np.array([[0, 1, 2]], np.int64))
ZERO_AREA_POINTS = np.array([[0.5, 0.375, 0.5], [3.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.5, -2.0, 0.0]])
ZERO_AREA_DISTANCE = np.array([0.625, 1.0, 1.0, 2.0])


def nan_vertex_mesh():
    """The triangle beside one with a NaN vertex, which is dropped."""
    v = np.concatenate([TRIANGLE[0], [[np.nan, 0.0, 1.0]]])
    return v, np.array([[0, 1, 3], [0, 1, 2]], np.int64)


# ---- points ------------------------------------------------------------------------------------------------------------------------------
def box_points(n, seed=3, h=(0.5, 0.3, 0.2)):
    """n points in twice the box, none within 1e-3 of a face plane (inside / outside is then decided)."""
    rng = np.random.default_rng(seed)
    h = np.asarray(h)
    p = rng.uniform(-2.0, 2.0, (4 * n + 64, 3)) * h
    ok = (np.abs(np.abs(p) - h) > 1e-3).all(axis=1)
    return p[ok][:n]


def raw_base_points():
    """Case "robot base, raw STL": rng(7), 1500 uniform in the mesh's box inflated by 0.2 x its largest extent, then 500 centroids
    of randomly drawn triangles plus normal(0, 0.01 extent).  Returns (points, extent)."""
    v, f = base_mesh()
    rng = np.random.default_rng(7)
    lo, hi = v.min(0), v.max(0)
    extent = float((hi - lo).max())
    a = rng.uniform(lo - 0.2 * extent, hi + 0.2 * extent, (1500, 3))
    t = rng.integers(0, len(f), 500)
    b = v[f[t]].mean(axis=1) + rng.normal(0.0, 0.01 * extent, (500, 3))
    return np.concatenate([a, b]), extent


def similarity_points(n=2000, seed=11, pad=0.05):
    """Case "robot base under the shipped similarity": (moved mesh, n points uniform in its box inflated by ``pad``)."""
    mesh = moved(base_mesh(), shipped_similarity())
    rng = np.random.default_rng(seed)
    lo, hi = mesh[0].min(0), mesh[0].max(0)
    return mesh, rng.uniform(lo - pad, hi + pad, (n, 3))


def surface_points(mesh, n, sigma, rng):
    """n points on randomly drawn triangles of ``mesh`` (uniform barycentric) plus normal(0, sigma): a splat's centres around a link."""
    v, f = mesh
    tri = v[f[rng.integers(0, len(f), n)]]
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    return (tri * b[:, :, None]).sum(axis=1) + rng.normal(0.0, sigma, (n, 3))


# ---- references and tolerances -----------------------------------------------------------------------------------------------------------
_REF = {}


def reference(key, points, meshes, max_distance=np.inf):
    """(float64, float32) ``mesh_query_ref.query`` results of a case, computed once per ``key`` and left unchanged."""
    if key not in _REF:
        r64, r32 = ref.query(points, meshes, max_distance, np.float64), ref.query(points, meshes, max_distance, np.float32)
        for r in (r64, r32):
            for a in r.values():
                a.setflags(write=False)
        _REF[key] = (r64, r32)
    return _REF[key]


def tolerances(points, meshes, r64, r32):
    """Per mesh (tol_d, tol_w, e32_d, e32_w): e32 = the largest float32-against-float64 difference of the NumPy reference over the
    pairs that are not culled; tol_d = 4 e32_d + 8 eps32 L, L the largest absolute finite coordinate of the case; tol_w = 4 e32_w +
    eps32 (T + 8), T the mesh's triangle count."""
    coords = [np.asarray(points, np.float64).reshape(-1)] + [np.asarray(v, np.float64).reshape(-1) for v, _ in meshes]
    allc = np.concatenate(coords)
    L = float(np.abs(allc[np.isfinite(allc)]).max()) if np.isfinite(allc).any() else 0.0
    out = []
    for m, (_, f) in enumerate(meshes):
        live = ~r64["culled"][m]
        e_d = float(np.abs(r32["distance"][m][live] - r64["distance"][m][live]).max()) if live.any() else 0.0
        e_w = float(np.abs(r32["winding"][m][live] - r64["winding"][m][live]).max()) if live.any() else 0.0
        out.append((4 * e_d + 8 * EPS32 * L, 4 * e_w + EPS32 * (len(f) + 8), e_d, e_w))
    return out
