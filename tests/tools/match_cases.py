"""Clouds, transforms and registration cases shared by the point-matching tests (tests/test_register_cpu.py,
tests/test_gpu_m_match.py) and tools/match_probe.py.  Every case is drawn once (``functools.lru_cache``) and its arrays are left
unchanged; the reference loops of the two registration cases run once per process."""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import match_ref as mr  # noqa: E402
import mesh_query_cases as qc  # noqa: E402

from sim_a_splat_amd import mesh_io  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
THRESHOLD = 0.2   # the reference's correspondence distance (match_splat.py:190)


def axis_angle(axis, degrees) -> np.ndarray:
    """Rodrigues' rotation about ``axis`` (normalised here)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def similarity(scale, axis, degrees, translation) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3] = scale * axis_angle(axis, degrees)
    T[:3, 3] = translation
    return T


TRUTH = similarity(0.93, (0.3, -0.5, 0.8), 12.0, (0.21, -0.13, 0.34))   # scale 0.93, 12 degrees about a skew axis, a translation


def apply(T, p) -> np.ndarray:
    return np.asarray(p, np.float64).reshape(-1, 3) @ np.asarray(T)[:3, :3].T + np.asarray(T)[:3, 3]


def perturbed(T, degrees, shift, scale, about) -> np.ndarray:
    """``T`` followed by a small similarity about the point ``about``: rotation of ``degrees`` about (1, -1, 1), ``scale``, and a
    translation of (shift, -shift, shift)."""
    P = similarity(scale, (1.0, -1.0, 1.0), degrees, (shift, -shift, shift))
    C, Ci = np.eye(4), np.eye(4)
    C[:3, 3], Ci[:3, 3] = about, -np.asarray(about)
    return C @ P @ Ci @ T


def clutter(true_points, n, rng, clearance=THRESHOLD + 0.05) -> np.ndarray:
    """n float32 points in the true points' box inflated by 0.6, every one further than ``clearance`` from every true point."""
    lo, hi = true_points.min(0) - 0.6, true_points.max(0) + 0.6
    out = np.zeros((0, 3), np.float32)
    while len(out) < n:
        c = rng.uniform(lo, hi, (4 * n, 3)).astype(np.float32)
        d2 = ((c.astype(np.float64)[:, None, :] - true_points.astype(np.float64)[None, :, :]) ** 2).sum(-1).min(1)
        out = np.concatenate([out, c[d2 > clearance ** 2]])
    return out[:n]


def drawn(S, T, seed, spread=1.0) -> tuple:
    """(source [S,3], target [T,3]) float32, normal(0, spread)."""
    rng = np.random.default_rng(seed)
    return rng.normal(0, spread, (S, 3)).astype(np.float32), rng.normal(0, spread, (T, 3)).astype(np.float32)


def coordinate_scale(*arrays) -> float:
    """L: the largest absolute finite coordinate."""
    a = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in arrays])
    a = a[np.isfinite(a)]
    return float(np.abs(a).max()) if a.size else 0.0


# ---- the two registration cases ---------------------------------------------------------------------------------------------------------
def _case(n_source, n_clutter, sigma, seed, perturbation):
    v, f = qc.base_mesh()
    rng = np.random.default_rng(seed)
    source = mesh_io.sample_surface(v, f, n_source, seed=seed).astype(np.float32)
    true = apply(TRUTH, source)
    if sigma:
        true = true + rng.normal(0.0, sigma, true.shape)
    true = true.astype(np.float32)
    target = np.concatenate([true, clutter(true, n_clutter, rng)])
    init = perturbed(TRUTH, *perturbation, about=true.astype(np.float64).mean(0))
    for a in (source, target, init):
        a.setflags(write=False)
    return {"source": source, "target": target, "init": init, "n_true": n_source, "L": coordinate_scale(source, target)}


@functools.lru_cache(maxsize=None)
def clean_case():
    """2 000 samples of the welded base mesh; the target is, in this index order, the same points under TRUTH rounded to float32,
    then 1 000 clutter points further than 0.2 from every true point.  The guess is TRUTH perturbed by 3 degrees, 2 % of scale and
    (0.01, -0.01, 0.01) about the target's centre: the float64 loop reaches the limits in 10 iterations (test_register_cpu.py)."""
    return _case(2000, 1000, 0.0, 5, (3.0, 0.01, 1.02))


@functools.lru_cache(maxsize=None)
def noisy_case():
    """Another sample (700), the true points moved by normal(0, 0.003), 300 clutter points; the same perturbation."""
    return _case(700, 300, 0.003, 9, (3.0, 0.01, 1.02))


@functools.lru_cache(maxsize=None)
def loops(which):
    """(float32 loop, float64 loop, e32) of a case through ``match_ref.icp``: e32 = |T_match32 - T_match64|_max, what float32
    matching costs the registration -- the yardstick of the GPU's free loop."""
    c = {"clean": clean_case, "noisy": noisy_case}[which]()
    l32 = mr.icp(c["source"], c["target"], c["init"], mr.match32, THRESHOLD)
    l64 = mr.icp(c["source"], c["target"], c["init"], mr.match64, THRESHOLD)
    return l32, l64, float(np.abs(l32["T"] - l64["T"]).max())


# ---- the end-to-end scene: the T block and the robot's base in a splat -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_case():
    """The two links of tests/test_gpu_l_mesh_query.py::test_link_masks_end_to_end -- the T block shifted by 0.35 along x and the
    base, both under the shipped similarity -- as a registration problem: ``means`` = 1 500 Gaussian centres around each placed link
    (normal(0, 0.006)) and 1 000 background centres behind them; ``source`` = 1 500 samples of the two unplaced meshes as one surface;
    the guess is the shipped similarity perturbed by 2 degrees, 1 % of scale and 0.008."""
    rng = np.random.default_rng(31)
    icp = qc.shipped_similarity()
    shift = np.eye(4)
    shift[:3, 3] = (0.35, 0.0, 0.0)
    meshes, local = [qc.tblock_mesh(), qc.base_mesh()], [shift, np.eye(4)]
    placed = [qc.moved(m, icp @ S) for m, S in zip(meshes, local)]
    c0, c1 = placed[0][0].mean(0), placed[1][0].mean(0)
    lo, hi = np.minimum(c0, c1) - 0.4, np.maximum(c0, c1) + 0.4
    lo[2] = max(placed[0][0][:, 2].max(), placed[1][0][:, 2].max()) + 0.1      # the background lies behind both links (+z)
    hi[2] = lo[2] + 0.5
    means = np.concatenate([qc.surface_points(placed[0], 1500, 0.006, rng), qc.surface_points(placed[1], 1500, 0.006, rng),
                            rng.uniform(lo, hi, (1000, 3))]).astype(np.float32)
    unplaced = [qc.moved(m, S) for m, S in zip(meshes, local)]
    verts = np.concatenate([unplaced[0][0], unplaced[1][0]])
    faces = np.concatenate([unplaced[0][1], unplaced[1][1] + len(unplaced[0][0])])
    source = mesh_io.sample_surface(verts, faces, 1500, seed=2).astype(np.float32)
    init = perturbed(icp, 2.0, 0.008, 1.01, about=0.5 * (c0 + c1))
    return {"means": means, "source": source, "init": init, "truth": icp, "meshes": meshes, "local": local, "vertices": verts,
            "centres": (c0, c1)}
