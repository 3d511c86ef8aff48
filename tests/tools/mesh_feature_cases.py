"""Shared by test_gpu_i_mesh_features.py and test_mesh_features_cpu.py: what a frame with meshes must deliver as feature channels,
labels and scene depth ("Feature channels over meshes" and "Scene depth"), from oracle.mesh_ref and the depth-limited
oracle alone.  Everything here runs on the CPU and builds on tests/tools/mesh_cases.py, whose cases and stability caps carry over:
stability does not depend on colours.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_cases as mc  # noqa: E402
import oracle_fuzz as fz  # noqa: E402
from obs_fuzz import label_rule  # noqa: E402

EPS32 = 2.0 ** -24
CHANNELS = (3, 9, 24)                    # one chunk of 8, a partial second chunk, three chunks
CASES = {"entry_points": mc.case_entry_points, "size_17x33": lambda: mc.case_size(17, 33), "soup": mc.case_soup, "tblock": mc.case_tblock}
DEPTH_MOVES_TOLERANCES = 1000.0          # "the depth moved": further than this many tolerances from the splat-only depth ...
DEPTH_MOVES_MIN_SHARE = 0.20             # ... on at least this share of the frame, for the cases below
DEPTH_MOVES_CASES = ("entry_points", "size_17x33", "soup")
LABEL_MIN_SHARE = 0.20
MAX_REL_TOL = 1e-4                       # the scene-depth tolerance stays below this share of D_ref on every compared pixel
# oracle_fuzz.draw_mesh_case seeds that go through the recolouring and scene-depth checks: twenty, from 0 upward, skipping those
# whose reference does not meet the caps (seeds 3 and 11: triangles seen at so grazing an angle that kappa, and with it the depth
# tolerance, exceeds MAX_REL_TOL of the depth).  tests/test_mesh_features_cpu.py recomputes the list.  The skipped seeds still go
# through the recolouring identity, which compares GPU frames on every pixel and needs neither stability nor a tolerance.
DRAWN_SEEDS_SKIPPED = (3, 11)
DRAWN_SEEDS = tuple(s for s in range(22) if s not in DRAWN_SEEDS_SKIPPED)


def draw_features(case, C, seed):
    """(f [n,C], fm [T,C], fbg [C]) in [0,1]."""
    rng = np.random.default_rng(seed)
    n, T = case["sc"]["means"].shape[0], len(case["mesh"]["tris"])
    return (rng.uniform(0, 1, size=(n, C)).astype(np.float32), rng.uniform(0, 1, size=(T, C)).astype(np.float32),
            rng.uniform(0, 1, size=C).astype(np.float32))


def triples(C):
    return sorted({0, C // 2 - 1 if C >= 6 else 0, C - 3})   # the first, one across a chunk boundary (C = 24: 11..13), the last


def recoloured(case, col, mcol, bg):
    """The case with its Gaussians coloured `col [n,3]` (final RGB), its triangles `mcol [T,3]` unshaded, background `bg [3]`."""
    sc = dict(case["sc"], colors=np.ascontiguousarray(col, dtype=np.float32), sh=-1)
    m = dict(case["mesh"], cols=np.ascontiguousarray(mcol, dtype=np.float32), ka=1.0, kd=0.0)
    return dict(case, sc=sc, mesh=m, bg=tuple(float(v) for v in bg))


def oracle_recoloured_rgb(case, e, view, col, mcol, bg):
    """rgb of the recoloured case from the depth-limited oracle: colors = col, sh_degree = -1, zlim of the case's reference
    (`e`: mc.expected of the case), bgmap = where(covered, mcol[winner], bg)."""
    w = e["ref"]["winner"]
    bgmap = np.where((w >= 0)[..., None], np.asarray(mcol, np.float32)[np.maximum(w, 0)], np.asarray(bg, np.float32).reshape(1, 1, 3))
    rc = recoloured(case, col, mcol, bg)
    return mc.oracle_frame(rc["sc"], case["cams"][view], rc["bg"], Rt=mc.view_poses(case, view), zlim=e["zlim"],
                           bgmap=np.ascontiguousarray(bgmap, dtype=np.float32))["rgb"]


# ---- scene depth (SAS_MESH_SURFACE) ------------------------------------------------------------------------------------------
def surface_reference(e):
    """What alpha and depth of a frame rendered with the flag are held to, from mc.expected's `e` (depth_mode 0).

    On a covered pixel the kernel closes the depth chain on the triangle: D = fma(z_m, T, d), alpha = 1.  The reference, float64,
    from the depth-limited oracle's outputs (ED = d / max(alpha, 1e-10), alpha) and the mesh reference's z:
        D_ref = ED * alpha + (1 - alpha) * z_m
        tol   = (delta + 4 * 2^-24) * max(z_m, D_ref)
    delta = 16 * 2^-24 * kappa is oracle/mesh_ref.py's own bound on the kernel's float32 z_m.  Four further half-ulps: the
    oracle's division ED = d / alpha, undone here by a product (ED * alpha is d up to 2^-24 relative); T = 1 - alpha taken back
    from the rounded alpha (2^-24 ABSOLUTE, times z_m: hence max(z_m, .)); the product z_m * T and the final rounding of the fma
    (one rounding in the kernel, counted as two).  Derived, not measured.
    Returns D_ref, tol [H,W] float64 (NaN where no triangle), covered, and the masks the checks run on."""
    ref, frame, stable = e["ref"], e["frame"], e["stable"]
    covered = ref["winner"] >= 0
    a = frame["alpha"][..., 0].astype(np.float64)
    ed = frame["depth"][..., 0].astype(np.float64)
    z = np.where(covered, ref["z"], np.nan)
    with np.errstate(invalid="ignore"):
        D = ed * a + (1.0 - a) * z
        tol = (ref["delta"] + 4.0 * EPS32) * np.maximum(z, D)
        moved = covered & stable & (np.abs(D - ed) > DEPTH_MOVES_TOLERANCES * tol)
    return dict(D=D, tol=tol, covered=covered, on=stable & covered, off=stable & ~covered, moved_share=float(moved.mean()),
                splat_depth=ed)


def check_surface(got, e, s=None):
    """Differences between a frame rendered with the flag (`got`: alpha, depth [H,W,1]) and the reference; [] when none."""
    s = surface_reference(e) if s is None else s
    ga, gd = np.asarray(got["alpha"])[..., 0], np.asarray(got["depth"])[..., 0]
    diffs = []
    for k, g in (("alpha", ga), ("depth", gd)):
        x, y = g[s["off"]], np.asarray(e["frame"][k])[..., 0][s["off"]]
        if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            diffs.append(f"{k}: {int((x != y).sum())} stable uncovered pixels differ from the oracle frame")
    if not np.array_equal(ga[s["on"]], np.ones(int(s["on"].sum()), np.float32)):
        diffs.append(f"alpha: {int((ga[s['on']] != 1).sum())} stable covered pixels are not 1.0f")
    err = np.abs(gd[s["on"]].astype(np.float64) - s["D"][s["on"]])
    bad = ~(err <= s["tol"][s["on"]])
    if bad.any():
        diffs.append(f"depth: {int(bad.sum())} stable covered pixels beyond tol, worst {float((err / s['tol'][s['on']]).max()):.2f} tolerances")
    return diffs


def moved_share(with_flag, without_flag, s):
    """Share of the frame on which the delivered depth lies more than DEPTH_MOVES_TOLERANCES tolerances from the splat-only one."""
    a, b = np.asarray(with_flag)[..., 0].astype(np.float64), np.asarray(without_flag)[..., 0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return float((s["on"] & (np.abs(a - b) > DEPTH_MOVES_TOLERANCES * s["tol"])).mean())


# ---- labels ----------------------------------------------------------------------------------------------------------------------
labels_of = label_rule   # rasterizer.group_labels in NumPy (obs_fuzz.py: the one text of the rule the label references share)


def case_labels():
    """The tilted plane of plane_n2k_groups on a pose row of its own: the scene's groups keep their rows and poses, the plane
    takes row G (identity), its vertices in world coordinates."""
    sc, cam = mc.twin("n2k_groups")
    z = mc.visible_depths(sc, cam)
    world, tris = mc.tilted_quad(cam, float(np.quantile(z, 0.10)), float(np.quantile(z, 0.90)))
    G = sc["G"]
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(1, 12).astype(np.float32)
    sc = dict(sc, G=G + 1, Rt=np.concatenate([np.asarray(sc["Rt"], np.float32).reshape(G, 12), eye]))
    cols = np.array([mc.C_PLANE, (0.2, 0.8, 0.3)], np.float32)
    return dict(sc=sc, cams=[cam], mesh=mc._mesh(world, tris, cols, [G, G]), bg=mc.BG, poses=None)


def expected_labels(case, e, view=0, min_alpha=0.5):
    """Labels, weights [H,W,G] and the scene's alpha from the oracle: one-hot rows composited three at a time (zero background,
    the triangle's one-hot row where one shows), alpha 1 on a covered pixel."""
    sc, m = case["sc"], case["mesh"]
    G = sc["G"]
    pad = 3 * ((G + 2) // 3)
    f = np.zeros((sc["means"].shape[0], pad), np.float32)
    f[np.arange(f.shape[0]), np.asarray(sc["gid"], np.int64)] = 1.0
    fm = np.zeros((len(m["tris"]), pad), np.float32)
    fm[np.arange(fm.shape[0]), np.asarray(m["groups"], np.int64)] = 1.0
    w = np.concatenate([oracle_recoloured_rgb(case, e, view, f[:, o:o + 3], fm[:, o:o + 3], (0.0, 0.0, 0.0)) for o in range(0, pad, 3)], -1)[..., :G]
    alpha = np.where(e["ref"]["winner"] >= 0, np.float32(1.0), e["frame"]["alpha"][..., 0])
    return dict(labels=labels_of(w, alpha, min_alpha), weights=w, alpha=alpha)


# ---- drawn cases -------------------------------------------------------------------------------------------------------------------
def drawn_case(seed):
    """oracle_fuzz.draw_mesh_case(seed) as a case of mesh_cases' form (the tests take its first view)."""
    return fz.as_case(fz.draw_mesh_case(seed))
