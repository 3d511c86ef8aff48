"""CPU: the yardstick of the mesh frames before it measures anything -- the oracle's per-pixel depth limit and background
(oracle.render(zlim=, bgmap=)), the float64 mesh reference (oracle/mesh_ref.py) against a Moeller-Trumbore ray cast, and the
EXCLUSION CAPS of every fixed GPU case (tests/tools/mesh_cases.py) and every mesh fuzz seed the GPU slice runs: `stable` is
false on at most 10 % of a frame, and at least 20 % of it is stable, mesh-covered, with list entries cut off by the depth limit
and entries kept.  A case that misses a cap is replaced by another input, not given a wider cap."""
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from oracle import mesh_ref

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import oracle_fuzz as fz  # noqa: E402


# ---- the depth limit and the background map against the identity the flat-quad GPU tests rest on ----------------------------
@pytest.mark.parametrize("name", ["n2k_groups", "doorb", "dense"])
@pytest.mark.parametrize("depth_mode", [0, 1])
def test_constant_limit_is_the_filtered_scene(name, depth_mode):
    sc, cam = mc.twin(name)
    V, K, W, H = cam
    c = (0.9, 0.2, 0.1)
    dump = mc.oracle_frame(sc, cam, mc.BG, dump=True)
    vis = (dump["radii"][:, 0] > 0) & (dump["radii"][:, 1] > 0)
    d = np.float32(np.median(dump["depths"][vis]))
    keep = np.nonzero(dump["depths"] < d)[0]
    assert 0 < keep.size < vis.sum()
    got = mc.oracle_frame(sc, cam, mc.BG, zlim=np.full((H, W), d, np.float32), bgmap=np.broadcast_to(np.float32(c), (H, W, 3)),
                          depth_mode=depth_mode)
    want = mc.oracle_frame(sc, cam, c, keep=keep, depth_mode=depth_mode)
    mc.same(got, want)
    # no limit, the frame's own background as a map: the plain frame
    plain = mc.oracle_frame(sc, cam, mc.BG, depth_mode=depth_mode)
    mc.same(mc.oracle_frame(sc, cam, (0, 0, 0), zlim=np.full((H, W), np.inf, np.float32),
                            bgmap=np.broadcast_to(np.float32(mc.BG), (H, W, 3)), depth_mode=depth_mode), plain)


def test_limit_is_per_pixel():
    sc, cam = mc.twin("n2k_groups")
    V, K, W, H = cam
    dump = mc.oracle_frame(sc, cam, mc.BG, dump=True)
    d = np.float32(np.median(dump["depths"][dump["radii"][:, 0] > 0]))
    zl = np.full((H, W), np.inf, np.float32)
    zl[:, : W // 2] = d
    zl[5, W // 2 + 3] = 0.0            # behind nothing: the pixel is the background
    got = mc.oracle_frame(sc, cam, mc.BG, zlim=zl)
    left = np.zeros((H, W), bool)
    left[:, : W // 2] = True
    mc.same(got, mc.oracle_frame(sc, cam, mc.BG, keep=np.nonzero(dump["depths"] < d)[0]), where=left)
    right = ~left
    right[5, W // 2 + 3] = False
    mc.same(got, mc.oracle_frame(sc, cam, mc.BG), where=right)
    assert got["alpha"][5, W // 2 + 3, 0] == 0.0 and np.array_equal(got["rgb"][5, W // 2 + 3], np.float32(mc.BG))


# ---- the mesh reference against the ray cast ---------------------------------------------------------------------------------
def _awkward_mesh(cam, seed):
    """The coverage test's random triangles plus degenerate, off-screen, behind-the-camera and non-finite ones."""
    verts, tris = mc.random_triangles(cam, 30, seed)
    W, H = cam[2], cam[3]
    pc = np.array([[0.1, 0.1, 2.0], [0.1, 0.1, 2.0], [0.4, -0.2, 2.5],            # two equal corners
                   [0.0, 0.0, 1.0], [0.5, 0.5, 2.0], [1.0, 1.0, 3.0],            # (nearly, after rounding) collinear
                   [50.0, 40.0, 2.0], [55.0, 41.0, 2.5], [52.0, 48.0, 2.2],      # far off screen
                   [0.1, 0.2, -1.0], [0.3, -0.2, -2.0], [-0.2, 0.1, -1.5],       # behind the camera
                   [0.0, 0.0, 0.0], [0.3, 0.1, 3.0], [-0.2, 0.4, 3.0],           # a corner AT the camera centre
                   [-0.002, -0.0015, 0.005], [0.002, -0.0012, 0.02], [0.0003, 0.002, 0.015]])   # straddling the near plane closely
    extra = mc.cam_to_world(cam, pc).astype(np.float32)
    bad = np.array([[np.nan, 0, 2], [0.5, 0.2, 2], [0.1, 0.7, 2], [np.inf, 0, 2], [0.5, 0.2, 2], [0.1, 0.7, 2]], np.float32)
    v = np.concatenate([verts, extra, bad])
    n0 = len(verts)
    t = np.concatenate([tris, np.arange(n0, n0 + len(extra) + len(bad), dtype=np.int32).reshape(-1, 3)])
    return v, t


@pytest.mark.parametrize("seed,size", [(7, (80, 60)), (8, (131, 77)), (9, (33, 17))])
def test_reference_matches_ray_cast(seed, size):
    cam = mc.ring(size[0], size[1], 0.9 * size[0], yaw=25.0)
    v, t = _awkward_mesh(cam, seed)
    ref = mesh_ref.reference(v, t, (1, 1, 1), None, None, 1.0, 0.0, cam[0], cam[1], cam[2], cam[3])
    # dropped: the non-finite ones, the one with two equal corners, the one behind the camera
    assert not ref["valid"][-2:].any() and not ref["valid"][-8] and not ref["valid"][-5] and ref["valid"][:30].sum() > 20
    # the same float32 camera-frame vertices to both (two float64 formulations of one geometry)
    cv = np.where(np.isfinite(ref["camera_vertices"]), ref["camera_vertices"], np.nan)
    win, z = mc.ray_cast(cam, cv, None, camera_frame=True, want_depth=True)
    stable = ~ref["probe_differs"] & ~ref["near_second"]
    assert stable.mean() > 0.9
    assert np.array_equal(win[stable], ref["winner"][stable]), np.argwhere(stable & (win != ref["winner"]))[:5]
    hit = stable & (win >= 0)
    assert hit.sum() > 0.3 * hit.size and len(np.unique(win[hit])) > 8
    assert np.abs(z[hit] - ref["z"][hit]).max() <= 1e-9 * z[hit].max()
    assert (np.abs(z[hit] - ref["z"][hit]) <= 1e-9 * z[hit]).all()
    assert np.isinf(ref["z"][ref["winner"] < 0]).all()


def test_reference_probe_rule_matches_the_ray_casts_probes():
    """An edge 3e-4 px beside a column of pixel centres: the reference and the ray cast's own five maps call exactly those
    pixels unstable (pixel units: fx = fy = 1, u = x / z)."""
    W, H = 48, 40
    cam = (np.eye(4, dtype=np.float32), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), W, H)
    v = np.array([[10.5003, 2.25, 1], [40.25, 2.25, 1], [10.5003, 30.25, 1]], np.float32)
    ref = mesh_ref.reference(v, [[0, 1, 2]], (1, 1, 1), None, None, 1.0, 0.0, cam[0], cam[1], W, H)
    maps = [mc.ray_cast(cam, ref["camera_vertices"], None, e, camera_frame=True) for e in ((0, 0), (1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3))]
    rc_unstable = ~np.all([m == maps[0] for m in maps[1:]], axis=0)
    assert np.array_equal(rc_unstable, ref["probe_differs"])
    assert ref["probe_differs"][3:29, 10].all() and ref["probe_differs"].sum() == ref["probe_differs"][:, 10].sum() > 20
    assert (ref["winner"][3:29, 10] == -1).all() and (ref["winner"][3:20, 11] == 0).all()


def test_reference_shading():
    cam = mc.ring(64, 48, 60.0, yaw=0.0)
    rng = np.random.default_rng(4)
    for trial in range(4):
        pc = np.array([[-3.0, -2.5, 3.0], [3.5, -2.0, 4.5], [0.2, 3.0, 2.0]]) + rng.normal(0, 0.3, (3, 3))
        verts = mc.cam_to_world(cam, pc).astype(np.float32)
        col = rng.uniform(0.1, 1.0, 3)
        ka, kd = float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.3, 0.8))
        ref = mesh_ref.reference(verts, [[0, 1, 2]], col, None, None, ka, kd, cam[0], cam[1], cam[2], cam[3])
        w = verts.astype(np.float64)
        n = np.cross(w[1] - w[0], w[2] - w[0])
        n /= np.linalg.norm(n)
        Vd = np.asarray(cam[0], np.float64)
        campos = -Vd[:3, :3].T @ Vd[:3, 3]
        d = w.mean(0) - campos
        d /= np.linalg.norm(d)
        m = np.clip(col * (ka + kd * abs(n @ d)), 0, 1)
        assert np.abs(ref["tri_color"][0] - m).max() < 1e-6          # (float32 ka, kd, campos and colour)
        inside = ref["winner"] == 0
        assert inside.sum() > 100 and np.array_equal(ref["color"][inside], np.broadcast_to(ref["tri_color"][0], (int(inside.sum()), 3)))
        zlim, bgmap = mesh_ref.frame_inputs(ref, mc.BG)
        assert np.array_equal(bgmap[~inside], np.broadcast_to(np.float32(mc.BG), (int((~inside).sum()), 3))) and np.isinf(zlim[~inside]).all()
        assert np.array_equal(zlim[inside], ref["z"][inside].astype(np.float32))


def test_posed_vertices_follow_the_oracles_means():
    """oracle.pose_points is the chain project_one moves the means with: a Gaussian at a vertex has the vertex's camera depth."""
    sc, cam = mc.twin("n2k_groups")
    V, K, W, H = cam
    dump = mc.oracle_frame(sc, cam, mc.BG, dump=True)
    _, camv, _ = oracle.pose_points(sc["means"], V, sc["gid"], sc["Rt"])
    vis = dump["radii"][:, 0] > 0
    assert vis.sum() > 500 and np.array_equal(camv[vis, 2], dump["depths"][vis])


# ---- the caps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.FIXED_CASES))
def test_fixed_case_caps(name):
    case = mc.FIXED_CASES[name]()
    for view in range(len(case["cams"])):
        e = mc.expect(name, case, view)
    if name.startswith("size_"):      # mesh edges inside the ragged tiles: covered and uncovered pixels in the last tile column and row
        W, H = case["cams"][0][2], case["cams"][0][3]
        win = e["ref"]["winner"]
        for sl in (win[:, 16 * (W // 16):], win[16 * (H // 16):, :]):
            assert (sl >= 0).any() and ((sl < 0).any() or sl.shape[0] * sl.shape[1] <= 33)
        assert (win[:, -1] >= 0).any() or (win[:, 16 * (W // 16):] < 0).any()


def test_a_tilted_plane_drives_both_batches():
    """Across the tilted-plane cases at least one compared tile has a list longer than 512 entries with stable pixels cut inside
    its first 256-entry batch and stable pixels cut after it."""
    hits = {n: mc.expected(mc.case_plane(n))["tiles_cut_in_both_batches"] for n in ("dense", "cfg3")}
    assert hits["dense"] >= 1, hits


def test_full_hd_case_scans_eight_rounds():
    case = mc.case_1080p()
    W, H = case["cams"][0][2], case["cams"][0][3]
    assert ((W + 15) // 16) * ((H + 15) // 16) == 8160 and 2000 <= len(case["mesh"]["tris"]) <= 5000
    assert 15000 <= case["sc"]["means"].shape[0] <= 25000


def test_mesh_fuzz_seeds():
    """The 40 seeds of the GPU slice: from 0 upward, skipping those whose excluded share exceeds 10 %; at most 5 of the first 45
    are skipped.  draw_mesh_case leaves draw_case's draw alone."""
    seeds, skipped = [], []
    seed = 0
    while len(seeds) < 40:
        c = fz.draw_mesh_case(seed)
        (seeds if fz.mesh_excluded_share(c) <= fz.MESH_MAX_EXCLUDED else skipped).append(seed)
        seed += 1
    assert tuple(seeds) == tuple(fz.MESH_FUZZ_SEEDS), (seeds, skipped)
    assert len([s for s in skipped if s < 45]) <= 5
    cases = [fz.draw_mesh_case(s) for s in seeds if s % 8 == 1]
    for c in cases:
        b = fz.draw_case(c["seed"])
        assert np.array_equal(c["scene"].means, b["scene"].means, equal_nan=True) and (c["W"], c["H"], c["deg"]) == (b["W"], b["H"], b["deg"])
        assert 1 <= len(c["mesh"]["tris"]) <= 60 and c["entry"] in ("single", "batch", "posed", "host")
    drawn = [fz.draw_mesh_case(s) for s in seeds]
    assert any(c["mesh"]["poisoned_vertices"] for c in drawn) and any(c["poisoned"] for c in drawn)
    assert any(c["mesh"]["groups"] is not None for c in drawn)


@pytest.mark.parametrize("seed", fz.MESH_SEEDS_VERTEX_AT_1E30)
def test_named_mesh_seeds_stay_within_the_exclusion_cap(seed):
    assert fz.mesh_excluded_share(fz.draw_mesh_case(seed)) <= fz.MESH_MAX_EXCLUDED
