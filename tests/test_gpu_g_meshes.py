"""GPU: triangle meshes composited into the frames (sas_scene_meshes; DESIGN.md 3, "Meshes").

A mesh pixel hides every splat at or behind its depth and takes the background's place.  So a quad that covers the frame at
a depth d, flat-coloured c, renders exactly the oracle's frame of the scene filtered to the Gaussians in front of d with
background c -- asserted bit for bit, with d in a gap of the GPU's own Gaussian depths.  Coverage (which triangle wins a
pixel) is held to a float64 ray cast, away from edges.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError
from sim_a_splat_amd.synthetic import make_scene

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
from mesh_cases import (BG, OUTS, DrawMsg as _DrawMsg, cam_to_world as _cam_to_world, colours as _colours, config3_window as _config3_window,  # noqa: E402
                        full_quad as _full_quad, oracle_frame as _oracle, random_triangles as _random_triangles, ray_cast as _ray_cast,
                        ring as _ring, same as _same, screen_quad as _screen_quad, stable_ref as _stable_ref, synthetic as _synthetic,
                        to_numpy as _np, twin as _twin, upload as _upload)

pytestmark = pytest.mark.gpu

def _frame(r, cam, bg, want=OUTS):
    V, K, W, H = cam
    return _np(r.render(V, K, W, H, bg, want=want))


def _visible_depths(r):
    p = r.read_projection()
    return np.sort(p["depths"][(p["radii"][:, 0] > 0) & (p["radii"][:, 1] > 0)].astype(np.float64)), p["depths"]


def _gap_depth(r, lo_q=0.45):
    """A depth in a gap (1e-3 relative or wider) of the GPU's own depths of the visible Gaussians, near their quantile lo_q;
    None when the scene has no such gap."""
    z, _ = _visible_depths(r)
    assert z.size > 10
    gaps = (z[1:] - z[:-1]) / z[1:]
    ok = np.nonzero(gaps > 2e-3)[0]
    if ok.size == 0:
        return None
    i = int(ok[np.argmin(np.abs(ok - lo_q * z.size))])
    return float(0.5 * (z[i] + z[i + 1]))


def _subset(sc, keep):
    out = dict(sc)
    for k in ("means", "op", "colors", "quats", "scales", "cov6", "gid"):
        if sc[k] is not None:
            out[k] = np.asarray(sc[k])[keep]
    return out


def _scene_with_gap(r, sc, cam):
    """Upload sc and return (scene, d): d in a gap of its depths.  A dense scene without one (config 3) gets a gap carved
    out: the Gaussians within 2e-3 relative of the median depth are left out."""
    _upload(r, sc)
    _frame(r, cam, BG)
    d = _gap_depth(r)
    if d is None:
        z, depths = _visible_depths(r)
        d = float(z[z.size // 2])
        sc = _subset(sc, np.nonzero(np.abs(depths.astype(np.float64) - d) > 2e-3 * d)[0])
        _upload(r, sc)
        _frame(r, cam, BG)
        assert _gap_depth(r) is not None
    return sc, d


C = (0.9, 0.2, 0.1)


# ---- (a) a quad behind every Gaussian is the background ---------------------------------------------------------------
def test_a_quad_behind_everything_is_background():
    sc = _synthetic(3000, 11, 0.03, n_groups=3)
    cam = _ring()
    r = Rasterizer(0)
    try:
        _upload(r, sc)
        _frame(r, cam, BG)
        far = float(r.read_projection()["depths"].max()) * 4 + 10
        v, t = _full_quad(cam, far)
        ref = _oracle(sc, cam, C)
        r.upload_meshes(v, t, C, groups=None, ambient=1.0, diffuse=0.0)
        _same(_frame(r, cam, BG), ref)
        V, K, W, H = cam
        Vs, Ks = np.stack([V, V]), np.stack([K, K])
        b = _np(r.render_batch(Vs, Ks, W, H, BG, want=("rgb", "alpha", "depth", "rgb8")))
        for k in range(2):
            _same({q: b[q][k] for q in b}, ref)
        hb = r.render_batch_host(Vs, Ks, W, H, BG)
        for k in range(2):
            assert np.array_equal(np.asarray(hb)[k], ref["rgb8"])
        sets = np.stack([sc["Rt"], sc["Rt"]]).astype(np.float32)
        bp = _np(r.render_batch(Vs, Ks, W, H, BG, want=("rgb", "rgb8"), pose_sets=sets, pose_set=[0, 1]))
        for k in range(2):
            assert np.array_equal(bp["rgb8"][k], ref["rgb8"]) and np.array_equal(bp["rgb"][k].view(np.uint8), ref["rgb"].view(np.uint8))
    finally:
        r.close()


def test_a_cameras_host():
    sc = _synthetic(2000, 5, 0.03)
    r = Rasterizer(0)
    try:
        _upload(r, sc)
        W, H, fov = 96, 64, 1.1
        wxyz = np.array([[0.0, 0.0, 1.0, 0.0]], np.float64)    # 180 degrees about y: looking at the scene from +z
        pos = np.array([[0.1, 0.05, 3.0]], np.float64)
        Vs = np.zeros((1, 16), np.float32)
        Ks = np.zeros((1, 9), np.float32)
        L = _capi.lib()
        assert L.sas_camera_matrices(1, wxyz.ctypes.data, pos.ctypes.data, fov, W, H, Vs.ctypes.data, Ks.ctypes.data) == 0
        cam = (Vs[0].reshape(4, 4), Ks[0].reshape(3, 3), W, H)
        plain = np.asarray(r.render_cameras_host(wxyz, pos, fov, W, H, BG))[0]
        ref0 = _oracle(sc, cam, BG)
        assert np.array_equal(plain, ref0["rgb8"])
        v, t = _full_quad(cam, 100.0)
        r.upload_meshes(v, t, C, ambient=1.0, diffuse=0.0)
        got = np.asarray(r.render_cameras_host(wxyz, pos, fov, W, H, BG))[0]
        assert np.array_equal(got, _oracle(sc, cam, C)["rgb8"])
    finally:
        r.close()


# ---- (b) a quad at a depth inside the scene: the oracle's frame of the Gaussians in front of it -------------------------
CASES_B = ["n2k_groups", "doorb", "cfg3"]


def _case(name):
    return _config3_window() if name == "cfg3" else _twin(name)


@pytest.mark.parametrize("name", CASES_B)
def test_b_quad_at_depth_is_filtered_scene(name):
    sc, cam = _case(name)
    r = Rasterizer(0)
    try:
        sc, d = _scene_with_gap(r, sc, cam)
        depths = r.read_projection()["depths"]
        v, t = _full_quad(cam, d)
        r.upload_meshes(v, t, C, ambient=1.0, diffuse=0.0)
        got = _frame(r, cam, BG)
        keep = np.nonzero(depths < d)[0]
        ref = _oracle(sc, cam, C, keep=keep)
        _same(got, ref)
        assert 0 < keep.size < sc["means"].shape[0]
    finally:
        r.close()


# ---- (c) the same quad over the left half only -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n2k_groups", "doorb"])
def test_c_half_frame_quad(name):
    sc, cam = _case(name)
    W, H = cam[2], cam[3]
    r = Rasterizer(0)
    try:
        sc, d = _scene_with_gap(r, sc, cam)
        plain = _frame(r, cam, BG)
        v, t = _full_quad(cam, d)
        r.upload_meshes(v, t, C, ambient=1.0, diffuse=0.0)
        full = _frame(r, cam, BG)
        v, t = _screen_quad(cam, d, -20.0, W / 2, -20.0, H + 20.0)
        r.upload_meshes(v, t, C, ambient=1.0, diffuse=0.0)
        half = _frame(r, cam, BG)
        left = np.zeros((H, W), bool)
        left[:, : W // 2] = True
        _same(half, full, where=left)
        _same(half, plain, where=~left)
    finally:
        r.close()


# ---- (d) coverage against a float64 ray cast ------------------------------------------------------------------------------
def _winner_map(rgb8, cols8):
    key = rgb8.astype(np.int64) @ np.array([1, 256, 65536])
    lut = {int(c @ np.array([1, 256, 65536])): i for i, c in enumerate(cols8.astype(np.int64))}
    return np.vectorize(lambda k: lut.get(int(k), -1))(key)


def _empty_scene_rasterizer(n_groups=0):
    r = Rasterizer(0)
    z = np.zeros((0, 3), np.float32)
    r.upload(z, np.zeros(0, np.float32), z, quats=np.zeros((0, 4), np.float32), scales=z, sh_degree=-1,
             group_id=np.zeros(0, np.uint8) if n_groups else None, n_groups=n_groups)
    return r


def test_d_coverage_matches_ray_cast():
    cam = _ring(80, 60, 70.0, yaw=25.0)
    verts, tris = _random_triangles(cam, 30, 7)
    cols = _colours(len(tris), 3)
    r = _empty_scene_rasterizer()
    try:
        r.upload_meshes(verts, tris, cols / 255.0, ambient=1.0, diffuse=0.0)
        got = _frame(r, cam, (0.0, 0.0, 0.0), want=("rgb8",))["rgb8"]
        win = _winner_map(got, cols)
        bg = np.all(got == 0, -1)
        win[bg] = -1
        ref, stable = _stable_ref(cam, verts.astype(np.float64), tris)
        assert stable.mean() > 0.9
        bad = (win != ref) & stable
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
        assert len(np.unique(ref[stable])) > 10     # many triangles are seen
    finally:
        r.close()


# ---- (e) shading --------------------------------------------------------------------------------------------------------
def test_e_shading_within_one_lsb():
    cam = _ring(64, 48, 60.0, yaw=0.0)
    rng = np.random.default_rng(4)
    r = _empty_scene_rasterizer()
    try:
        for trial in range(4):
            pc = np.array([[-3.0, -2.5, 3.0], [3.5, -2.0, 4.5], [0.2, 3.0, 2.0]]) + rng.normal(0, 0.3, (3, 3))
            verts = _cam_to_world(cam, pc).astype(np.float32)
            col = rng.uniform(0.1, 1.0, 3)
            ka, kd = float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.3, 0.8))
            r.upload_meshes(verts, [[0, 1, 2]], col, ambient=ka, diffuse=kd)
            got = _frame(r, cam, (0.0, 0.0, 0.0), want=("rgb8",))["rgb8"].astype(int)
            w = verts.astype(np.float64)
            n = np.cross(w[1] - w[0], w[2] - w[0])
            n /= np.linalg.norm(n)
            Vd = np.asarray(cam[0], np.float64)
            campos = -Vd[:3, :3].T @ Vd[:3, 3]
            d = w.mean(0) - campos
            d /= np.linalg.norm(d)
            m = np.clip(col * (ka + kd * abs(n @ d)), 0, 1)
            want = np.floor(m * 255 + 0.5).astype(int)
            ref, stable = _stable_ref(cam, w, np.array([[0, 1, 2]]))
            inside = (ref == 0) & stable
            assert inside.sum() > 100
            assert np.abs(got[inside] - want).max() <= 1
            assert (got[(ref == -1) & stable] == 0).all()
    finally:
        r.close()


# ---- (f) posed meshes --------------------------------------------------------------------------------------------------
def test_f_posed_group_and_pose_sets():
    sc = _synthetic(2000, 21, 0.02, n_groups=3)
    cam = _ring(96, 64, 90.0, yaw=10.0)
    r = Rasterizer(0)
    try:
        _upload(r, sc)
        # a triangle near the camera (in front of every Gaussian) on group 2
        pc = np.array([[-0.5, -0.4, 1.2], [0.6, -0.3, 1.4], [0.0, 0.5, 1.0]])
        Rt = sc["Rt"].reshape(-1, 3, 4).astype(np.float64)
        world = _cam_to_world(cam, pc)
        local = (world - Rt[2][:, 3]) @ Rt[2][:, :3]            # pose^-1: the mesh-local vertices
        verts = local.astype(np.float32)
        r.upload_meshes(verts, [[0, 1, 2]], (1.0, 0.0, 1.0), groups=[2], ambient=1.0, diffuse=0.0)
        got = _frame(r, cam, BG, want=("rgb8",))["rgb8"]
        mask = np.all(got == np.array([255, 0, 255]), -1)
        posed = verts.astype(np.float64) @ Rt[2][:, :3].T + Rt[2][:, 3]
        ref, stable = _stable_ref(cam, posed, np.array([[0, 1, 2]]))
        assert (ref[stable] == 0).sum() > 200
        assert np.array_equal(mask[stable & (ref == 0)], np.ones(int((stable & (ref == 0)).sum()), bool))
        assert not mask[stable & (ref == -1)].any()
        # pose sets: each view shows its own set's mesh pose, bit-equal to a single render with it
        R2 = sc["Rt"].copy().reshape(-1, 12)
        R2[2, 3] += 0.15
        R2[2, 7] -= 0.1
        sets = np.stack([sc["Rt"].reshape(-1, 12), R2]).astype(np.float32)
        V, K, W, H = cam
        b = _np(r.render_batch(np.stack([V, V, V]), np.stack([K, K, K]), W, H, BG, want=("rgb", "rgb8"), pose_sets=sets,
                               pose_set=[1, 0, 1]))
        singles = []
        for s in range(2):
            r.set_group_poses(sets[s])
            singles.append(_frame(r, cam, BG, want=("rgb", "rgb8")))
        assert not np.array_equal(singles[0]["rgb8"], singles[1]["rgb8"])
        for k, s in enumerate([1, 0, 1]):
            _same({q: b[q][k] for q in b}, singles[s], keys=("rgb", "rgb8"))
        hb = np.asarray(r.render_batch_host(np.stack([V, V, V]), np.stack([K, K, K]), W, H, BG, pose_sets=sets, pose_set=[1, 0, 1]))
        for k, s in enumerate([1, 0, 1]):
            assert np.array_equal(hb[k], singles[s]["rgb8"])
    finally:
        r.close()


# ---- (h) lifetime, async, status codes, determinism -----------------------------------------------------------------------
def test_h_clear_and_new_upload_forget_meshes():
    sc = _synthetic(3000, 2, 0.03)
    cam = _ring()
    r = Rasterizer(0)
    try:
        _upload(r, sc)
        plain = _frame(r, cam, BG)
        v, t = _full_quad(cam, 3.0)
        r.upload_meshes(v, t, C)
        assert not np.array_equal(_frame(r, cam, BG)["rgb8"], plain["rgb8"])
        r.clear_meshes()
        _same(_frame(r, cam, BG), plain)
        r.upload_meshes(v, t, C)
        _upload(r, sc)
        _same(_frame(r, cam, BG), plain)
    finally:
        r.close()


def test_h_async_frame_keeps_its_pose():
    sc = _synthetic(2000, 8, 0.02, n_groups=2)
    cam = _ring()
    V, K, W, H = cam
    r = Rasterizer(0)
    try:
        _upload(r, sc)
        v, t = _screen_quad(cam, 2.5, 10, 60, 10, 50)
        r.upload_meshes(v, t, C, groups=[1, 1])
        A = sc["Rt"].reshape(-1, 12).astype(np.float32)
        B = A.copy()
        B[1, 3] += 0.3
        r.set_group_poses(A)
        ref = _frame(r, cam, BG, want=("rgb",))
        out = r.render(V, K, W, H, BG, want=("rgb",), block=False)
        r.set_group_poses(B)
        other = r.render(V, K, W, H, BG, want=("rgb",), block=False)
        r.wait()
        torch.cuda.synchronize()
        assert np.array_equal(out["rgb"].cpu().numpy().view(np.uint8), ref["rgb"].view(np.uint8))
        assert not np.array_equal(other["rgb"].cpu().numpy(), ref["rgb"])
    finally:
        r.close()


def test_h_status_codes():
    L = _capi.lib()
    r = Rasterizer(0)
    try:
        v = np.zeros((3, 3), np.float32)
        t = np.array([[0, 1, 2]], np.int32)
        c = np.ones((1, 3), np.float32)
        g = np.zeros(1, np.uint8)
        p = lambda a: a.ctypes.data
        assert L.sas_scene_meshes(r._ctx, 3, p(v), 1, p(t), p(c), p(g), 0.4, 0.6) == -3    # SAS_ERR_NO_SCENE
        sc = _synthetic(500, 1, 0.03, n_groups=2)
        _upload(r, sc)
        bad_t = np.array([[0, 1, 3]], np.int32)
        assert L.sas_scene_meshes(r._ctx, 3, p(v), 1, p(bad_t), p(c), p(g), 0.4, 0.6) == -1  # SAS_ERR_INVALID
        bad_g = np.array([2], np.uint8)
        assert L.sas_scene_meshes(r._ctx, 3, p(v), 1, p(t), p(c), p(bad_g), 0.4, 0.6) == -1
        assert L.sas_scene_meshes(r._ctx, 3, p(v), 1, p(t), p(c), p(g), float("nan"), 0.6) == -1
        with pytest.raises(SasError):
            r.upload_meshes(v, [[0, 1, 2]], c, groups=[5])
        r.upload_features(None)
        cam = _ring()
        r.render_features(cam[0], cam[1], cam[2], cam[3])
        r.upload_meshes(v, t, c)
        with pytest.raises(SasError):
            r.render_features(cam[0], cam[1], cam[2], cam[3])
    finally:
        r.close()


def test_h_coplanar_overlap_is_deterministic():
    cam = _ring(80, 60, 70.0)
    r = _empty_scene_rasterizer()
    try:
        v1, t1 = _screen_quad(cam, 2.0, 5, 60, 5, 50)
        v2, t2 = _screen_quad(cam, 2.0, 20, 75, 10, 55)
        verts = np.concatenate([v1, v2])
        tris = np.concatenate([t1, t2 + 4])
        cols = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]], np.float32)
        r.upload_meshes(verts, tris, cols, ambient=1.0, diffuse=0.0)
        a = _frame(r, cam, BG)
        for _ in range(2):
            _same(_frame(r, cam, BG), a)
        assert len(np.unique(a["rgb8"].reshape(-1, 3), axis=0)) >= 3
    finally:
        r.close()


# ---- (b') RGB-D with a mesh: points / mask describe the splats in front of it -------------------------------------------------
def test_b_rgbd_is_filtered_scene():
    sc, cam = _case("n2k_groups")
    V, K, W, H = cam
    r, r2 = Rasterizer(0), Rasterizer(0)
    try:
        sc, d = _scene_with_gap(r, sc, cam)
        keep = np.nonzero(r.read_projection()["depths"] < d)[0]
        v, t = _full_quad(cam, d)
        r.upload_meshes(v, t, C, ambient=1.0, diffuse=0.0)
        _upload(r2, _subset(sc, keep))
        a = _np(r.render_rgbd(V, K, W, H, BG, max_depth=0.5 * d))
        b = _np(r2.render_rgbd(V, K, W, H, C, max_depth=0.5 * d))
        assert set(a) == set(b) and "points" in a
        _same(a, b, keys=tuple(a))
    finally:
        r.close()
        r2.close()


# ---- list overflow: the frame is rendered again with larger lists ------------------------------------------------------------
def test_overflow_regrows_and_matches():
    cam = _ring(1920, 1080, 1000.0, yaw=0.0)
    r = _empty_scene_rasterizer()
    try:
        n = 300
        vs, ts = [], []
        for k in range(n):
            v, t = _full_quad(cam, 2.0 + 0.01 * k)
            vs.append(v)
            ts.append(t + 4 * k)
        cols = _colours(2 * n, 9) / 255.0
        r.upload_meshes(np.concatenate(vs), np.concatenate(ts), cols, ambient=1.0, diffuse=0.0)
        before = r.stats()["regrows"]
        got = _frame(r, cam, BG, want=("rgb", "rgb8"))
        assert r.stats()["regrows"] > before                  # 600 frame-covering triangles: 4.9 M list entries
        r.upload_meshes(vs[0], ts[0], cols[:2], ambient=1.0, diffuse=0.0)   # the nearest quad alone
        _same(got, _frame(r, cam, BG, want=("rgb", "rgb8")), keys=("rgb", "rgb8"))
    finally:
        r.close()


# ---- shared edges: a split square whose diagonal runs exactly through pixel centres ------------------------------------------
def test_top_left_rule_no_holes_no_overlap():
    W = H = 48
    V = np.eye(4, dtype=np.float32)
    K = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)       # u = x / z, v = y / z: exact vertices in pixels
    cam = (V, K, W, H)
    verts = np.array([[8, 8, 1], [40, 8, 1], [40, 40, 1], [8, 40, 1]], np.float32)
    r = _empty_scene_rasterizer()
    try:
        for tris in ([[0, 1, 2], [0, 2, 3]], [[2, 0, 1], [3, 2, 0]]):
            r.upload_meshes(verts, np.array(tris, np.int32), [[1, 0, 0], [0, 0, 1]], ambient=1.0, diffuse=0.0)
            got = _frame(r, cam, (0.0, 0.0, 0.0), want=("rgb8",))["rgb8"].astype(int)
            inside = np.zeros((H, W), bool)
            inside[8:40, 8:40] = True
            red = (got[..., 0] == 255) & (got[..., 2] == 0)
            blue = (got[..., 2] == 255) & (got[..., 0] == 0)
            assert (red | blue)[inside].all() and not (red | blue)[~inside].any()
            diag = red[np.arange(8, 40), np.arange(8, 40)]
            assert diag.all() or not diag.any()                      # the shared edge's centres go to one side
            assert red[inside].sum() in (32 * 31 // 2, 32 * 33 // 2)
    finally:
        r.close()


# ---- (g) the T-block through SplatHandler(meshes=("task",)) ------------------------------------------------------------------
def test_g_task_mesh_through_handler(golden_dir):
    from sim_a_splat_amd import poses
    from sim_a_splat_amd.covariance import compute_cov, sh2rgb
    from sim_a_splat_amd.handler import SplatHandler, TASK_MESH_COLOR
    from sim_a_splat_amd.mesh_io import load_obj
    sc = make_scene(4000, seed=2, log_scale_mean=float(np.log(0.02)))
    covs = compute_cov(torch.from_numpy(sc.quats), torch.from_numpy(sc.scales)).numpy()
    colors = np.clip(sh2rgb(torch.from_numpy(sc.sh[:, 0])).numpy(), 0, 1)
    masks = {"link0": np.arange(4000) < 500, "link1": (np.arange(4000) >= 500) & (np.arange(4000) < 900)}
    ang = 0.4
    icp = np.eye(4)
    icp[:3, :3] = 1.3 * np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    icp[:3, 3] = (0.2, -0.1, 0.05)
    fk = [np.eye(4), np.eye(4)]
    args = (sc.means, covs, colors, sc.opacities, masks, icp, fk)
    h0 = SplatHandler.from_arrays(*args, device=0)
    h1 = SplatHandler.from_arrays(*args, device=0, meshes=())
    h = SplatHandler.from_arrays(*args, device=0, meshes=("task",), task_assets_path=str(golden_dir), task_assets_name="tblock_paper.obj")
    try:
        s, Ri, ti = poses.decompose_icp(icp)
        t_world = np.array([4.0, 4.5, 5.0])                          # far from the Gaussians (all within [-1,1]^3)
        p = Ri.T @ (t_world - ti) / s
        q = np.array([0.9, 0.2, -0.3, 0.25]) * 2.0
        msg = _DrawMsg([3, 3, 2], [(1, 0, 0, 0), (1, 0, 0, 0), q], [(0, 0, 0), (0.01, 0, 0), p])
        for x in (h0, h1, h):
            x.draw_handler(msg)
        cam_q, cam_p = np.array([1.0, 0.0, 0.0, 0.0]), t_world + np.array([0.05, -0.02, -0.7])
        size = [[240, 320]]
        f0, f1 = (x.render(x.scene, [(cam_q, cam_p)], size)[0] for x in (h0, h1))
        assert np.array_equal(f0, f1)
        got = h.render(h.scene, [(cam_q, cam_p)], size)[0].astype(int)
        # the NumPy reference: the posed, scaled block; the draw message's pose through the handle's quaternion
        idx, rows = h.mesh_pose_rows(msg)
        Rt = rows.reshape(3, 4).astype(np.float64)
        v, f = load_obj(golden_dir / "tblock_paper.obj")
        world = (v * s).astype(np.float32).astype(np.float64) @ Rt[:, :3].T + Rt[:, 3]
        V, K = h.scene._view_and_K(240, 320, cam_q, cam_p, h.scene.camera.fov)
        ref, stable = _stable_ref((V, K, 320, 240), world, f)
        assert (ref >= 0).sum() > 500
        cov = stable & (ref >= 0)
        assert (got[cov].sum(-1) > 0).all() and (got[stable & (ref < 0)] == 0).all()
        Vd = np.asarray(V, np.float64)
        campos = -Vd[:3, :3].T @ Vd[:3, 3]
        want = np.zeros((len(f), 3))
        for k, (a, b, c) in enumerate(f):
            n = np.cross(world[b] - world[a], world[c] - world[a])
            d = world[[a, b, c]].mean(0) - campos
            want[k] = np.clip(np.array(TASK_MESH_COLOR) * (0.4 + 0.6 * abs(n @ d) / np.linalg.norm(n) / np.linalg.norm(d)), 0, 1)
        want8 = np.floor(want * 255 + 0.5).astype(int)
        assert np.abs(got[cov] - want8[ref[cov]]).max() <= 1
    finally:
        for x in (h0, h1, h):
            x.scene.close()
