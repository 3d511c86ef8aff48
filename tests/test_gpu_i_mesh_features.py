"""GPU: feature channels, group masks and scene depth of frames WITH meshes (sas_scene_mesh_features, SAS_MESH_SURFACE;
DESIGN.md 3, "Feature channels over meshes" and "Scene depth").

The contract: F[p,k] = sum_{i < cut(p)} vis_i f[i,k] + (1 - alpha_p) m[p,k], m the feature row of the pixel's triangle (the
feature background where none shows), with the triangle, the cut and the weights of the frame's own k_blend_mesh.  Its consequence,
asserted bit for bit on EVERY pixel: for features in [0,1] every clamped triple of channels is the rgb of the scene recoloured with
those channels, its meshes coloured with the triangles' and unshaded.  Against the depth-limited oracle the same holds on the pixels
oracle.mesh_ref calls stable.  With SAS_MESH_SURFACE alpha is exactly 1 where a triangle shows and depth closes on it, within the
derived tolerance of mesh_feature_cases.surface_reference.  The caps asserted here on the reference are settled on the CPU
(tests/test_mesh_features_cpu.py).  Every test fails without the feature: a mesh context refuses feature frames, and mesh_surface is
an unknown argument.  The file runs unchanged under the bounds-checked build.
"""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle
from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import mesh_feature_cases as mf  # noqa: E402

pytestmark = pytest.mark.gpu
OUTS = mc.OUTS
FRAME = ("rgb", "alpha", "depth")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, expectation of view 0): computed once, shared, never modified."""
    case = mf.CASES[name]()
    e = mc.expected(case, 0)
    print(mc.report(name, case, e))
    assert e["excluded"] <= mc.MAX_EXCLUDED, mc.report(name, case, e)
    return case, e


def _setup(r, case, view=0):
    mc.upload_case(r, case)
    Rt = mc.view_poses(case, view)
    if Rt is not None:
        r.set_group_poses(Rt)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _features(r, name, C):
    """F [H,W,C] of a case with drawn features, and what they were."""
    case, _ = _case(name)
    f, fm, fbg = mf.draw_features(case, C, seed=1000 + C)
    V, K, W, H = case["cams"][0]
    _setup(r, case)
    r.upload_features(f)
    r.upload_mesh_features(fm)
    F = r.render_features(V, K, W, H, case["bg"], feature_background=fbg)["features"].cpu().numpy()
    assert F.shape == (H, W, C) and F.dtype == np.float32
    return F, f, fm, fbg


def _recoloured_rgb(r, case, col, mcol, bg, view=0):
    rc = mf.recoloured(case, col, mcol, bg)
    V, K, W, H = case["cams"][view]
    _setup(r, rc, view)
    return r.render(V, K, W, H, rc["bg"], want=("rgb",))["rgb"].cpu().numpy()


# ---- 1. the recolouring identity, GPU against GPU, every pixel ---------------------------------------------------------------------
@pytest.mark.parametrize("C", mf.CHANNELS)
@pytest.mark.parametrize("name", list(mf.CASES))
def test_recolouring_identity_all_pixels(rasterizer, name, C):
    case, _ = _case(name)
    F, f, fm, fbg = _features(rasterizer, name, C)
    for o in mf.triples(C):
        want = np.clip(F[..., o:o + 3], 0.0, 1.0)
        rgb = _recoloured_rgb(rasterizer, case, f[:, o:o + 3], fm[:, o:o + 3], fbg[o:o + 3])
        assert _bits_equal(rgb, want), (name, C, o, int((rgb != want).any(-1).sum()), float(np.abs(rgb - want).max()))


def test_single_channel_takes_the_red_chain(rasterizer):
    """A channel count that is no multiple of 3: channel k against the red channel of the frame recoloured (f_k, f_k, f_k)."""
    name, C, k = "size_17x33", 7, 6
    case, e = _case(name)
    F, f, fm, fbg = _features(rasterizer, name, C)
    rep = lambda a: np.repeat(a[..., k:k + 1], 3, axis=-1)
    want = np.clip(F[..., k], 0.0, 1.0)
    rgb = _recoloured_rgb(rasterizer, case, rep(f), rep(fm), rep(fbg))
    assert _bits_equal(rgb[..., 0], want)
    ref = mf.oracle_recoloured_rgb(case, e, 0, rep(f), rep(fm), rep(fbg))
    assert _bits_equal(ref[..., 0][e["stable"]], want[e["stable"]])


# ---- 2. against the depth-limited oracle on stable pixels ----------------------------------------------------------------------------
@pytest.mark.parametrize("C", mf.CHANNELS)
@pytest.mark.parametrize("name", list(mf.CASES))
def test_features_against_the_oracle(rasterizer, name, C):
    case, e = _case(name)
    F, f, fm, fbg = _features(rasterizer, name, C)
    st = e["stable"]
    for o in mf.triples(C):
        want = np.clip(F[..., o:o + 3], 0.0, 1.0)
        ref = mf.oracle_recoloured_rgb(case, e, 0, f[:, o:o + 3], fm[:, o:o + 3], fbg[o:o + 3])
        d = ref[st] != want[st]
        assert not d.any(), (name, C, o, int(d.sum()), float(np.abs(ref[st] - want[st]).max()))


# ---- 3. the frame of a feature call is the frame of render ----------------------------------------------------------------------------
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("fill", [False, True])
def test_frame_outputs_equal_render(rasterizer, fill, surface):
    case, _ = _case("entry_points")
    V, K, W, H = case["cams"][0]
    f, fm, _ = mf.draw_features(case, 5, seed=3)
    _setup(rasterizer, case)
    rasterizer.upload_features(f)
    rasterizer.upload_mesh_features(fm)
    a = mc.to_numpy(rasterizer.render_features(V, K, W, H, case["bg"], want=FRAME + ("features",), depth_fill_max=fill, mesh_surface=surface))
    b = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=FRAME, depth_fill_max=fill, mesh_surface=surface))
    for k in FRAME:
        assert _bits_equal(a[k], b[k]), (k, fill, surface)


# ---- 4. labels ---------------------------------------------------------------------------------------------------------------------------
def test_labels_with_a_mesh_row(rasterizer):
    case = mf.case_labels()
    e = mc.expected(case, 0)
    want = mf.expected_labels(case, e)
    st, G = e["stable"], case["sc"]["G"]
    mesh_share = float((st & (want["labels"] == G - 1)).mean())
    splat_share = float((st & (want["labels"] < G - 1)).mean())
    print(f"labels: excluded {100 * e['excluded']:.2f} %, mesh row on {100 * mesh_share:.1f} %, splat rows on {100 * splat_share:.1f} % of the frame")
    assert e["excluded"] <= mc.MAX_EXCLUDED and mesh_share >= mf.LABEL_MIN_SHARE and splat_share >= mf.LABEL_MIN_SHARE
    V, K, W, H = case["cams"][0]
    _setup(rasterizer, case)
    o = rasterizer.render_group_masks(V, K, W, H)
    lab, w, a = o["labels"].cpu().numpy(), o["weights"].cpu().numpy(), o["alpha"].cpu().numpy()[..., 0]
    assert lab.dtype == np.uint8 and lab.shape == (H, W) and w.shape == (H, W, G)
    assert np.array_equal(lab[st], want["labels"][st]), int((lab[st] != want["labels"][st]).sum())
    assert np.array_equal(lab[st], mf.labels_of(w, a)[st])
    covered = st & (e["ref"]["winner"] >= 0)
    assert np.array_equal(a[covered], np.ones(int(covered.sum()), np.float32))
    assert float(np.abs(w.sum(-1) - a)[st].max()) <= 1e-6           # sum_g weights = alpha up to rounding
    # a second call finds both one-hot stores in place
    assert torch.equal(rasterizer.render_group_masks(V, K, W, H)["labels"], o["labels"])


# ---- 5. scene depth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mf.CASES))
def test_scene_depth(rasterizer, name):
    """With SAS_MESH_SURFACE: rgb / rgb8 keep their bits; stable uncovered pixels are the oracle frame's; on stable covered pixels
    alpha == 1.0f and |D - D_ref| <= tol, D_ref = ED alpha + (1 - alpha) z_m in float64 from the depth-limited oracle and the mesh
    reference, tol = (delta + 4 * 2^-24) max(z_m, D_ref): delta = 16 * 2^-24 kappa is oracle/mesh_ref.py's bound on the kernel's
    z_m, the four half-ulps are the oracle's division, the 1 - alpha round trip (absolute: hence the max), the product and the
    final fma (mesh_feature_cases.surface_reference).  Derived, not measured."""
    case, e = _case(name)
    s = mf.surface_reference(e)
    V, K, W, H = case["cams"][0]
    _setup(rasterizer, case)
    a = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=OUTS))
    b = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=OUTS, mesh_surface=True))
    assert _bits_equal(a["rgb"], b["rgb"]) and _bits_equal(a["rgb8"], b["rgb8"])
    for k in ("alpha", "depth"):
        assert _bits_equal(a[k][s["off"]], b[k][s["off"]]), k
    assert not mc.compare_stable({k: a[k] for k in FRAME}, e["frame"], e["stable"])   # (the frame without the flag is the oracle's)
    err = np.abs(b["depth"][..., 0][s["on"]].astype(np.float64) - s["D"][s["on"]]) / s["tol"][s["on"]]
    moved = mf.moved_share(b["depth"], a["depth"], s)
    print(f"{name}: covered+stable {int(s['on'].sum())} px, worst depth error {float(err.max(initial=0.0)):.3f} tolerances, "
          f"depth moved on {100 * moved:.1f} % of the frame (reference: {100 * s['moved_share']:.1f} %)")
    diffs = mf.check_surface(b, e, s)
    assert not diffs, (name, diffs)
    if name in mf.DEPTH_MOVES_CASES:
        assert moved >= mf.DEPTH_MOVES_MIN_SHARE, moved


def test_scene_depth_rgbd_and_fill(rasterizer):
    case, e = _case("entry_points")
    s = mf.surface_reference(e)
    V, K, W, H = case["cams"][0]
    _setup(rasterizer, case)
    md = float(np.quantile(s["D"][s["on"]], 0.6))
    for fill in (False, True):
        g = mc.to_numpy(rasterizer.render_rgbd(V, K, W, H, case["bg"], max_depth=md, depth_fill_max=fill, mesh_surface=True))
        ref = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=FRAME, depth_fill_max=fill, mesh_surface=True))
        for k in FRAME:
            assert _bits_equal(g[k], ref[k]), (k, fill)
        assert not mf.check_surface(g, e, s)
        pts, mask = oracle.unproject(g["depth"], K, md)
        assert _bits_equal(g["points"], pts) and np.array_equal(g["mask"], mask)
        assert mask.any() and not mask.all()


def test_scene_depth_posed_batch_equals_single_views(rasterizer):
    case = mc.case_tblock()
    V, K, W, H = case["cams"][0]
    sets = np.stack(case["poses"]).astype(np.float32)
    order = [1, 0, 1]
    mc.upload_case(rasterizer, case)
    Vs, Ks = np.stack([V] * 3), np.stack([K] * 3)
    b = mc.to_numpy(rasterizer.render_batch(Vs, Ks, W, H, case["bg"], want=OUTS, mesh_surface=True, pose_sets=sets, pose_set=order))
    plain = mc.to_numpy(rasterizer.render_batch(Vs, Ks, W, H, case["bg"], want=OUTS, pose_sets=sets, pose_set=order))
    assert not _bits_equal(b["depth"], plain["depth"]) and _bits_equal(b["rgb"], plain["rgb"])
    for k, sidx in enumerate(order):
        rasterizer.set_group_poses(sets[sidx])
        one = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=OUTS, mesh_surface=True))
        for q in OUTS:
            assert _bits_equal(b[q][k], one[q]), (q, k)


# ---- 6. state and status ------------------------------------------------------------------------------------------------------------------
def test_mesh_features_are_forgotten_and_the_refusal_returns(rasterizer):
    case, _ = _case("size_17x33")
    V, K, W, H = case["cams"][0]
    m = case["mesh"]
    f, fm, _ = mf.draw_features(case, 4, seed=9)
    render = lambda: rasterizer.render_features(V, K, W, H)
    forget = (lambda: mc.upload(rasterizer, case["sc"]),
              lambda: rasterizer.upload_meshes(m["verts"], m["tris"], m["cols"], groups=m["groups"]),
              lambda: rasterizer.upload_features(f))
    for step in forget:
        _setup(rasterizer, case)
        rasterizer.upload_features(f)
        with pytest.raises(SasError):
            render()                                        # meshes without features: today's refusal
        rasterizer.upload_mesh_features(fm)
        render()
        step()
        if step is forget[0]:
            rasterizer.upload_features(f)
            render()                                        # (the upload forgot the meshes too: a plain feature frame)
            rasterizer.upload_meshes(m["verts"], m["tris"], m["cols"], groups=m["groups"])
        with pytest.raises(SasError):
            render()
    with pytest.raises(ValueError):
        rasterizer.upload_mesh_features(np.ones((len(m["tris"]) + 1, 4), np.float32))
    with pytest.raises(ValueError):
        rasterizer.upload_mesh_features(np.ones((len(m["tris"]), 5), np.float32))


def test_c_abi_status_codes():
    L = _capi.lib()
    assert _capi.SAS_MESH_SURFACE == 64
    ctx = ctypes.c_void_p()
    assert L.sas_create(0, ctypes.byref(ctx)) == 0
    try:
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        vm = np.eye(4, dtype=np.float32)
        vm[2, 3] = 3.0
        K = np.array([50, 0, 32, 0, 50, 24, 0, 0, 1], np.float32)
        out = torch.empty((48, 64, 3), device="cuda")
        feats = lambda: L.sas_render_features(ctx, p(vm), p(K), 64, 48, None, None, 0, None, None, None, out.data_ptr(), None)
        fm = np.ones((2, 3), np.float32)
        assert L.sas_scene_mesh_features(ctx, 2, 3, p(fm)) == -3                 # SAS_ERR_NO_SCENE
        from sim_a_splat_amd.synthetic import make_scene
        s = make_scene(10, seed=1)
        gid = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0], np.uint8)
        col = np.ascontiguousarray(s.sh[:, 0])
        assert L.sas_scene_upload(ctx, 10, p(s.means), p(s.quats), p(s.scales), None, p(s.opacities), p(col), -1, p(gid), 3) == 0
        assert L.sas_scene_mesh_features(ctx, 2, 3, p(fm)) == -1                 # no meshes
        v = np.array([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float32)
        t = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        c = np.ones((2, 3), np.float32)
        g = np.array([0, 2], np.uint8)
        assert L.sas_scene_meshes(ctx, 4, p(v), 2, p(t), p(c), p(g), 1.0, 0.0) == 0
        assert L.sas_scene_mesh_features(ctx, 2, 3, p(fm)) == -1                 # no feature store
        assert L.sas_scene_features(ctx, 10, 3, None) == 0
        assert feats() == -1                                                     # meshes without features: refused
        assert L.sas_scene_mesh_features(ctx, 3, 3, p(fm)) == -1                 # n_triangles is not the meshes'
        assert L.sas_scene_mesh_features(ctx, 2, 4, p(fm)) == -1                 # channels is not the store's
        assert feats() == -1
        assert L.sas_scene_mesh_features(ctx, 2, 3, p(fm)) == 0
        assert feats() == 0
        assert L.sas_scene_mesh_features(ctx, 2, 3, None) == 0                   # one-hot of the pose groups
        assert feats() == 0
        torch.cuda.synchronize()
        assert abs(float(out[24, 32].sum()) - 1.0) <= 1e-6                       # splat weights + (1 - alpha) of a one-hot row ...
        assert float(out[2, 2].sum()) < 0.5                                      # (no triangle in the corner, zero background)
        f2 = np.ones((10, 2), np.float32)
        assert L.sas_scene_features(ctx, 10, 2, p(f2)) == 0                      # ... a new store forgets the rows
        assert feats() == -1
        assert L.sas_scene_mesh_features(ctx, 2, 2, None) == -1                  # one-hot: group 2 has no channel among 2
        assert L.sas_scene_mesh_features(ctx, 2, 2, p(fm)) == 0
        assert L.sas_scene_meshes(ctx, 4, p(v), 2, p(t), p(c), p(g), 1.0, 0.0) == 0
        assert feats() == -1                                                     # forgotten by sas_scene_meshes
    finally:
        L.sas_destroy(ctx)


def test_overflowing_mesh_lists_rerender_to_the_same_features():
    """80 frame-covering triangles over 1200 tiles: 96 000 list entries against the first guess of 65 536."""
    r = Rasterizer(0)
    try:
        sc = mc.synthetic(3000, 17, 0.03)
        cam = mc.ring(640, 480, 500.0, yaw=0.0)
        mc.upload(r, sc)
        vs, ts = [], []
        for k in range(40):
            v, t = mc.full_quad(cam, 2.6 + 0.02 * k)
            vs.append(v)
            ts.append(t + 4 * k)
        rng = np.random.default_rng(5)
        r.upload_meshes(np.concatenate(vs), np.concatenate(ts), rng.uniform(0, 1, (80, 3)).astype(np.float32), ambient=1.0, diffuse=0.0)
        r.upload_features(rng.uniform(0, 1, (3000, 10)).astype(np.float32))
        r.upload_mesh_features(rng.uniform(0, 1, (80, 10)).astype(np.float32))
        V, K, W, H = cam
        before = r.stats()["regrows"]
        a = r.render_features(V, K, W, H, want=("features", "rgb"))
        grown = r.stats()["regrows"]
        assert grown > before
        b = r.render_features(V, K, W, H, want=("features", "rgb"))
        assert r.stats()["regrows"] == grown
        assert torch.equal(a["features"].view(torch.int32), b["features"].view(torch.int32))
        assert torch.equal(a["rgb"], r.render(V, K, W, H, want=("rgb",))["rgb"])
        alpha = r.render(V, K, W, H, want=("alpha",))["alpha"]
        assert float(alpha.max()) > 0.5 and float(alpha.min()) < 0.5            # splats in front of the nearest quad, and gaps
    finally:
        r.close()


def test_four_async_feature_frames_keep_their_poses(rasterizer):
    case = mc.case_tblock()
    V, K, W, H = case["cams"][0]
    p0, p1 = (np.asarray(p, np.float32) for p in case["poses"])
    p2, p3 = p0.copy(), p1.copy()
    p2[2, 3] += 0.1
    p3[2, 7] -= 0.1
    sets = [p0, p1, p2, p3]
    f, fm, fbg = mf.draw_features(case, 9, seed=21)
    mc.upload_case(rasterizer, case)
    rasterizer.upload_features(f)
    rasterizer.upload_mesh_features(fm)
    outs = []
    for p in sets:
        rasterizer.set_group_poses(p)
        outs.append(rasterizer.render_features(V, K, W, H, case["bg"], feature_background=fbg, want=("features", "rgb"), block=False))
    rasterizer.wait()
    torch.cuda.synchronize()
    for p, o in zip(sets, outs):
        rasterizer.set_group_poses(p)
        ref = rasterizer.render_features(V, K, W, H, case["bg"], feature_background=fbg, want=("features", "rgb"))
        assert torch.equal(o["features"].view(torch.int32), ref["features"].view(torch.int32)) and torch.equal(o["rgb"], ref["rgb"])
    for i in range(4):
        for j in range(i):
            assert not torch.equal(outs[i]["features"], outs[j]["features"])


# ---- 7. Door B -------------------------------------------------------------------------------------------------------------------------------
def test_door_b_segmentation():
    from sim_a_splat_amd.covariance import compute_cov, sh2rgb
    from sim_a_splat_amd.scene import SplatScene
    from sim_a_splat_amd.synthetic import make_scene
    s = make_scene(3000, seed=6, log_scale_mean=float(np.log(0.04)))
    covs = compute_cov(torch.from_numpy(s.quats), torch.from_numpy(s.scales)).numpy()
    cols = np.clip(sh2rgb(torch.from_numpy(s.sh[:, 0])).numpy(), 0, 1).astype(np.float32)
    first = np.arange(3000) < 1200
    wxyz, pos = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, -3.0])
    H, W = 120, 160
    plane_v = np.array([[-2.0, -2.0, 0.1], [0.2, -2.0, 0.1], [0.2, 2.0, -0.1], [-2.0, 2.0, -0.1]], np.float32)
    plane_f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    scene = SplatScene(device=0)
    r = Rasterizer(0)
    try:
        scene.add_gaussian_splats("link", s.means[first], covs[first], cols[first], s.opacities[first], position=(0.1, 0.0, 0.0))
        scene.add_gaussian_splats("rest", s.means[~first], covs[~first], cols[~first], s.opacities[~first])
        scene.add_mesh_simple("table", plane_v, plane_f, color=(0.3, 0.6, 0.9), position=(0.0, 0.05, 0.0))
        assert scene.row_names() == ["link", "rest", "table"]
        seg = scene.get_segmentation(H, W, wxyz, pos)
        lab = seg["labels"].cpu().numpy()
        assert lab.dtype == np.uint8 and lab.shape == (H, W) and seg["weights"].shape == (H, W, 3) and seg["alpha"].shape == (H, W, 1)
        # the same arrays at the Rasterizer level
        order = np.concatenate([np.nonzero(first)[0], np.nonzero(~first)[0]])
        gid = np.concatenate([np.zeros(int(first.sum()), np.uint8), np.ones(int((~first).sum()), np.uint8)])
        r.upload(s.means[order], s.opacities[order], cols[order], covariances=covs[order], sh_degree=-1, group_id=gid, n_groups=3)
        r.upload_meshes(plane_v, plane_f, np.array([0.3, 0.6, 0.9], np.float32), groups=[2, 2], ambient=scene.mesh_ambient, diffuse=scene.mesh_diffuse)
        r.set_group_poses(scene.group_pose_rows())
        V, K = SplatScene._view_and_K(H, W, wxyz, pos, scene.camera.fov)
        want = r.render_group_masks(V, K, W, H)
        assert np.array_equal(lab, want["labels"].cpu().numpy())
        assert torch.equal(seg["weights"].view(torch.int32), want["weights"].view(torch.int32))
        names = scene.row_names()
        shown = {names[i] for i in np.unique(lab) if i != 255}
        assert shown == {"link", "rest", "table"}, shown
        assert float((lab == 2).mean()) > 0.05
        # mesh_surface through the float door: alpha 1 where the table shows
        fl = scene.get_render_float(H, W, wxyz, pos, mesh_surface=True)
        assert bool((fl["alpha"][..., 0][seg["labels"] == 2] == 1.0).all())
    finally:
        r.close()
        scene.close()


def test_handler_render_segmentation():
    from sim_a_splat_amd.handler import SplatHandler
    hs = mc.handler_setup()
    h = SplatHandler.from_arrays(*hs["args"], device=0, meshes=("task",), task_assets_path=str(mc.GOLDEN), task_assets_name="tblock_paper.obj")
    try:
        h.draw_handler(hs["msg"])
        H, W = hs["size"]
        labs = h.render_segmentation(h.scene, [hs["cam"], hs["cam"]], [[H, W], [H // 2, W // 2]])
        assert len(labs) == 2 and labs[0].shape == (H, W) and labs[1].shape == (H // 2, W // 2)
        assert all(lab.dtype == np.uint8 for lab in labs)
        names = h.scene.row_names()
        assert len(names) == 4 and set(np.unique(labs[0])) <= set(range(4)) | {255}
        assert np.array_equal(labs[0], h.scene.get_segmentation(H, W, *hs["cam"])["labels"].cpu().numpy())
    finally:
        h.scene.close()


# ---- 8. drawn cases -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", mf.DRAWN_SEEDS_SKIPPED)
def test_drawn_cases_recolouring_only(rasterizer, seed):
    """The drawn seeds whose grazing triangles put the scene-depth tolerance beyond its cap: the recolouring identity on every
    pixel needs no reference, so the hardest geometry is not left out of it."""
    case = mf.drawn_case(seed)
    print(case["describe"])
    V, K, W, H = case["cams"][0]
    C = 9
    f, fm, fbg = mf.draw_features(case, C, seed=4000 + seed)
    _setup(rasterizer, case)
    rasterizer.upload_features(f)
    rasterizer.upload_mesh_features(fm)
    F = rasterizer.render_features(V, K, W, H, case["bg"], feature_background=fbg)["features"].cpu().numpy()
    for o in mf.triples(C):
        want = np.clip(F[..., o:o + 3], 0.0, 1.0)
        rgb = _recoloured_rgb(rasterizer, case, f[:, o:o + 3], fm[:, o:o + 3], fbg[o:o + 3])
        assert _bits_equal(rgb, want), (seed, o, int((rgb != want).any(-1).sum()))


@pytest.mark.parametrize("seed", mf.DRAWN_SEEDS)
def test_drawn_cases(rasterizer, seed):
    """oracle_fuzz.draw_mesh_case(seed), first view: the recolouring identity on every pixel (C = 9: a partial second chunk) and
    the scene depth against the reference."""
    import oracle_fuzz as fz
    case = mf.drawn_case(seed)
    e = mc.expected(case, 0)
    print(f"{case['describe']} | excluded {100 * e['excluded']:.2f} %")
    assert e["excluded"] <= fz.MESH_MAX_EXCLUDED
    V, K, W, H = case["cams"][0]
    C = 9
    f, fm, fbg = mf.draw_features(case, C, seed=4000 + seed)
    _setup(rasterizer, case)
    rasterizer.upload_features(f)
    rasterizer.upload_mesh_features(fm)
    F = rasterizer.render_features(V, K, W, H, case["bg"], feature_background=fbg)["features"].cpu().numpy()
    a = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=OUTS))
    b = mc.to_numpy(rasterizer.render(V, K, W, H, case["bg"], want=OUTS, mesh_surface=True))
    assert _bits_equal(a["rgb"], b["rgb"]) and _bits_equal(a["rgb8"], b["rgb8"])
    diffs = mf.check_surface(b, e)
    assert not diffs, (seed, diffs)
    for o in mf.triples(C):
        want = np.clip(F[..., o:o + 3], 0.0, 1.0)
        rgb = _recoloured_rgb(rasterizer, case, f[:, o:o + 3], fm[:, o:o + 3], fbg[o:o + 3])
        assert _bits_equal(rgb, want), (seed, o, int((rgb != want).any(-1).sum()))
