"""GPU: per-Gaussian feature channels (sas_scene_features / sas_render_features) and splat-group masks.

The contract ("Feature channels"): F[p,k] = sum_i vis_i f[i,k] + (1 - alpha_p) fbg[k] with the frame's own
weights, unclamped, features through the colours' finite mapping.  Its consequence, asserted bit for bit: for features in
[0,1], every clamped triple of channels IS the rgb of the scene recoloured with those three channels (sh_degree = -1,
fbg = bg) -- on the lazy path, the full path and the C oracle.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle
from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError, group_labels
from sim_a_splat_amd.synthetic import make_scene, random_group_poses, ring_camera

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
from scene_cases import config3_window as _config3_window, synthetic as _synthetic, twin as _twin, upload as _upload  # noqa: E402

pytestmark = pytest.mark.gpu
FMAX = np.float32(3.402823466e38)


def _oracle_rgb(sc, colors, view, bg):
    V, K, W, H = view
    kw = dict(cov6=sc["cov6"]) if sc["cov6"] is not None else dict(quats=sc["quats"], scales=sc["scales"])
    return oracle.render(sc["means"], sc["op"], colors, V, K, W, H, sh_degree=-1, group_id=sc["gid"], group_Rt=sc["Rt"],
                         background=tuple(float(v) for v in bg), **kw)["rgb"]


def _feat(r, sc, view, f, fbg=None, **kw):
    _upload(r, sc)
    r.upload_features(f)
    V, K, W, H = view
    return r.render_features(V, K, W, H, feature_background=fbg, **kw)["features"].cpu().numpy()


def _triples(C):
    return sorted({0, C // 2 - 1, C - 3})   # the first, one across a chunk boundary (C = 37: 17..19), the chunk tail


def _check_recolour(r, sc, view, C, seed, with_oracle=True, fast_exp=False):
    rng = np.random.default_rng(seed)
    n = sc["means"].shape[0]
    f = rng.uniform(0.0, 1.0, size=(n, C)).astype(np.float32)
    fbg = rng.uniform(0.0, 1.0, size=C).astype(np.float32)
    F = _feat(r, sc, view, f, fbg, fast_exp=fast_exp)
    V, K, W, H = view
    assert F.shape == (H, W, C) and F.dtype == np.float32
    for o in _triples(C):
        want = np.clip(F[..., o:o + 3], 0.0, 1.0)
        col, bg = np.ascontiguousarray(f[:, o:o + 3]), tuple(float(v) for v in fbg[o:o + 3])
        _upload(r, sc, colors=col)
        for full in ((False,) if fast_exp else (False, True)):
            rgb = r.render(V, K, W, H, bg, want=("rgb",), fast_exp=fast_exp, full_sort=full)["rgb"].cpu().numpy()
            assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32)), (o, full, np.abs(rgb - want).max())
        if with_oracle and not fast_exp:
            ref = _oracle_rgb(sc, col, view, bg)
            assert np.array_equal(ref.view(np.uint32), want.view(np.uint32)), (o, np.abs(ref - want).max())
    return F


# ---- 1. the recolour identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n2k", "n2k_groups", "dense", "inside"])
@pytest.mark.parametrize("C", [7, 37])
def test_recolour_identity_on_twin_fixtures(rasterizer, name, C):
    sc, view = _twin(name)
    _check_recolour(rasterizer, sc, view, C, seed=C)


@pytest.mark.parametrize("C", [7, 37])
def test_recolour_identity_ragged_frame(rasterizer, C):
    sc = _synthetic(20000, seed=5, ls=0.02, n_groups=3)
    cam = ring_camera(1000, 600, 700.0, yaw_deg=30.0)
    view = (cam.viewmat, cam.K, 1000, 600)
    F = _check_recolour(rasterizer, sc, view, C, seed=100 + C)
    assert (F[..., 0] != 0).mean() > 0.2


@pytest.mark.parametrize("C", [7, 37])
def test_recolour_identity_config3_window(rasterizer, C):
    sc, view = _config3_window()
    _check_recolour(rasterizer, sc, view, C, seed=200 + C, with_oracle=C == 7)


def test_recolour_identity_fast_exp(rasterizer):
    for name in ("n2k", "dense"):
        sc, view = _twin(name)
        _check_recolour(rasterizer, sc, view, 7, seed=3, fast_exp=True)


# ---- 2. the frame itself is unchanged ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True])
def test_frame_outputs_equal_render(rasterizer, fill):
    sc, view = _twin("dense")
    V, K, W, H = view
    _upload(rasterizer, sc)
    rasterizer.upload_features(np.random.default_rng(1).normal(size=(sc["means"].shape[0], 5)).astype(np.float32))
    bg = (0.1, 0.7, 0.3)
    a = rasterizer.render_features(V, K, W, H, bg, want=("features", "rgb", "alpha", "depth"), depth_fill_max=fill)
    b = rasterizer.render(V, K, W, H, bg, want=("rgb", "alpha", "depth"), depth_fill_max=fill)
    for k in ("rgb", "alpha", "depth"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert set(a) == {"features", "rgb", "alpha", "depth"}


def test_full_sort_frames_composite_with_k_blend_alone(rasterizer):
    """A SAS_FULL_SORT frame (plain or with features) is composited by k_blend alone: the lazy tile kernel, which counts the
    tiles it had to order completely, must not run behind it.  Coplanar splats make every tile such a tile."""
    rng = np.random.default_rng(21)
    s = make_scene(20000, seed=97, log_scale_mean=float(np.log(0.02)))
    s.means[:, 2] = 0.0
    s.means[:, :2] = rng.uniform(-0.5, 0.5, size=(s.n, 2)).astype(np.float32)
    s.opacities[:] = np.clip(s.opacities, 0.01, 0.05)
    cam = ring_camera(96, 64, 90.0)
    r = rasterizer
    r.upload(s.means, s.opacities, s.sh, quats=s.quats, scales=s.scales, sh_degree=s.sh_degree)
    lazy = r.render(cam.viewmat, cam.K, 96, 64, want=("rgb", "alpha"))
    assert r.stats()["fallback_tiles"] > 0
    full = r.render(cam.viewmat, cam.K, 96, 64, want=("rgb", "alpha"), full_sort=True)
    assert r.stats()["fallback_tiles"] == 0
    r.upload_features(np.ones((s.n, 1), np.float32))
    feat = r.render_features(cam.viewmat, cam.K, 96, 64, want=("features", "rgb", "alpha"))
    assert r.stats()["fallback_tiles"] == 0
    for k in ("rgb", "alpha"):
        assert torch.equal(lazy[k], full[k]) and torch.equal(lazy[k], feat[k]), k


# ---- 3. outside [0,1]: exact identities -------------------------------------------------------------------------------
def test_sign_scale_and_channel_identities(rasterizer):
    sc, view = _twin("n2k_groups")
    n = sc["means"].shape[0]
    f = np.random.default_rng(7).uniform(-2.0, 3.0, size=(n, 37)).astype(np.float32)
    F = _feat(rasterizer, sc, view, f)
    assert np.abs(F).max() > 1.0
    z = lambda a: (a + np.float32(0.0)).view(np.uint32)   # (-0 and +0: a pixel nothing reaches holds +0 either way)
    assert np.array_equal(z(_feat(rasterizer, sc, view, -f)), z(-F))
    for k in (3, -3):
        s = np.float32(2.0 ** k)
        assert np.array_equal(_feat(rasterizer, sc, view, f * s).view(np.uint32), (F * s).view(np.uint32)), k
    for ch in (0, 8, 20, 36):
        one = _feat(rasterizer, sc, view, np.ascontiguousarray(f[:, ch:ch + 1]))
        assert np.array_equal(one[..., 0].view(np.uint32), F[..., ch].view(np.uint32)), ch


# ---- 4. poisoned features -----------------------------------------------------------------------------------------------
def test_poisoned_features_render_as_their_finite_mapping(rasterizer):
    sc, view = _twin("dense")
    n = sc["means"].shape[0]
    rng = np.random.default_rng(9)
    f = rng.uniform(0.0, 1.0, size=(n, 11)).astype(np.float32)
    poison = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    hit = rng.random(size=f.shape) < 0.2
    f[hit] = rng.choice(poison, size=int(hit.sum()))
    mapped = np.where(np.isnan(f), -FMAX, np.clip(f, -FMAX, FMAX)).astype(np.float32)
    fbg = rng.uniform(0, 1, size=11).astype(np.float32)
    a = _feat(rasterizer, sc, view, f, fbg)
    b = _feat(rasterizer, sc, view, mapped, fbg)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # device-resident input takes the same path
    c = _feat(rasterizer, sc, view, torch.from_numpy(f).cuda(), fbg)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ---- 5. group masks ---------------------------------------------------------------------------------------------------------
def _xarm_scene(golden_dir):
    from sim_a_splat_amd.covariance import compute_cov, sh2rgb
    with np.load(golden_dir / "scene_assets_xarm6_1.npz") as z:
        a = {k: z[k] for k in z.files}
    n = int(a["n"])
    masks = [np.unpackbits(b, count=n).astype(bool) for b in a["mask_bits"]]
    s = make_scene(n, seed=2, log_scale_mean=float(np.log(0.012)))
    covs = compute_cov(torch.from_numpy(s.quats), torch.from_numpy(s.scales)).numpy()
    colors = np.clip(sh2rgb(torch.from_numpy(s.sh[:, 0])).numpy(), 0, 1).astype(np.float32)
    # registration order of the handler: the links (a Gaussian in two masks twice), then the static rest (group 7)
    idx = [np.nonzero(m)[0] for m in masks]
    rest = np.nonzero(~np.logical_or.reduce(masks))[0]
    order = np.concatenate(idx + [rest])
    gid = np.concatenate([np.full(len(ix), i, np.uint8) for i, ix in enumerate(idx)] + [np.full(len(rest), 7, np.uint8)])
    cov6 = np.stack([covs[:, 0, 0], covs[:, 0, 1], covs[:, 0, 2], covs[:, 1, 1], covs[:, 1, 2], covs[:, 2, 2]], 1)[order]
    Rt = random_group_poses(8, seed=31, max_angle=0.4, max_shift=0.15)[[1, 2, 3, 4, 5, 6, 7, 0]]   # group 7 (static) identity
    return dict(means=s.means[order], op=s.opacities[order], colors=colors[order], sh=-1, quats=None, scales=None,
                cov6=np.ascontiguousarray(cov6, dtype=np.float32), gid=gid, G=8, Rt=Rt)


def test_group_masks_on_the_shipped_link_masks(rasterizer, golden_dir):
    sc = _xarm_scene(golden_dir)
    assert not np.allclose(sc["Rt"][:7], np.tile([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], (7, 1)))
    cam = ring_camera(640, 480, 520.0, yaw_deg=25.0, elev=0.3)
    view = (cam.viewmat, cam.K, 640, 480)
    r = rasterizer
    _upload(r, sc)
    m = r.render_group_masks(cam.viewmat, cam.K, 640, 480, min_alpha=0.5)
    Wt, lab, alpha = m["weights"].cpu().numpy(), m["labels"].cpu().numpy(), m["alpha"].cpu().numpy()
    assert Wt.shape == (480, 640, 8) and lab.shape == (480, 640) and lab.dtype == np.uint8 and alpha.shape == (480, 640, 1)
    # device one-hot == an explicit one-hot upload, bitwise
    onehot = np.eye(8, dtype=np.float32)[sc["gid"]]
    F = _feat(r, sc, view, onehot)
    assert np.array_equal(F.view(np.uint32), Wt.view(np.uint32))
    # every weight triple is the rgb of the scene coloured by one-hot group triples
    for o in (0, 3, 5):
        _upload(r, sc, colors=np.ascontiguousarray(onehot[:, o:o + 3]))
        rgb = r.render(cam.viewmat, cam.K, 640, 480, (0.0, 0.0, 0.0), want=("rgb",))["rgb"].cpu().numpy()
        assert np.array_equal(rgb.view(np.uint32), np.clip(Wt[..., o:o + 3], 0, 1).view(np.uint32)), o
    assert np.abs(Wt.sum(-1, dtype=np.float64) - alpha[..., 0]).max() <= 1e-6
    top = Wt.max(-1, keepdims=True)
    ref = np.argmax(Wt == top, axis=-1).astype(np.uint8)
    ref[alpha[..., 0] < 0.5] = 255
    assert np.array_equal(lab, ref)
    seen = set(np.unique(lab).tolist())
    assert len(seen - {255}) >= 4, seen      # several links are in view
    # a second call reuses the one-hot store
    m2 = r.render_group_masks(cam.viewmat, cam.K, 640, 480)
    assert torch.equal(m2["labels"], m["labels"])


# ---- 6. edge cases -------------------------------------------------------------------------------------------------------
def test_empty_scene(rasterizer):
    e = np.zeros((0, 3), np.float32)
    rasterizer.upload(e, np.zeros((0,), np.float32), np.zeros((0, 3), np.float32), quats=np.zeros((0, 4), np.float32),
                      scales=e, sh_degree=-1)
    rasterizer.upload_features(np.zeros((0, 4), np.float32))
    cam = ring_camera(64, 48, 50.0)
    o = rasterizer.render_features(cam.viewmat, cam.K, 64, 48, feature_background=[1, 2, 3, 4], want=("features", "alpha"))
    assert torch.equal(o["alpha"], torch.zeros_like(o["alpha"]))
    assert torch.equal(o["features"], torch.tensor([1.0, 2, 3, 4], device="cuda").expand(48, 64, 4))


def test_overflowing_lists_regrow_and_render_the_same_features():
    """Lists beyond the first intersection buffer (2^20 keys here): the frame is rendered again, features included."""
    r = Rasterizer("cuda:0")
    sc = _synthetic(30000, seed=444, ls=0.12)
    _upload(r, sc)
    f = np.random.default_rng(4).uniform(0, 1, size=(30000, 10)).astype(np.float32)
    r.upload_features(f)
    cam = ring_camera(640, 480, 500.0, yaw_deg=0.0)
    a = r.render_features(cam.viewmat, cam.K, 640, 480, want=("features", "rgb"))
    st = r.stats()
    assert st["regrows"] >= 1 and st["n_isect"] > (1 << 20)
    b = r.render_features(cam.viewmat, cam.K, 640, 480, want=("features", "rgb"))
    assert r.stats()["regrows"] == st["regrows"]
    assert torch.equal(a["features"].view(torch.int32), b["features"].view(torch.int32))
    ref = r.render(cam.viewmat, cam.K, 640, 480, want=("rgb",))["rgb"]
    assert torch.equal(a["rgb"], ref)
    r.close()


def test_four_async_frames(rasterizer):
    sc = _synthetic(8000, seed=8, ls=0.03, n_groups=2)
    _upload(rasterizer, sc)
    f = np.random.default_rng(12).uniform(-1, 1, size=(8000, 9)).astype(np.float32)
    rasterizer.upload_features(f)
    cams = [ring_camera(320, 240, 260.0, yaw_deg=40.0 * i, elev=0.1 * i) for i in range(4)]
    outs = [rasterizer.render_features(c.viewmat, c.K, 320, 240, want=("features", "alpha"), block=False) for c in cams]
    rasterizer.wait()
    for c, o in zip(cams, outs):
        ref = rasterizer.render_features(c.viewmat, c.K, 320, 240, want=("features", "alpha"))
        assert torch.equal(o["features"].view(torch.int32), ref["features"].view(torch.int32))
        assert torch.equal(o["alpha"], ref["alpha"]) and float(o["alpha"].max()) > 0.5
    assert not torch.equal(outs[0]["features"], outs[1]["features"])


def test_c_abi_status_codes():
    L = _capi.lib()
    ctx = ctypes.c_void_p()
    assert L.sas_create(0, ctypes.byref(ctx)) == 0
    try:
        vm = np.eye(4, dtype=np.float32)
        vm[2, 3] = 3.0
        K = np.array([50, 0, 32, 0, 50, 24, 0, 0, 1], np.float32)
        out = torch.empty((48, 64, 3), device="cuda")
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        f = np.ones((10, 3), np.float32)
        assert L.sas_scene_features(ctx, 10, 3, p(f)) == -3                       # no scene
        assert L.sas_render_features(ctx, p(vm), p(K), 64, 48, None, None, 0, None, None, None, out.data_ptr(), None) == -3
        s = make_scene(10, seed=1)
        gid = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0], np.uint8)
        col = np.ascontiguousarray(s.sh[:, 0])
        assert L.sas_scene_upload(ctx, 10, p(s.means), p(s.quats), p(s.scales), None, p(s.opacities), p(col), -1, p(gid), 3) == 0
        assert L.sas_render_features(ctx, p(vm), p(K), 64, 48, None, None, 0, None, None, None, out.data_ptr(), None) == -1  # none set
        assert L.sas_scene_features(ctx, 9, 3, p(f)) == -1                       # n is not the scene's
        assert L.sas_scene_features(ctx, 10, 0, p(f)) == -1                      # C out of range
        assert L.sas_scene_features(ctx, 10, 257, p(np.ones((10, 257), np.float32))) == -1
        assert L.sas_scene_features(ctx, 10, 4, None) == -1                      # one-hot needs C == n_groups
        assert L.sas_scene_features(ctx, 10, 3, None) == 0
        assert L.sas_render_features(ctx, p(vm), p(K), 64, 48, None, None, 0, None, None, None, None, None) == -1  # no output
        assert L.sas_render_features(ctx, p(vm), p(K), 64, 48, None, None, 0, None, None, None, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert L.sas_scene_upload(ctx, 10, p(s.means), p(s.quats), p(s.scales), None, p(s.opacities), p(col), -1, None, 0) == 0
        assert L.sas_render_features(ctx, p(vm), p(K), 64, 48, None, None, 0, None, None, None, out.data_ptr(), None) == -1  # forgotten
        assert L.sas_scene_features(ctx, 10, 3, None) == -1                      # one-hot without groups
        assert L.sas_scene_features(ctx, 10, 3, p(f)) == 0
    finally:
        L.sas_destroy(ctx)


def test_python_errors(rasterizer):
    sc, view = _twin("n2k")
    _upload(rasterizer, sc)
    V, K, W, H = view
    with pytest.raises(SasError):
        rasterizer.render_features(V, K, W, H)                 # nothing uploaded for this scene
    with pytest.raises(ValueError):
        rasterizer.upload_features(None)                       # no groups
    with pytest.raises(ValueError):
        rasterizer.upload_features(np.ones((3, 2), np.float32))
    rasterizer.upload_features(np.ones((sc["means"].shape[0], 2), np.float32))
    with pytest.raises(ValueError):
        rasterizer.render_features(V, K, W, H, feature_background=[1.0, 2.0, 3.0])
    o = rasterizer.render_features(V, K, W, H, want=("features", "alpha"))
    assert torch.equal(o["features"][..., :1], o["features"][..., 1:])
    # every pixel: 1 * sum(vis) = alpha up to rounding
    assert float((o["features"][..., :1] - o["alpha"]).abs().max()) <= 1e-6
    assert torch.equal(group_labels(o["features"], o["alpha"], 2.0), torch.full((H, W), 255, dtype=torch.uint8, device="cuda"))
