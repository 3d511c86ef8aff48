"""GPU: feature lifting (sas_lift_features; DESIGN.md 3, "Feature lifting"): per-Gaussian sums of the pixels' quantised channels,
weighted by the compositing weights, and what the host makes of them.

The integer outputs are compared for exact int64 equality with tests/tools/lift_features_ref.py: the weights of the C oracle's
one-hot frames (or, for the dense scene, of render_features with explicit one-hot features), quantised and multiplied in numpy.
Integer sums have no order, so there is nothing to tolerate.  Every test fails without the feature (no symbol, no method).  The file
runs unchanged under the bounds-checked build.
"""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import LIFT_FEATURE_ONE, SasError
from sim_a_splat_amd.semantics import features_from_sums, lift_feature_views, masks_from_relevancy, relevancy

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import lift_features_fuzz as ff  # noqa: E402
import lift_features_ref as fr  # noqa: E402
import lift_ref as lr  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (40, 24), (17, 33)]   # whole tiles; ragged in both axes
CHANNELS = [1, 3, 8, 9, 17, 256]         # below, at and beyond one chunk of 8; three chunks with a ragged one; the most


@functools.lru_cache(maxsize=None)
def _small(size):
    """The 64-Gaussian scene in 3 posed groups, its camera and its weights [64,H,W] from the oracle (once per size)."""
    W, H = size
    sc = lr.blob_scene(64, 11, 0.12, n_groups=3)
    cam = sc_kit.ring(W, H, f=0.45 * max(W, H))
    return sc, cam, lr.weights_oracle(sc, cam)


@functools.lru_cache(maxsize=None)
def _features(size, C, views=1, seed=0):
    """N(0,1) feature images [views,H,W,C] from a fixed seed, and their scale 32767 / max|f|."""
    W, H = size
    img = np.random.default_rng(1000 + C + 7919 * seed).normal(size=(views, H, W, C)).astype(np.float32)
    return img, fr.auto_scale(img)


def _eq(got, sums, weight):
    s, w = got["sums"].cpu().numpy(), got["weight"].cpu().numpy()
    assert s.dtype == np.int64 and w.dtype == np.int64 and s.shape == sums.shape and w.shape == weight.shape
    assert np.array_equal(w, weight), (int((w != weight).sum()), np.abs(w - weight).max())
    assert np.array_equal(s, sums), (int((s != sums).sum()), np.abs(s - sums).max())


# ---- 1. sizes and channel counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("size", SIZES)
def test_sizes_and_channel_counts(rasterizer, size, C):
    r = rasterizer
    sc, cam, w = _small(size)
    V, K, W, H = cam
    img, scale = _features(size, C)
    sums, weight = fr.sums(w, img[0], scale)
    assert (weight > 0).all() and 1e11 < np.abs(sums).max() < 1e12           # every Gaussian is seen; far from int64's end
    if C == 17:   # (a property of the case) no weight that counts at label lifting's 2^32 is lost at 2^24
        assert not ((lr.quantise(w) > 0) & (fr.quantise_weights(w) == 0)).any()
    sc_kit.upload(r, sc)
    got = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale)
    assert got["sums"].shape == (64, C) and got["weight"].shape == (64,) and got["sums"].is_cuda and got["feature_scale"] == scale
    _eq(got, sums, weight)
    assert LIFT_FEATURE_ONE == 2 ** 24 and int(got["weight"].max()) > LIFT_FEATURE_ONE   # more than one pixel's worth somewhere
    auto = r.lift_features(V[None], K[None], W, H, torch.from_numpy(img).cuda())           # the call's own scale is the same number
    assert auto["feature_scale"] == scale
    _eq(auto, sums, weight)


# ---- 2. the dense scene: batches of 256, pixels that terminate ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense():
    sc = lr.blob_scene(2000, 7, 0.15, spread=1.0, z_spread=0.5, op=(0.5, 0.95))
    cam = sc_kit.ring(32, 32, f=36.0, yaw=0.0, elev=0.0)
    return sc, cam


def test_dense_lists_cross_batches_and_pixels_terminate(rasterizer):
    r = rasterizer
    sc, cam = _dense()
    V, K, W, H = cam
    w = lr.weights_features(r, sc, cam)                        # [2000,32,32]; leaves the scene uploaded
    alpha = r.render(V, K, W, H, want=("alpha",), full_sort=True)["alpha"].cpu().numpy()[..., 0]
    lens = np.diff(r.read_tile_lists(4)["tile_offsets"])
    stopped = 1.0 - alpha <= 2e-4                              # (a property of the case: such a pixel has all but surely met the stop)
    print(f"dense: lists of {lens.min()}..{lens.max()} entries, {int(stopped.sum())} of {W * H} pixels at T <= 2e-4")
    assert lens.min() > 1024 and stopped.sum() > 100           # four batches and more per tile; the stop is exercised
    img, scale = _features((W, H), 9)
    sums, weight = fr.sums(w, img[0], scale)
    got = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale)
    _eq(got, sums, weight)
    assert (weight == 0).sum() > 0                             # Gaussians wholly behind the stop, or never passing the alpha test
    # the stopping entry and the tail are absent: what the Gaussians were given at a pixel sums to that pixel's alpha = 1 - T, no more
    # (per entry of a pixel's list, a weight loses < 2^-24 to the floor and T falls by it with one float32 rounding, <= 2^-25)
    per_pixel = float(lens.max()) * 1.5 * 2.0 ** -24
    assert abs(float(weight.sum()) / LIFT_FEATURE_ONE - float(alpha.astype(np.float64).sum())) < per_pixel * alpha.size


# ---- 3. the quantiser's edges, masks, constant images --------------------------------------------------------------------------------------
def test_quantiser_edges_and_mask(rasterizer):
    r = rasterizer
    sc, cam, w = _small((40, 24))
    V, K, W, H = cam
    scale = 4.0
    edge = np.array([np.nan, np.inf, -np.inf, 32767.0 / 4 + 1.0, -1e30, 1e30, 0.125, 0.375, 0.625, -0.125, -0.375, -0.0, 0.0, 8191.625,
                     8191.75, -8191.875], np.float32)
    assert fr.quantise_features(edge, scale).tolist() == [0, 32767, -32767, 32767, -32767, 32767, 0, 2, 2, 0, -2, 0, 0, 32766, 32767, -32767]
    rng = np.random.default_rng(3)
    img = edge[rng.integers(0, len(edge), size=(1, H, W, 11))]
    mask = rng.choice(np.array([0, 1, 200], np.uint8), size=(1, H, W))
    sc_kit.upload(r, sc)
    for m in (None, mask):
        sums, weight = fr.sums(w, img[0], scale, None if m is None else m[0])
        _eq(r.lift_features(V[None], K[None], W, H, img, feature_scale=scale, mask=m), sums, weight)
    full = fr.sums(w, img[0], scale)
    assert (weight < full[1]).any() and (weight > 0).any()     # the mask took weight away, and not all of it
    none = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale, mask=np.zeros((1, H, W), np.uint8))
    assert not none["sums"].any() and not none["weight"].any()  # a masked pixel adds to neither output
    # NaN and Inf do not touch the call's own scale: max over the finite values (here 1e30: everything else quantises to 0 or saturates)
    assert r.lift_features(V[None], K[None], W, H, img)["feature_scale"] == fr.auto_scale(img) == float(np.float32(32767.0 / float(np.float32(1e30))))


def test_constant_image_gives_fq_times_weight(rasterizer):
    r = rasterizer
    sc, cam, w = _small((17, 33))
    V, K, W, H = cam
    c = np.array([0.3, -1.7, 0.0, 2.5, -2.5, 1e9, -0.01, 5.0, 0.11], np.float32)
    scale = 100.0
    fq = fr.quantise_features(c, scale)
    assert fq.tolist() == [30, -170, 0, 250, -250, 32767, -1, 500, 11]
    sc_kit.upload(r, sc)
    got = r.lift_features(V[None], K[None], W, H, np.broadcast_to(c, (1, H, W, 9)), feature_scale=scale)
    weight = fr.quantise_weights(w).reshape(64, -1).sum(axis=1)
    _eq(got, weight[:, None] * fq[None, :], weight)


# ---- 4. accumulation, one output alone, group poses -----------------------------------------------------------------------------------------
def test_accumulation_over_views_and_calls(rasterizer):
    r = rasterizer
    sc, cam, w0 = _small((40, 24))
    V, K, W, H = cam
    cams = [cam, sc_kit.ring(W, H, f=0.45 * W, yaw=70.0, elev=0.4), sc_kit.ring(W, H, f=0.6 * W, yaw=200.0, elev=-0.3)]
    Vs, Ks = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    img, scale = _features((W, H), 9, views=3)
    refs = [fr.sums(w0 if k == 0 else lr.weights_oracle(sc, c), img[k], scale) for k, c in enumerate(cams)]
    sums, weight = sum(x[0] for x in refs), sum(x[1] for x in refs)
    assert not np.array_equal(refs[0][1], refs[1][1]) and not np.array_equal(refs[1][1], refs[2][1])
    sc_kit.upload(r, sc)
    kw = dict(feature_scale=scale)
    all3 = r.lift_features(Vs, Ks, W, H, img, **kw)                               # three views in one call
    _eq(all3, sums, weight)
    one = [r.lift_features(Vs[k:k + 1], Ks[k:k + 1], W, H, img[k:k + 1], **kw) for k in range(3)]   # ... equal one call each
    _eq({"sums": one[0]["sums"] + one[1]["sums"] + one[2]["sums"], "weight": one[0]["weight"] + one[1]["weight"] + one[2]["weight"]}, sums, weight)
    acc = r.lift_features(Vs[:2], Ks[:2], W, H, img[:2], **kw)                    # ... equal two calls into one buffer
    same = r.lift_features(Vs[2:], Ks[2:], W, H, img[2:], sums=acc["sums"], weight=acc["weight"], **kw)
    assert same["sums"].data_ptr() == acc["sums"].data_ptr() and same["weight"].data_ptr() == acc["weight"].data_ptr()
    _eq(acc, sums, weight)
    again = r.lift_features(Vs, Ks, W, H, img, **kw)                              # the same call again: the same bits
    assert torch.equal(again["sums"], all3["sums"]) and torch.equal(again["weight"], all3["weight"])
    loop = lift_feature_views(r, Vs, Ks, W, H, [img[0], torch.from_numpy(img[1]), img[2]], scale, views_per_call=2)
    assert torch.equal(loop["sums"], all3["sums"]) and torch.equal(loop["weight"], all3["weight"]) and loop["feature_scale"] == scale


def test_slabs_of_channels_beyond_256(rasterizer):
    r = rasterizer
    sc, cam, w = _small((17, 33))
    V, K, W, H = cam
    img, scale = _features((W, H), 300)
    sums, weight = fr.sums(w, img[0], scale)
    sc_kit.upload(r, sc)
    got = lift_feature_views(r, V[None], K[None], W, H, img, scale)
    assert got["sums"].shape == (64, 300)
    _eq(got, sums, weight)                                                        # (weight counted once, with the first slab)
    with pytest.raises(SasError, match="channels"):
        r.lift_features(V[None], K[None], W, H, img, feature_scale=scale)


def test_sums_alone_and_weight_alone(rasterizer):
    r = rasterizer
    sc, cam, w = _small((17, 33))
    V, K, W, H = cam
    img, scale = _features((W, H), 17)
    sums, weight = fr.sums(w, img[0], scale)
    sc_kit.upload(r, sc)
    only_w = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale, sums=False)
    only_s = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale, weight=False)
    assert set(only_w) == {"weight", "feature_scale"} and set(only_s) == {"sums", "feature_scale"}
    _eq({"sums": only_s["sums"], "weight": only_w["weight"]}, sums, weight)
    with pytest.raises(ValueError):
        r.lift_features(V[None], K[None], W, H, img, sums=False, weight=False)
    with pytest.raises(ValueError):
        r.lift_features(V[None], K[None], W, H, img, weight=torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        r.lift_features(V[None], K[None], W, H, img[:, :-1])
    with pytest.raises(ValueError):
        r.lift_features(V[None], K[None], W, H, img, mask=np.ones((1, H, W - 1), np.uint8))


def test_sums_follow_the_group_poses(rasterizer):
    r = rasterizer
    sc, cam, w0 = _small((32, 32))
    V, K, W, H = cam
    Rt = np.asarray(sc["Rt"], np.float32).reshape(3, 12).copy()
    Rt[1, 3] += 0.35
    Rt[2, 7] -= 0.3
    Rt[2, 11] += 0.2
    img, scale = _features((W, H), 9)
    sums, weight = fr.sums(lr.weights_oracle(sc, cam, Rt=Rt), img[0], scale)
    old = fr.sums(w0, img[0], scale)
    assert not np.array_equal(old[1], weight)
    sc_kit.upload(r, sc)
    _eq(r.lift_features(V[None], K[None], W, H, img, feature_scale=scale), *old)
    r.set_group_poses(Rt)
    _eq(r.lift_features(V[None], K[None], W, H, img, feature_scale=scale), sums, weight)


# ---- 5. errors leave the context usable ------------------------------------------------------------------------------------------------
def _raw(r, V, K, W, H, img, C, scale=1.0, mask=None, flags=0, sums=True, weight=True, n_views=1):
    L = _capi.lib()
    Vc, Kc = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(K, np.float32)
    s = torch.zeros((max(r.n, 1), max(min(C, 256), 1)), dtype=torch.int64, device="cuda")
    w = torch.zeros(max(r.n, 1), dtype=torch.int64, device="cuda")
    rc = L.sas_lift_features(r._ctx, n_views, Vc.ctypes.data, Kc.ctypes.data, W, H, img.data_ptr() if img is not None else None, C, scale,
                             mask.data_ptr() if mask is not None else None, flags, s.data_ptr() if sums else None,
                             w.data_ptr() if weight else None, None)
    torch.cuda.synchronize()
    return rc, L.sas_last_error(r._ctx).decode(), s, w


def test_errors_leave_the_context_usable():
    from sim_a_splat_amd.rasterizer import Rasterizer
    sc, cam, w = _small((32, 32))
    V, K, W, H = cam
    img_np, scale = _features((W, H), 3)
    img = torch.from_numpy(img_np).cuda()
    sums, weight = fr.sums(w, img_np[0], scale)
    r = Rasterizer(0)                                          # a context of its own: "before an upload" needs a fresh one
    try:
        rc, msg, _, _ = _raw(r, V, K, W, H, img, 3)
        assert rc == -3 and "sas_scene_upload" in msg, (rc, msg)                  # SAS_ERR_NO_SCENE
        sc_kit.upload(r, sc)

        def valid():
            _eq(r.lift_features(V[None], K[None], W, H, img, feature_scale=scale), sums, weight)
        valid()
        for C in (0, 257, -1):
            rc, msg, s, wt = _raw(r, V, K, W, H, img, C)
            assert rc == -1 and "channels" in msg and not s.any() and not wt.any(), (C, rc, msg)   # SAS_ERR_INVALID, nothing added
            valid()
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            rc, msg, s, wt = _raw(r, V, K, W, H, img, 3, scale=bad)
            assert rc == -1 and "feature_scale" in msg and not s.any() and not wt.any(), (bad, rc, msg)
            valid()
        for kw, word in ((dict(sums=False, weight=False), "NULL"), (dict(flags=_capi.SAS_ASYNC), "flags"), (dict(flags=_capi.SAS_FULL_SORT), "flags"),
                         (dict(flags=_capi.SAS_DEPTH_FILL_MAX), "flags"), (dict(n_views=0), "n_views")):
            rc, msg, s, wt = _raw(r, V, K, W, H, img, 3, **kw)
            assert rc == -1 and word in msg and not s.any() and not wt.any(), (kw, rc, msg)
            valid()
        rc, msg, _, _ = _raw(r, V, K, W, H, None, 3)
        assert rc == -1 and "images" in msg, (rc, msg)
        rc, msg, _, _ = _raw(r, V, K, 0, H, img, 3)
        assert rc == -1 and "size" in msg, (rc, msg)
        rc, msg, _, _ = _raw(r, V, K, W, -4, img, 3)
        assert rc == -1 and "size" in msg, (rc, msg)
        valid()
        # a context that holds meshes: occlusion by meshes is not lifted
        r.upload_meshes(np.array([[-1.0, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]], np.float32), np.array([[0, 1, 2]]), np.array([0.5, 0.5, 0.5], np.float32))
        with pytest.raises(SasError, match="clear the meshes first"):
            r.lift_features(V[None], K[None], W, H, img)
        r.clear_meshes()
        valid()
        # fast exponential: accepted (no bits are promised for v_exp_f32)
        fast = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale, fast_exp=True)
        assert int(fast["weight"].sum()) > 0 and bool((fast["sums"].abs() <= 32767 * fast["weight"][:, None]).all())
        valid()
    finally:
        r.close()


# ---- 6. round trip: feature frames lifted back give every Gaussian its own cluster's embedding -----------------------------------------
def test_two_clusters_round_trip(rasterizer):
    r = rasterizer
    sc = lr.two_clusters()
    cam = sc_kit.ring(64, 64, f=64.0, yaw=0.0, elev=0.0)
    V, K, W, H = cam
    left = np.arange(200) < 100
    emb = np.where(left[:, None], np.array([[1.0, 0.0]], np.float32), np.array([[0.0, 1.0]], np.float32)).astype(np.float32)
    sc_kit.upload(r, sc)
    r.upload_features(emb)
    views = r.render_features(V, K, W, H, want=("features",))["features"][None]   # [1,H,W,2], zero background
    assert bool((views[..., 0] * views[..., 1] == 0).all())                        # the footprints share no pixel
    got = r.lift_features(V[None], K[None], W, H, views)
    f, seen = features_from_sums(got["sums"], got["weight"], got["feature_scale"])
    f, seen = f.cpu().numpy(), seen.cpu().numpy()
    assert seen.sum() > 150 and f.dtype == np.float32 and (f[~seen] == 0).all()
    assert (f[seen & left, 1] == 0).all() and (f[seen & left, 0] > 0).all()
    assert (f[seen & ~left, 0] == 0).all() and (f[seen & ~left, 1] > 0).all()
    rel = relevancy(torch.from_numpy(f), emb[[0, 199]], np.array([[-1.0, -1.0]], np.float32))
    m = masks_from_relevancy(rel, ["left", "right"], seen=seen)
    assert np.array_equal(m["left"], seen & left) and np.array_equal(m["right"], seen & ~left)
    # and the exact sums, from the oracle's weights
    rs, rw = fr.reference(sc, cam, views[0].cpu().numpy(), got["feature_scale"])
    _eq(got, rs, rw)


# ---- 7. what the integers mean: the weighted mean feature ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_features_from_sums_against_the_float64_mean(rasterizer, size):
    """|features - sum vis f / sum vis| <= 0.5 / scale + 2 max|f| n 2^-24 / w per Gaussian, n its contributing pixels, w = sum vis: fq is
    within 0.5 of f scale (nothing saturates: scale = 32767 / max|f|), and each of the n weights loses less than 2^-24 to the floor, which
    moves numerator and denominator by at most max|f| n 2^-24 and n 2^-24 against w.  On the CPU reference the error is at most 0.64
    of the bound on these cases (0.60, 0.63, 0.57)."""
    r = rasterizer
    sc, cam, w = _small(size)
    V, K, W, H = cam
    img, scale = _features(size, 17)
    mean, tot, n = fr.float_mean(w, img[0])
    sc_kit.upload(r, sc)
    got = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale)
    f, seen = features_from_sums(got["sums"], got["weight"], scale)
    assert bool(seen.all()) and (tot > 0).all()
    bound = 0.5 / scale + 2.0 * float(np.abs(img).max()) * n * 2.0 ** -24 / tot
    err = np.abs(f.cpu().numpy().astype(np.float64) - mean)
    print(f"{size}: largest error / bound {float((err / bound[:, None]).max()):.3f}")
    assert (err <= bound[:, None]).all()


# ---- 8. Door A: compute_semantics --------------------------------------------------------------------------------------------------------
def test_door_a_compute_semantics():
    from sim_a_splat_amd.gaussian_splat import GaussianSplat, PinholeCamera, SplatModel, viewmat_from_c2w_opengl
    from sim_a_splat_amd.synthetic import c2w_opengl_from_viewmat
    rng = np.random.default_rng(2)
    n, W, H, D = 300, 40, 24, 5
    model = SplatModel(rng.normal(0, 0.4, (n, 3)), np.log(rng.uniform(0.05, 0.15, (n, 3))), rng.normal(size=(n, 4)), rng.normal(size=(n, 3)),
                       rng.normal(0, 0.1, (n, 15, 3)), rng.normal(0.5, 1.5, (n, 1)))
    cams = [sc_kit.ring(W, H, f=20.0, yaw=y, elev=0.1) for y in (0.0, 120.0, 240.0)]
    poses = [c2w_opengl_from_viewmat(c[0]) for c in cams]
    gs = GaussianSplat.from_model(model, PinholeCamera(torch.from_numpy(poses[0][:3]), 20.0, 20.0, W / 2, H / 2, W, H))
    r = model._rasterizer()
    try:
        plain = gs.render(poses[1])
        cameras = gs.cameras[0]
        with pytest.raises(TypeError, match="compute_semantics is not supported by a splatfacto model"):
            model.get_outputs_for_camera(cameras, compute_semantics=True)
        assert set(gs.render(poses[1], compute_semantics=True)) == set(plain)         # the reference's retry: the plain outputs
        # embeddings lifted from feature images of three views
        img = rng.normal(size=(3, H, W, D)).astype(np.float32)
        mask = rng.uniform(size=(3, H, W)) < 0.9
        got = gs.lift_features(poses, img, mask=mask, views_per_call=2)
        Vs, Ks = np.stack([viewmat_from_c2w_opengl(p[:3]) for p in poses]), np.stack([cams[0][1]] * 3)
        want = r.lift_features(Vs, Ks, W, H, img, mask=mask)
        assert got["feature_scale"] == want["feature_scale"] == fr.auto_scale(img)
        assert torch.equal(got["sums"], want["sums"]) and torch.equal(got["weight"], want["weight"]) and got["sums"].shape == (n, D)
        emb, seen = features_from_sums(got["sums"], got["weight"], got["feature_scale"])
        assert int(seen.sum()) > 100
        model.set_clip_embeds(emb)
        with pytest.raises(ValueError, match="set_language_queries"):
            gs.render(poses[1], compute_semantics=True)
        pos, neg = rng.normal(size=(2, D)).astype(np.float32), rng.normal(size=(3, D)).astype(np.float32)
        gs.set_language_queries(pos, neg)
        out = gs.render(poses[1], compute_semantics=True)
        assert set(out) == set(plain) | {"relevancy", "clip"} and out["relevancy"].shape == (H, W, 2) and out["clip"].shape == (H, W, D)
        assert all(torch.equal(out[k], plain[k]) for k in plain)
        rel = relevancy(emb, pos, neg)
        assert torch.equal(gs.get_semantic_point_cloud(pos, neg).cpu(), rel.cpu())
        V1 = viewmat_from_c2w_opengl(poses[1][:3])
        for key, rows in (("relevancy", rel), ("clip", emb)):
            r.upload_features(rows)
            assert torch.equal(out[key], r.render_features(V1, cams[0][1], W, H, want=("features",))["features"]), key
        assert float(out["relevancy"].max()) > 0.0
    finally:
        r.close()


# ---- 9. drawn cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ff.SUITE_SEEDS)
def test_drawn_cases_equal_their_references(rasterizer, seed):
    assert len(ff.SUITE_SEEDS) == 40
    c = ff.draw_case(seed)
    diffs = ff.run_case(rasterizer, c)
    assert not diffs, (ff.describe(c), diffs)


# ---- last: the bounds-checked build -------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above (the dense case's among them) was
    range-checked: none was out of range.  (The product library has no counter, and nothing to read.)"""
    r = rasterizer
    sc, cam = _dense()
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    img, scale = _features((W, H), 256)
    got = r.lift_features(V[None], K[None], W, H, img, feature_scale=scale)
    assert int(got["weight"].sum()) > 0
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
