"""GPU: label lifting (sas_lift_labels; DESIGN.md 3, "Label lifting"), the transpose of a label frame.

Every comparison is exact int64 equality against tests/tools/lift_ref.py: the weights of the C oracle's one-hot frames (or, for the
dense scene, of render_features with explicit one-hot features), quantised and summed in numpy.  Integer sums have no order, so there
is nothing to tolerate.  Every test fails without the feature (no symbol, no method).  The file runs unchanged under the bounds-checked
build.
"""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import LIFT_ONE, SasError
from sim_a_splat_amd.segment import lift_label_views, masks_from_votes

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import lift_ref as lr  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (40, 24), (17, 33)]   # whole tiles; ragged in both axes (tiles of 8 columns, of 8 rows, of 1 column, of 1 row)


def _labels(W, H, G, seed, views=1):
    """Random over {0..G-1, 255}, one pixel in eight unlabelled."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, G, size=(views, H, W)).astype(np.uint8)
    lab[rng.uniform(size=lab.shape) < 0.125] = 255
    return lab


@functools.lru_cache(maxsize=None)
def _small(size):
    """The 64-Gaussian scene in 3 posed groups, its camera and its weights [64,H,W] from the oracle (once per size)."""
    W, H = size
    sc = lr.blob_scene(64, 11, 0.12, n_groups=3)
    cam = sc_kit.ring(W, H, f=0.45 * max(W, H))
    return sc, cam, lr.weights_oracle(sc, cam)


def _eq(got, votes, seen):
    v, s = got["votes"].cpu().numpy(), got["seen"].cpu().numpy()
    assert v.dtype == np.int64 and s.dtype == np.int64 and v.shape == votes.shape and s.shape == seen.shape
    assert np.array_equal(s, seen), (int((s != seen).sum()), np.abs(s - seen).max())
    assert np.array_equal(v, votes), (int((v != votes).sum()), np.abs(v - votes).max())


# ---- 1. sizes and label counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 256])
@pytest.mark.parametrize("size", SIZES)
def test_sizes_and_label_counts(rasterizer, size, G):
    r = rasterizer
    sc, cam, w = _small(size)
    V, K, W, H = cam
    lab = _labels(W, H, G, 100 + G)
    votes, seen = lr.sums(w, lab[0], G)
    assert (seen > 0).sum() >= 60 and (votes > 0).any(axis=0).sum() >= min(G, 3)
    assert votes.sum() < seen.sum() if G < 256 else votes.sum() == seen.sum()   # 255 is unlabelled unless the call counts 256 labels
    sc_kit.upload(r, sc)
    got = r.lift_labels(V[None], K[None], W, H, lab, G)
    assert got["votes"].shape == (64, G) and got["seen"].shape == (64,) and got["votes"].is_cuda
    _eq(got, votes, seen)
    assert LIFT_ONE == 2 ** 32 and int(got["seen"].max()) > LIFT_ONE        # more than one pixel's worth somewhere


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
    # (a property of the case, not of the code under test: a pixel left with T within 2e-4 has all but surely met the T' <= 1e-4 stop)
    stopped = 1.0 - alpha <= 2e-4
    print(f"dense: lists of {lens.min()}..{lens.max()} entries, {int(stopped.sum())} of {W * H} pixels at T <= 2e-4")
    assert lens.min() > 1024 and stopped.sum() > 100           # four batches and more per tile; the stop is exercised
    lab = _labels(W, H, 3, 5)
    votes, seen = lr.sums(w, lab[0], 3)
    got = r.lift_labels(V[None], K[None], W, H, lab, 3)
    _eq(got, votes, seen)
    assert (seen == 0).sum() > 0                               # Gaussians wholly behind the stop, or never passing the alpha test
    # the stopping entry and the tail are absent: what the Gaussians were given at a pixel sums to that pixel's alpha = 1 - T, no more
    # (T falls by each weight with one float32 rounding, a weight loses < 2^-32 to the floor: < 1300 * 2^-24 < 1e-4 per pixel)
    assert abs(float(seen.sum()) / LIFT_ONE - float(alpha.astype(np.float64).sum())) < 1e-4 * alpha.size


# ---- 3. accumulation ----------------------------------------------------------------------------------------------------------------------
def test_accumulation_over_views_and_calls(rasterizer):
    r = rasterizer
    sc, cam, _ = _small((40, 24))
    V, K, W, H = cam
    cam2 = sc_kit.ring(W, H, f=0.45 * W, yaw=70.0, elev=0.4)
    Vs, Ks = np.stack([V, cam2[0]]), np.stack([K, cam2[1]])
    lab = _labels(W, H, 3, 9, views=2)
    refs = [lr.sums(lr.weights_oracle(sc, c), lab[k], 3) for k, c in enumerate((cam, cam2))]
    votes, seen = refs[0][0] + refs[1][0], refs[0][1] + refs[1][1]
    assert not np.array_equal(refs[0][1], refs[1][1])
    sc_kit.upload(r, sc)
    both = r.lift_labels(Vs, Ks, W, H, lab, 3)                                   # two views in one call
    _eq(both, votes, seen)
    acc = r.lift_labels(Vs[:1], Ks[:1], W, H, lab[:1], 3)                        # ... equal two calls into the same buffers
    same = r.lift_labels(Vs[1:], Ks[1:], W, H, lab[1:], 3, votes=acc["votes"], seen=acc["seen"])
    assert same["votes"].data_ptr() == acc["votes"].data_ptr() and same["seen"].data_ptr() == acc["seen"].data_ptr()
    _eq(acc, votes, seen)
    a, b = r.lift_labels(Vs[:1], Ks[:1], W, H, lab[:1], 3), r.lift_labels(Vs[1:], Ks[1:], W, H, lab[1:], 3)   # ... equal the sum of two fresh buffers
    _eq({"votes": a["votes"] + b["votes"], "seen": a["seen"] + b["seen"]}, votes, seen)
    again = r.lift_labels(Vs, Ks, W, H, lab, 3)                                  # the same call again on zeroed buffers: the same bits
    assert torch.equal(again["votes"], both["votes"]) and torch.equal(again["seen"], both["seen"])
    loop = lift_label_views(r, Vs, Ks, W, H, lab, 3, views_per_call=1)           # the loop over a list of views
    assert torch.equal(loop["votes"], both["votes"]) and torch.equal(loop["seen"], both["seen"])
    loop = lift_label_views(r, Vs, Ks, W, H, [lab[0], torch.from_numpy(lab[1])], 3)
    assert torch.equal(loop["votes"], both["votes"]) and torch.equal(loop["seen"], both["seen"])


# ---- 4. one output alone -------------------------------------------------------------------------------------------------------------------
def test_votes_alone_and_seen_alone(rasterizer):
    r = rasterizer
    sc, cam, w = _small((17, 33))
    V, K, W, H = cam
    lab = _labels(W, H, 3, 21)
    votes, seen = lr.sums(w, lab[0], 3)
    sc_kit.upload(r, sc)
    only_seen = r.lift_labels(V[None], K[None], W, H, lab, 3, votes=False)
    only_votes = r.lift_labels(V[None], K[None], W, H, torch.from_numpy(lab).cuda(), 3, seen=False)
    assert set(only_seen) == {"seen"} and set(only_votes) == {"votes"}
    _eq({"votes": only_votes["votes"], "seen": only_seen["seen"]}, votes, seen)
    with pytest.raises(ValueError):
        r.lift_labels(V[None], K[None], W, H, lab, 3, votes=False, seen=False)
    with pytest.raises(ValueError):
        r.lift_labels(V[None], K[None], W, H, lab, 3, seen=torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        r.lift_labels(V[None], K[None], W, H, lab[:, :-1], 3)


# ---- 5. group poses -----------------------------------------------------------------------------------------------------------------------
def test_votes_follow_the_group_poses(rasterizer):
    r = rasterizer
    sc, cam, w0 = _small((32, 32))
    V, K, W, H = cam
    Rt = np.asarray(sc["Rt"], np.float32).reshape(3, 12).copy()
    Rt[1, 3] += 0.35
    Rt[2, 7] -= 0.3
    Rt[2, 11] += 0.2
    lab = _labels(W, H, 3, 33)
    votes, seen = lr.sums(lr.weights_oracle(sc, cam, Rt=Rt), lab[0], 3)
    old = lr.sums(w0, lab[0], 3)
    assert not np.array_equal(old[1], seen)
    sc_kit.upload(r, sc)
    _eq(r.lift_labels(V[None], K[None], W, H, lab, 3), *old)
    r.set_group_poses(Rt)
    _eq(r.lift_labels(V[None], K[None], W, H, lab, 3), votes, seen)


# ---- 6. separation: label frames lifted back give every Gaussian to its own cluster ---------------------------------------------------
def test_two_clusters_come_back_apart(rasterizer):
    r = rasterizer
    sc = lr.two_clusters()
    cam = sc_kit.ring(64, 64, f=64.0, yaw=0.0, elev=0.0)
    V, K, W, H = cam
    left = np.arange(200) < 100
    a = sc_kit.oracle_frame(sc, cam, (0.0, 0.0, 0.0), keep=left)["alpha"][..., 0]
    b = sc_kit.oracle_frame(sc, cam, (0.0, 0.0, 0.0), keep=~left)["alpha"][..., 0]
    assert (a > 0).sum() > 50 and (b > 0).sum() > 50 and not ((a > 0) & (b > 0)).any()   # the footprints share no pixel
    sc_kit.upload(r, sc)
    lab = r.render_batch_labels(V[None], K[None], W, H, min_alpha=0.0)["labels"]
    assert set(torch.unique(lab).tolist()) == {0, 1}           # min_alpha 0: every pixel is labelled, the empty ones 0
    got = r.lift_labels(V[None], K[None], W, H, lab, 2)
    votes, seen = got["votes"].cpu().numpy(), got["seen"].cpu().numpy()
    own = left.astype(int) ^ 1
    idx = np.arange(200)
    assert (votes[idx, 1 - own] == 0).all() and (votes[idx, own] <= seen).all()
    assert (votes[idx, own] == seen).all()                     # (no pixel is unlabelled here)
    m = masks_from_votes(votes, seen, ["left", "right"], min_share=0.0)
    vis = seen > 0
    assert vis.sum() > 150
    assert np.array_equal(m["left"], vis & left) and np.array_equal(m["right"], vis & ~left)
    # and the exact sums, from the oracle's weights
    rv, rs = lr.reference(sc, cam, lab[0].cpu().numpy(), 2)
    assert np.array_equal(votes, rv) and np.array_equal(seen, rs)


# ---- 7. errors leave the context usable ------------------------------------------------------------------------------------------------
def _raw(r, V, K, W, H, lab, G, flags=0, votes=True, seen=True, n_views=1):
    L = _capi.lib()
    Vc, Kc = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(K, np.float32)
    v = torch.zeros((max(r.n, 1), max(G, 1)), dtype=torch.int64, device="cuda")
    s = torch.zeros(max(r.n, 1), dtype=torch.int64, device="cuda")
    rc = L.sas_lift_labels(r._ctx, n_views, Vc.ctypes.data, Kc.ctypes.data, W, H, lab.data_ptr() if lab is not None else None, G, flags,
                           v.data_ptr() if votes else None, s.data_ptr() if seen else None, None)
    torch.cuda.synchronize()
    return rc, L.sas_last_error(r._ctx).decode(), v, s


def test_errors_leave_the_context_usable():
    from sim_a_splat_amd.rasterizer import Rasterizer
    sc, cam, w = _small((32, 32))
    V, K, W, H = cam
    lab_np = _labels(W, H, 3, 41)
    lab = torch.from_numpy(lab_np).cuda()
    votes, seen = lr.sums(w, lab_np[0], 3)
    r = Rasterizer(0)                                          # a context of its own: "before an upload" needs a fresh one
    try:
        rc, msg, _, _ = _raw(r, V, K, W, H, lab, 3)
        assert rc == -3 and "sas_scene_upload" in msg, (rc, msg)                  # SAS_ERR_NO_SCENE
        sc_kit.upload(r, sc)

        def valid():
            _eq(r.lift_labels(V[None], K[None], W, H, lab, 3), votes, seen)
        valid()
        for G in (0, 257):
            rc, msg, v, s = _raw(r, V, K, W, H, lab, G)
            assert rc == -1 and "n_labels" in msg and not v.any() and not s.any(), (G, rc, msg)   # SAS_ERR_INVALID, nothing added
            valid()
        for kw, word in ((dict(votes=False, seen=False), "NULL"), (dict(flags=_capi.SAS_ASYNC), "flags"), (dict(flags=_capi.SAS_FULL_SORT), "flags"),
                         (dict(n_views=0), "n_views")):
            rc, msg, v, s = _raw(r, V, K, W, H, lab, 3, **kw)
            assert rc == -1 and word in msg and not v.any() and not s.any(), (kw, rc, msg)
            valid()
        rc, msg, _, _ = _raw(r, V, K, W, H, None, 3)
        assert rc == -1 and "label" in msg, (rc, msg)
        rc, msg, _, _ = _raw(r, V, K, 0, H, lab, 3)
        assert rc == -1 and "size" in msg, (rc, msg)
        valid()
        # a context that holds meshes: occlusion by meshes is not lifted
        r.upload_meshes(np.array([[-1.0, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]], np.float32), np.array([[0, 1, 2]]), np.array([0.5, 0.5, 0.5], np.float32))
        with pytest.raises(SasError, match="clear the meshes first"):
            r.lift_labels(V[None], K[None], W, H, lab, 3)
        r.clear_meshes()
        valid()
        with pytest.raises(SasError):
            r.lift_labels(V[None], K[None], W, H, lab, 0)
        valid()
    finally:
        r.close()


# ---- 8. fast exponential: accepted (no bits are promised for v_exp_f32) ------------------------------------------------------------------
def test_fast_exp_is_accepted(rasterizer):
    r = rasterizer
    sc, cam, _ = _small((32, 32))
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    got = r.lift_labels(V[None], K[None], W, H, _labels(W, H, 3, 51), 3, fast_exp=True)
    assert int(got["seen"].sum()) > 0 and bool((got["votes"].sum(dim=1) <= got["seen"]).all())


# ---- 9. Door A: camera-to-world poses, camera 0's intrinsics ---------------------------------------------------------------------------
def test_gaussian_splat_lift_labels():
    from sim_a_splat_amd.gaussian_splat import GaussianSplat, PinholeCamera, SplatModel, viewmat_from_c2w_opengl
    from sim_a_splat_amd.synthetic import c2w_opengl_from_viewmat
    rng = np.random.default_rng(2)
    n, W, H = 300, 40, 24
    model = SplatModel(rng.normal(0, 0.4, (n, 3)), np.log(rng.uniform(0.05, 0.15, (n, 3))), rng.normal(size=(n, 4)), rng.normal(size=(n, 3)),
                       rng.normal(0, 0.1, (n, 15, 3)), rng.normal(0.5, 1.5, (n, 1)))
    cams = [sc_kit.ring(W, H, f=20.0, yaw=y, elev=0.1) for y in (0.0, 120.0, 240.0)]
    poses = [c2w_opengl_from_viewmat(c[0]) for c in cams]
    gs = GaussianSplat.from_model(model, PinholeCamera(torch.from_numpy(poses[0][:3]), 20.0, 20.0, W / 2, H / 2, W, H))
    lab = _labels(W, H, 2, 71, views=3)
    got = gs.lift_labels(poses, lab, 2, views_per_call=2)
    r = model._rasterizer()
    Vs, Ks = np.stack([viewmat_from_c2w_opengl(p[:3]) for p in poses]), np.stack([cams[0][1]] * 3)
    want = r.lift_labels(Vs, Ks, W, H, lab, 2)
    assert got["votes"].shape == (n, 2) and torch.equal(got["votes"], want["votes"]) and torch.equal(got["seen"], want["seen"])
    assert int((got["seen"] > 0).sum()) > 100
    r.close()


# ---- last: the bounds-checked build -------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above (the dense case's among them) was
    range-checked: none was out of range.  (The product library has no counter, and nothing to read.)"""
    r = rasterizer
    sc, cam = _dense()
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    r.lift_labels(V[None], K[None], W, H, _labels(W, H, 256, 61), 256)
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
