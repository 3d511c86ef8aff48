"""GPU: the host layer around the frames -- which stores a context holds after each upload call ("What forgets
what"), that contexts give back what they took, the triangles' feature rows through the one store body, and what each call that
changes the resident scene invalidates ("What a change of the resident scene invalidates").

Shapes: the 64-Gaussian twin fixture in 3 splat groups, 2 triangles behind the splats, 9 channels (two chunks), 32x32 frames.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_twin_fixture
from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError

pytestmark = pytest.mark.gpu
FMAX = np.float32(np.finfo(np.float32).max)
W = H = 32
C = 9


@functools.lru_cache(maxsize=None)
def _scene():
    """The shared inputs (never modified): the n64 fixture, Gaussian i in group i % 3, its camera at 32x32, and a quad of two triangles
    (groups 0 and 2) that fills the frame 40 units in front of the camera, behind every splat."""
    g = load_twin_fixture("n64")
    V = np.ascontiguousarray(g["viewmat"], np.float32)
    K = np.ascontiguousarray(g["K"], np.float32).copy()
    K[:2] *= 0.5                                           # the fixture's 64x64 camera at 32x32
    cam = np.array([[-40, -40, 40], [40, -40, 40], [40, 40, 40], [-40, 40, 40]], np.float64)
    verts = ((cam - V[:3, 3].astype(np.float64)) @ V[:3, :3].astype(np.float64)).astype(np.float32)   # R^T (p - t)
    rng = np.random.default_rng(64)
    return dict(means=g["means"], op=g["opacities"], sh=g["colors"], quats=g["quats"], scales=g["scales"],
                gid=(np.arange(64) % 3).astype(np.uint8), V=V, K=K, bg=np.ascontiguousarray(g["background"], np.float32),
                verts=verts, tris=np.array([[0, 1, 2], [0, 2, 3]], np.int32), cols=np.array([[1, 0, 0], [0, 0, 1]], np.float32),
                tgroups=np.array([0, 2], np.uint8), f=rng.uniform(0, 1, (64, C)).astype(np.float32),
                fm=rng.uniform(0, 1, (2, C)).astype(np.float32))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- 1. state transitions ----------------------------------------------------------------------------------------------------
# States: which stores the context holds -- S scene, F features, M meshes, X mesh features; "0": none.
STATES = ("0", "S", "SF", "SM", "SFM", "SFMX")
# NEXT[call][state] = (status of the call through the C ABI, state after it).  Written from the parent commit's sas_api.cpp:
#   scene -> features, meshes, mesh features;  features -> mesh features;  meshes -> mesh features
# and WHERE each call forgets: sas_scene_features drops X right after its scene check (a rejected call has dropped it),
# sas_scene_meshes drops X at entry and M only once validated (or for n_triangles == 0), sas_scene_mesh_features and
# sas_scene_upload validate first.  -3: SAS_ERR_NO_SCENE, -1: SAS_ERR_INVALID.
NEXT = {
    "upload":            {"0": (0, "S"), "S": (0, "S"), "SF": (0, "S"), "SM": (0, "S"), "SFM": (0, "S"), "SFMX": (0, "S")},
    "upload_bad":        {s: (-1, s) for s in STATES},
    "features":          {"0": (-3, "0"), "S": (0, "SF"), "SF": (0, "SF"), "SM": (0, "SFM"), "SFM": (0, "SFM"), "SFMX": (0, "SFM")},
    "features_bad":      {"0": (-3, "0"), "S": (-1, "S"), "SF": (-1, "SF"), "SM": (-1, "SM"), "SFM": (-1, "SFM"), "SFMX": (-1, "SFM")},
    "meshes":            {"0": (-3, "0"), "S": (0, "SM"), "SF": (0, "SFM"), "SM": (0, "SM"), "SFM": (0, "SFM"), "SFMX": (0, "SFM")},
    "meshes_bad":        {"0": (-3, "0"), "S": (-1, "S"), "SF": (-1, "SF"), "SM": (-1, "SM"), "SFM": (-1, "SFM"), "SFMX": (-1, "SFM")},
    "meshes_none":       {"0": (-3, "0"), "S": (0, "S"), "SF": (0, "SF"), "SM": (0, "S"), "SFM": (0, "SF"), "SFMX": (0, "SF")},
    "mesh_features":     {"0": (-3, "0"), "S": (-1, "S"), "SF": (-1, "SF"), "SM": (-1, "SM"), "SFM": (0, "SFMX"), "SFMX": (0, "SFMX")},
    "mesh_features_bad": {"0": (-3, "0"), "S": (-1, "S"), "SF": (-1, "SF"), "SM": (-1, "SM"), "SFM": (-1, "SFM"), "SFMX": (-1, "SFMX")},
}
# Through Rasterizer a call is refused exactly where NEXT has a status != 0, with one difference in what is left behind:
# upload_features turns a wrong array down itself (ValueError), so the library is not entered and keeps its mesh features.
NEXT_PY = {("features_bad", "SFMX"): "SFMX"}
# What a state answers: sas_render (status, do the meshes show), sas_render_features (status, what sas_last_error names),
# Rasterizer.render_group_masks (accepted?  It sets the one-hot stores itself: only a context without a scene refuses).
ANSWERS = {
    "0":    dict(render=(-3, False), features=(-3, "scene"), masks=False),
    "S":    dict(render=(0, False), features=(-1, "no features"), masks=True),
    "SF":   dict(render=(0, False), features=(0, ""), masks=True),
    "SM":   dict(render=(0, True), features=(-1, "no features"), masks=True),
    "SFM":  dict(render=(0, True), features=(-1, "meshes"), masks=True),
    "SFMX": dict(render=(0, True), features=(0, ""), masks=True),
}
BUILD = {"0": (), "S": ("upload",), "SF": ("upload", "features"), "SM": ("upload", "meshes"), "SFM": ("upload", "features", "meshes"),
         "SFMX": ("upload", "features", "meshes", "mesh_features")}


def _c_call(L, ctx, call):
    """One upload call through the C ABI, accepted by its own validation or ("_bad") rejected by it."""
    s = _scene()
    if call.startswith("upload"):
        return L.sas_scene_upload(ctx, 64, _p(s["means"]), _p(s["quats"]), _p(s["scales"]), None, _p(s["op"]), _p(s["sh"]), 3,
                                  _p(s["gid"]), 300 if call.endswith("_bad") else 3)
    if call.startswith("features"):
        return L.sas_scene_features(ctx, 64, 0 if call.endswith("_bad") else C, _p(s["f"]))
    if call == "meshes_none":
        return L.sas_scene_meshes(ctx, 0, None, 0, None, None, None, 0.4, 0.6)
    if call.startswith("meshes"):
        return L.sas_scene_meshes(ctx, 4, _p(s["verts"]), 2, _p(s["tris"]), _p(s["cols"]), _p(s["tgroups"]),
                                  float("nan") if call.endswith("_bad") else 1.0, 0.0)
    return L.sas_scene_mesh_features(ctx, 2, C + 1 if call.endswith("_bad") else C, _p(s["fm"]))


def _py_call(r, call):
    """The same through Rasterizer: 0, or the status NEXT would show for the refusal (any non-zero: only refused / accepted is held)."""
    s = _scene()
    try:
        if call.startswith("upload"):
            r.upload(s["means"], s["op"], s["sh"], quats=s["quats"], scales=s["scales"], sh_degree=3, group_id=s["gid"],
                     n_groups=300 if call.endswith("_bad") else 3)
        elif call.startswith("features"):
            r.upload_features(s["f"][:-1] if call.endswith("_bad") else s["f"])
        elif call == "meshes_none":
            r.clear_meshes()
        elif call.startswith("meshes"):
            r.upload_meshes(s["verts"], s["tris"], s["cols"], groups=s["tgroups"], ambient=float("nan") if call.endswith("_bad") else 1.0,
                            diffuse=0.0)
        else:
            r.upload_mesh_features(s["fm"][:, :-1] if call.endswith("_bad") else s["fm"])
    except (SasError, ValueError):
        return -1
    return 0


def _c_answers(L, ctx, bufs):
    """(render, features) of ANSWERS as the library answers them for this context; neither call changes a store."""
    s = _scene()
    rgb, alpha, feat = bufs
    rc = L.sas_render(ctx, _p(s["V"]), _p(s["K"]), W, H, _p(s["bg"]), 0, rgb.data_ptr(), alpha.data_ptr(), None, None, None)
    shows = False
    if rc == 0:
        torch.cuda.synchronize()
        empty = alpha[..., 0] == 0                         # no splat: the background, or the quad behind the splats
        assert bool(empty.any())
        shows = not bool((rgb[empty] == torch.from_numpy(s["bg"]).to(rgb.device)).all())
    rf = L.sas_render_features(ctx, _p(s["V"]), _p(s["K"]), W, H, None, None, 0, None, None, None, feat.data_ptr(), None)
    msg = L.sas_last_error(ctx).decode() if rf else ""
    names = "scene" if "before sas_scene_upload" in msg else "no features" if "no features set" in msg else "meshes" if "meshes" in msg else msg
    return (rc, shows), (rf, names)


def _accepts(fn):
    try:
        fn()
    except (SasError, ValueError):
        return False
    return True


@pytest.mark.parametrize("door", ["c_abi", "rasterizer"])
def test_state_transitions(door):
    """From every reachable state, every upload call once accepted and once rejected by its own validation (and sas_scene_meshes
    once more with no triangles): the call's status, and the state it leaves, told by what render / render_features / render_group_masks
    answer.  Through Rasterizer the library beneath is asked as well: the mirror refuses exactly when the library does."""
    L = _capi.lib()
    s = _scene()
    bufs = (torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 1), device="cuda"), torch.empty((H, W, C), device="cuda"))
    shared = Rasterizer(0)                                 # (every state but "0" starts with an upload, which forgets everything)
    try:
        for state in STATES:
            for call, row in NEXT.items():
                r = Rasterizer(0) if state == "0" else shared
                try:
                    ctx = r._ctx
                    for step in BUILD[state]:
                        assert (_c_call(L, ctx, step) if door == "c_abi" else _py_call(r, step)) == 0, (state, step)
                    status, after = row[state]
                    got = _c_call(L, ctx, call) if door == "c_abi" else _py_call(r, call)
                    where = (door, state, call)
                    if door == "c_abi":
                        assert got == status, where
                    else:
                        assert (got == 0) == (status == 0), where
                        after = NEXT_PY.get((call, state), after)
                    want = ANSWERS[after]
                    render, feats = _c_answers(L, ctx, bufs)
                    assert render == want["render"] and feats == want["features"], (where, after, render, feats)
                    if door == "rasterizer":
                        assert _accepts(lambda: r.render(s["V"], s["K"], W, H, s["bg"], want=("rgb",))) == (want["render"][0] == 0), where
                        assert _accepts(lambda: r.render_features(s["V"], s["K"], W, H)) == (want["features"][0] == 0), where
                        assert _accepts(lambda: r.render_group_masks(s["V"], s["K"], W, H)) == want["masks"], where
                        if want["masks"]:                  # ... and it has left both one-hot stores behind, in the library too
                            assert _c_answers(L, ctx, bufs[:2] + (torch.empty((H, W, 3), device="cuda"),))[1] == (0, ""), where
                finally:
                    if r is not shared:
                        r.close()
    finally:
        shared.close()


# ---- 2. lifetime -------------------------------------------------------------------------------------------------------------
GRANULE = 2 << 20          # what the device allocator hands out at the least: the resolution of mem_get_info for this purpose
PARENT_DROP = 0            # bytes; see test_contexts_give_back_what_they_took


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _round(wait=True):
    """One context through every store and every kind of frame, so that every buffer of its slots exists; then close()."""
    s = _scene()
    V, K, bg = s["V"], s["K"], s["bg"]
    r = Rasterizer(0)
    try:
        assert _py_call(r, "upload") == 0 and _py_call(r, "features") == 0 and _py_call(r, "meshes") == 0 and _py_call(r, "mesh_features") == 0
        if wait:
            r.render(V, K, W, H, bg)
            r.render_rgbd(V, K, W, H, bg)
            r.render_features(V, K, W, H, bg)
            r.render_batch(np.stack([V] * 4), np.stack([K] * 4), W, H, bg, want=("rgb", "depth"))
            r.render_batch_host(np.stack([V] * 2), np.stack([K] * 2), W, H, bg)
        out = [r.render(V, K, W, H, bg, block=False) for _ in range(1 if wait else 3)]
        if wait:
            r.wait()
    finally:
        r.close()
    del out


def test_contexts_give_back_what_they_took():
    """12 rounds of create / upload everything / one frame of every kind / close: the device's free memory after round 12 against
    after round 2 (the first rounds fill torch's caching allocator and the runtime's pools).

    Measured on an MI355X, three runs each: the parent commit (hand-kept release lists) drops 0, 0, 0 bytes; this tree (owners)
    0, 0, 0 bytes.  The bound is the parent's drop plus one allocation granule.  mem_get_info sees whole granules only: a leak of
    a few bytes, an event or a stream does not show here -- that each of the four runtime calls that give something back is
    written once, inside its owner, is what covers those."""
    _round()
    _round()
    before = _free_bytes()
    for _ in range(10):
        _round()
    drop = before - _free_bytes()
    print(f"free memory after round 2: {before} bytes, drop after round 12: {drop} bytes")
    assert drop <= PARENT_DROP + GRANULE, drop


def test_a_context_destroyed_with_frames_in_flight_comes_back_clean():
    _round(wait=False)
    _round(wait=False)
    before = _free_bytes()
    for _ in range(4):
        _round(wait=False)
    drop = before - _free_bytes()
    print(f"in flight at close: drop {drop} bytes")
    assert drop <= PARENT_DROP + GRANULE, drop


# ---- 3. poisoned triangle rows -----------------------------------------------------------------------------------------------
def test_poisoned_mesh_features_render_as_their_finite_mapping(rasterizer):
    """NaN and +-Inf in upload_mesh_features rows come out as the colours' finite mapping (NaN -> -FLT_MAX, +-Inf -> +-FLT_MAX): the
    frame is the frame of the mapped rows bit for bit, and where a triangle shows under zero splat alpha the pixel IS the mapped
    row (F = 0 + (1 - 0) m).  Mirrors test_poisoned_features_render_as_their_finite_mapping for the triangles' rows."""
    s = _scene()
    fm = s["fm"].copy()
    fm[0, [0, 4, 8]] = [np.nan, np.inf, -np.inf]           # both chunks of both rows
    fm[1, [1, 7, 8]] = [-np.inf, np.nan, np.inf]
    mapped = np.where(np.isnan(fm), -FMAX, np.clip(fm, -FMAX, FMAX)).astype(np.float32)
    assert _py_call(rasterizer, "upload") == 0 and _py_call(rasterizer, "features") == 0 and _py_call(rasterizer, "meshes") == 0

    def frame(rows):
        rasterizer.upload_mesh_features(rows)
        o = rasterizer.render_features(s["V"], s["K"], W, H, s["bg"], want=("features", "alpha"))
        return o["features"].cpu().numpy(), o["alpha"].cpu().numpy()[..., 0]

    a, alpha = frame(fm)
    b, _ = frame(mapped)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c, _ = frame(torch.from_numpy(fm).cuda())              # device-resident rows take the same path
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    bare = a[alpha == 0]                                   # no splat in front: the triangle's row as it was stored
    rows = [(bare.view(np.uint32) == mapped[t].view(np.uint32)).all(-1) for t in (0, 1)]
    assert rows[0].any() and rows[1].any() and (rows[0] | rows[1]).all(), (len(bare), int(rows[0].sum()), int(rows[1].sum()))


# ---- 4. what a change of the resident scene invalidates ----------------------------------------------------------------------
# Start: scene and features uploaded, the last frame a render_backward frame (its sums in the context).  One call is applied, then
# the context is asked, in this order (the first three change nothing, the last renders a frame): sas_read_projection,
# sas_read_tile_lists, sas_density_accumulate without d_means2d (the scratch path), sas_render_features.  INVALIDATES[call] = their
# (status, words of sas_last_error), written from the parent commit's sas_api.cpp:
#   a step that moves something and an opacity reset change VALUES: the last frame and its backward status go, the stores stay;
#   densify changes COUNT AND ORDER: the features go as well;  upload changes EVERYTHING: every store beside the scene goes;
#   a step whose rates are all zero returns before it touches anything;  adam_reset, density_accumulate and photometric_loss do not
#   touch the scene.
OK = (0, "")
NO_FRAME = (-3, "no frame rendered")
NO_BACKWARD = (-3, "no backward frame since the last upload, optimiser step, densify or opacity reset")
NO_FEATURES = (-1, "no features set for this scene")
INVALIDATES = {
    "adam_step":          (NO_FRAME, NO_FRAME, NO_BACKWARD, OK),
    "adam_step_zero":     (OK, OK, OK, OK),
    "adam_reset":         (OK, OK, OK, OK),
    "density_accumulate": (OK, OK, OK, OK),
    "reset_opacity":      (NO_FRAME, NO_FRAME, NO_BACKWARD, OK),
    "densify_off":        (NO_FRAME, NO_FRAME, NO_BACKWARD, NO_FEATURES),
    "upload":             (NO_FRAME, NO_FRAME, NO_BACKWARD, NO_FEATURES),
    "photometric_loss":   (OK, OK, OK, OK),
}


def _backward_start(r):
    """The section's start on ``r``; returns the backward frame's gradients (what adam_step takes)."""
    s = _scene()
    assert _py_call(r, "upload") == 0 and _py_call(r, "features") == 0
    return r.render_backward(s["V"], s["K"], W, H, g_rgb=np.ones((H, W, 3), np.float32))


def _stats(r, grad=0.0, count=0):
    return dict(grad_sum=torch.full((r.n,), grad, device=r.device), count=torch.full((r.n,), count, dtype=torch.int32, device=r.device))


def _change(r, call, grads):
    if call == "adam_step":
        r.adam_step(grads, dict(opacities=5e-2, sh_dc=1e-2, sh_rest=1e-2, scales=5e-3), 1)
    elif call == "adam_step_zero":
        r.adam_step(grads, {}, 1)
    elif call == "adam_reset":
        r.adam_reset()
    elif call == "density_accumulate":
        r.density_accumulate(W, H, _stats(r))
    elif call == "reset_opacity":
        r.reset_opacity(0.01)
    elif call == "densify_off":
        r.densify(_stats(r), grow=False, prune_opacity_on=False, prune_scale_on=False)
    elif call == "densify":
        return r.densify(_stats(r, 1.0, 1), prune_opacity_on=False, prune_scale_on=False, seed=7)
    elif call == "upload":
        assert _py_call(r, "upload") == 0
    else:
        assert call == "photometric_loss", call
        rgb = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(4))
        r.photometric_loss(rgb, 1.0 - rgb)


def _asked(L, r):
    """The four answers of INVALIDATES as the library gives them now."""
    s = _scene()
    ctx = r._ctx
    off, ids = np.zeros(257, np.int32), np.zeros(1 << 16, np.int32)   # (16 tiles of 8 pixels at the most; 64 Gaussians reach far fewer)
    st = _stats(r)
    feat = torch.empty((H, W, C), device=r.device)
    asks = (lambda: L.sas_read_projection(ctx, None, None, None, None, None),
            lambda: L.sas_read_tile_lists(ctx, _p(off), _p(ids), ids.size),
            lambda: L.sas_density_accumulate(ctx, W, H, None, st["grad_sum"].data_ptr(), st["count"].data_ptr(), None, r._stream()),
            lambda: L.sas_render_features(ctx, _p(s["V"]), _p(s["K"]), W, H, None, None, 0, None, None, None, feat.data_ptr(), None))
    got = []
    for ask in asks:
        rc = ask()
        got.append((rc, L.sas_last_error(ctx).decode() if rc else ""))
    torch.cuda.synchronize()
    return got


def test_what_a_change_of_the_resident_scene_invalidates():
    L = _capi.lib()
    r = Rasterizer(0)                                      # (every start begins with an upload, which forgets everything)
    try:
        for call, want in INVALIDATES.items():
            _change(r, call, _backward_start(r))
            got = _asked(L, r)
            for (rc, msg), (status, words) in zip(got, want):
                assert rc == status and words in msg, (call, got)
    finally:
        r.close()


@pytest.mark.parametrize("call", ["adam_step", "reset_opacity", "densify"])
def test_a_frame_straight_behind_a_change_shows_the_changed_scene(call):
    """The order promise of the three calls that change values: a render enqueued straight behind the call, with no wait in between,
    is the frame of the changed scene -- bit for bit the frame of a fresh context uploaded read_scene's arrays.  (The step moves no
    mean and densify's storage order is the upload's, so both contexts hold the same planes.)  tests/test_gpu_u_fit.py::
    test_planes_stay_well_formed and tests/test_gpu_w_densify.py hold the same equality behind a read_scene, which waits."""
    s = _scene()
    outs = ("rgb", "alpha", "depth")
    frame = lambda q: {k: v.cpu().numpy() for k, v in q.render(s["V"], s["K"], W, H, s["bg"], want=outs).items()}
    r, fresh = Rasterizer(0), Rasterizer(0)
    try:
        assert _py_call(r, "upload") == 0
        before = frame(r)
        grads = _backward_start(r)
        torch.cuda.synchronize()
        res = _change(r, call, grads)
        a = frame(r)
        x = r.read_scene()
        gid = s["gid"] if res is None else s["gid"][res["parents"].cpu().numpy()]
        assert r.n == (64 if res is None else res["n"]) and (res is None or res["n"] > 64)
        fresh.upload(x["means"], x["opacities"], x["colors"], quats=x["quats"], scales=x["scales"], sh_degree=3, group_id=gid, n_groups=3)
        b = frame(fresh)
        for k in outs:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (call, k)
        assert not np.array_equal(a["rgb"], before["rgb"]), call
    finally:
        r.close()
        fresh.close()
