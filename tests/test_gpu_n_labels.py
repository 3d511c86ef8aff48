"""GPU: label frames (sas_render_batch_labels[_posed]; DESIGN.md 3, "Label frames").

The contract: labels[v,p] = L(w_v[p,:], a_v[p]) with w_v and a_v bit for bit what sas_render_features delivers for view v under that
view's poses (one-hot stores, zero feature background, SAS_MESH_SURFACE when the scene holds meshes) and L = rasterizer.group_labels.
The reference is therefore the earlier path on the same context -- per view set_group_poses + render_group_masks -- and every pixel
must be equal.  With meshes the labels are also held to the oracle (mesh_feature_cases.expected_labels) on the reference's stable
pixels, with the stability mask and the cap test_gpu_i_mesh_features.py uses for its label test (mesh_cases.MAX_EXCLUDED).  Every
test fails without the feature (no symbol, no method).  The file runs unchanged under the bounds-checked build.
"""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError, group_labels

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import mesh_feature_cases as mf  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu
DRAWN_SEEDS = (35, 50)   # oracle_fuzz.draw_mesh_case seeds with splat groups and a posed mesh: G = 40 (five chunks) and G = 3


def _parent_labels(r, V, K, W, H, Rt=None, min_alpha=0.5):
    """The earlier path: the view's poses set on the context, one feature frame, four torch kernels."""
    if Rt is not None:
        r.set_group_poses(Rt)
    return r.render_group_masks(V, K, W, H, min_alpha=min_alpha)


def _one(r, cam, **kw):
    V, K, W, H = cam
    return r.render_batch_labels(V[None], K[None], W, H, **kw)


# ---- 1. channel counts around the chunk edge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(96, 64), (100, 70)])
@pytest.mark.parametrize("G", [1, 7, 8, 9, 17])
def test_channel_counts_and_ragged_frames(rasterizer, G, size):
    r = rasterizer
    sc = sc_kit.synthetic(2000, 40 + G, 0.02, n_groups=G)
    cam = sc_kit.ring(size[0], size[1], f=40.0)
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    got = _one(r, cam)["labels"]
    assert got.shape == (1, H, W) and got.dtype == torch.uint8
    tw, th = (W + 15) // 16, (H + 15) // 16
    off = r.read_tile_lists(tw * th)["tile_offsets"]          # the label frame is a full-sort frame: its lists are the ones kept
    lens = np.diff(off)
    print(f"G={G} {W}x{H}: {tw * th} tiles, lists of {lens.min()}..{lens.max()} entries")
    assert (lens == 0).any(), lens                                              # a tile with an empty list
    want = _parent_labels(r, V, K, W, H)
    assert torch.equal(got[0], want["labels"]), int((got[0] != want["labels"]).sum())
    assert len(torch.unique(got)) >= min(G, 2)
    empty = np.nonzero(lens == 0)[0][0]
    ty, tx = divmod(int(empty), tw)
    assert (got[0, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] == 255).all()    # nothing there: alpha 0 < 0.5


# ---- 2. G = 256 --------------------------------------------------------------------------------------------------------------------------
def test_256_groups(rasterizer):
    r = rasterizer
    sc = sc_kit.synthetic(4000, 77, 0.03)
    sc = dict(sc, gid=(np.arange(4000) % 256).astype(np.uint8), G=256, Rt=sc_kit.random_group_poses(256, 78))
    cam = sc_kit.ring(96, 64, f=60.0)
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    for min_alpha in (0.5, 0.0):
        got = _one(r, cam, min_alpha=min_alpha)["labels"][0]
        want = _parent_labels(r, V, K, W, H, min_alpha=min_alpha)
        assert torch.equal(got, want["labels"]), (min_alpha, int((got != want["labels"]).sum()))
        # 255 is "group 255" and "none" alike, exactly as group_labels gives it
        assert torch.equal(got, group_labels(want["weights"], want["alpha"], min_alpha))
    assert len(torch.unique(got)) > 100


# ---- 3. batches and pose sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [1, 2, 3])
def test_batch_and_pose_sets(rasterizer, n_views):
    r = rasterizer
    sc, cam = sc_kit.twin("n2k_groups")
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    G = sc["G"]
    base = np.asarray(sc["Rt"], np.float32).reshape(G, 12)
    sets = np.stack([base, base.copy(), base.copy()])
    sets[1, :, 3] += 0.05
    sets[1, 1, 11] += 0.08
    sets[2, :, 7] -= 0.04
    sets[2, G - 1, 3] += 0.1
    Vs, Ks = np.stack([V, V, V]).copy(), np.stack([K, K, K]).copy()
    Vs[1, :3, 3] += np.array([0.12, -0.07, 0.2], np.float32)
    Ks[1, 0, 0] *= 1.1
    Vs[2, :3, 3] += np.array([-0.1, 0.05, 0.1], np.float32)
    Ks[2, 1, 2] += 3.0
    Vs, Ks, pose_set = Vs[:n_views], Ks[:n_views], [2, 0, 1][:n_views]
    before = r.get_group_poses()
    got = r.render_batch_labels(Vs, Ks, W, H, mc.BG, want=("labels", "rgb8", "depth"), pose_sets=sets, pose_set=pose_set)
    assert np.array_equal(r.get_group_poses(), before)                       # the context's poses are not touched
    assert got["labels"].shape == (n_views, H, W) and got["rgb8"].shape == (n_views, H, W, 3) and got["depth"].shape == (n_views, H, W, 1)
    frames = r.render_batch(Vs, Ks, W, H, mc.BG, want=("rgb8", "depth"), pose_sets=sets, pose_set=pose_set)
    assert torch.equal(got["rgb8"], frames["rgb8"]) and torch.equal(got["depth"].view(torch.int32), frames["depth"].view(torch.int32))
    labs = []
    for v in range(n_views):
        want = _parent_labels(r, Vs[v], Ks[v], W, H, Rt=sets[pose_set[v]])["labels"]
        assert torch.equal(got["labels"][v], want), (v, int((got["labels"][v] != want).sum()))
        labs.append(want)
    r.set_group_poses(before)
    if n_views == 3:
        assert not torch.equal(labs[0], labs[1]) and not torch.equal(labs[1], labs[2])
    # the same poses as the context's current ones, without pose sets
    r.set_group_poses(sets[2])
    plain = r.render_batch_labels(Vs[:1], Ks[:1], W, H)["labels"]
    assert torch.equal(plain[0], got["labels"][0])


# ---- 4. meshes ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh_case(name):
    """(case, expectation of view 0, the oracle's labels): computed once on the CPU, shared, never modified."""
    case = mf.case_labels() if name == "labels" else mf.drawn_case(int(name))
    e = mc.expected(case, 0)
    print(f"{name}: {case.get('describe', 'case_labels')} | excluded {100 * e['excluded']:.2f} %")
    assert e["excluded"] <= mc.MAX_EXCLUDED, (name, e["excluded"])     # settled on the CPU, before anything runs on the GPU
    return case, e, mf.expected_labels(case, e)


@pytest.mark.parametrize("name", ["labels"] + [str(s) for s in DRAWN_SEEDS])
def test_meshes(rasterizer, name):
    r = rasterizer
    case, e, want = _mesh_case(name)
    V, K, W, H = case["cams"][0]
    mc.upload_case(r, case)
    Rt = mc.view_poses(case, 0)
    if Rt is not None:
        r.set_group_poses(Rt)
    got = _one(r, case["cams"][0])["labels"][0]
    parent = _parent_labels(r, V, K, W, H)
    assert torch.equal(got, parent["labels"]), int((got != parent["labels"]).sum())
    st = e["stable"]
    lab = got.cpu().numpy()
    assert np.array_equal(lab[st], want["labels"][st]), int((lab[st] != want["labels"][st]).sum())
    mesh_rows = set(np.unique(np.asarray(case["mesh"]["groups"])).tolist())
    assert mesh_rows & set(np.unique(lab).tolist())                     # a mesh's row shows
    # without SAS_MESH_SURFACE alpha is the splats' alone: a covered pixel of thin splats reads 255
    off = _one(r, case["cams"][0], mesh_surface=False)["labels"][0]
    o = r.render_features(V, K, W, H, want=("features", "alpha"), mesh_surface=False)
    assert torch.equal(off, group_labels(o["features"], o["alpha"], 0.5))
    assert not torch.equal(off, got)


# ---- 5. min_alpha -------------------------------------------------------------------------------------------------------------------------
def test_min_alpha(rasterizer):
    r = rasterizer
    case, e, _ = _mesh_case("labels")
    cam = case["cams"][0]
    V, K, W, H = cam
    mc.upload_case(r, case)
    ref = _parent_labels(r, V, K, W, H)
    w, a = ref["weights"], ref["alpha"]
    for min_alpha in (0.0, 0.5, 1.0):
        got = _one(r, cam, min_alpha=min_alpha)["labels"][0]
        assert torch.equal(got, group_labels(w, a, min_alpha)), min_alpha
        if min_alpha == 0.0:
            assert not (got == 255).any()                                 # G < 256: no 255 from the argmax either
        if min_alpha == 1.0:
            assert torch.equal(got != 255, a[..., 0] == 1.0) and (got != 255).any()      # (the plane covers this frame: alpha is 1)
    assert torch.equal(_one(r, cam)["labels"][0], ref["labels"])        # the default is 0.5
    # the same on a scene without meshes, where alpha never reaches 1
    sc = sc_kit.synthetic(2000, 47, 0.02, n_groups=7)
    cam = sc_kit.ring(96, 64, f=40.0)
    sc_kit.upload(r, sc)
    ref = _parent_labels(r, *cam)
    for min_alpha in (0.0, 1.0):
        got = _one(r, cam, min_alpha=min_alpha)["labels"][0]
        assert torch.equal(got, group_labels(ref["weights"], ref["alpha"], min_alpha))
        assert torch.equal(got != 255, ref["alpha"][..., 0] >= min_alpha)    # G = 7: 255 comes from the alpha rule alone


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    r = Rasterizer(0)
    L = _capi.lib()
    INVALID, NO_SCENE = -1, -3
    cam = sc_kit.ring(96, 64, f=40.0)
    V, K, W, H = cam
    Vc, Kc = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(K, np.float32)
    labels = torch.zeros((1, H, W), dtype=torch.uint8, device=r.device)

    def call(flags=0, out=labels):
        return L.sas_render_batch_labels(r._ctx, 1, Vc.ctypes.data, Kc.ctypes.data, W, H, None, 0.5, flags, None, None, None, None,
                                         out.data_ptr() if out is not None else None, None)

    def refused(status, *words, **kw):
        assert call(**kw) == status
        msg = L.sas_last_error(r._ctx).decode()
        assert msg and all(w in msg for w in words), msg

    try:
        refused(NO_SCENE)                                                  # nothing uploaded
        with pytest.raises((SasError, ValueError)):
            r.render_batch_labels(V[None], K[None], W, H)
        plain = sc_kit.synthetic(500, 3, 0.03)
        sc_kit.upload(r, plain)
        refused(INVALID, "feature store")                                  # a scene without groups has no one-hot store
        with pytest.raises((SasError, ValueError)):
            r.render_batch_labels(V[None], K[None], W, H)
        sc = sc_kit.synthetic(2000, 47, 0.02, n_groups=7)
        sc_kit.upload(r, sc)
        refused(INVALID, "feature store")                                  # groups, but no store selected: the library selects none
        r.upload_features(np.random.default_rng(0).uniform(size=(2000, 7)).astype(np.float32))
        refused(INVALID, "one-hot")                                        # the caller's own features
        r.upload_features(None)
        assert call() == 0                                                 # ... and the valid call right behind it
        want = _parent_labels(r, V, K, W, H)["labels"]
        assert torch.equal(labels[0], want)
        refused(INVALID, "SAS_ASYNC", flags=_capi.SAS_ASYNC)
        refused(INVALID, "flags", flags=_capi.SAS_FULL_SORT)
        refused(INVALID, "labels", out=None)
        labels.zero_()
        assert call() == 0 and torch.equal(labels[0], want)
        v, t = mc.full_quad(cam, 3.2)
        r.upload_meshes(v, t, np.array([0.5, 0.5, 0.5], np.float32), groups=[1, 1])
        refused(INVALID, "meshes", "one-hot")                              # meshes without rows
        r.upload_mesh_features(np.zeros((2, 7), np.float32))
        refused(INVALID, "meshes", "one-hot")                              # ... with the caller's rows
        r.upload_mesh_features(None)
        assert call(flags=_capi.SAS_MESH_SURFACE) == 0
        assert torch.equal(labels[0], _parent_labels(r, V, K, W, H)["labels"])
        # the Python layer selects the stores itself, as render_group_masks does
        r.upload_features(np.zeros((2000, 7), np.float32))
        assert torch.equal(r.render_batch_labels(V[None], K[None], W, H)["labels"][0], labels[0])
    finally:
        r.close()


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_same_bytes(rasterizer):
    r = rasterizer
    sc, cam = sc_kit.twin("n2k_groups")
    V, K, W, H = cam
    sc_kit.upload(r, sc)
    Vs, Ks = np.stack([V, V]), np.stack([K, K])
    a = r.render_batch_labels(Vs, Ks, W, H, want=("labels", "rgb8"))
    b = r.render_batch_labels(Vs, Ks, W, H, want=("labels", "rgb8"))
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["rgb8"], b["rgb8"]) and torch.equal(a["labels"][0], a["labels"][1])
    assert a["labels"].data_ptr() != b["labels"].data_ptr()


# ---- last: the bounds-checked build -------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
