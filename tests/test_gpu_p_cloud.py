"""GPU: point clouds (sas_sample_points / Rasterizer.sample_point_cloud; DESIGN.md 3, "Point clouds") against tests/tools/cloud_ref.py,
which tests/test_cloud_cpu.py holds to its float64 form on cases where float32 arithmetic is exact.

Every check is BIT-EQUAL to ``cloud32``, the contract restated in NumPy float32: ``index``, ``points``, ``colors``, ``labels`` and
``count``; there is no tolerance anywhere in this file.  Shapes are the smallest that reach each edge: wave and workgroup sizes of the
sampling kernel (64, 1024), the capacity of its register-resident form (CLOUD_RESIDENT) with the streaming form beyond it, strides
that do not divide the image, crop and voxel edges one float apart.  Every check prints what it measured.  Every test fails without
the feature: the entry point, the method and the observation mode do not exist.  The file runs unchanged under the bounds-checked
build, and its last test reads that build's counter.
"""
import ctypes
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import CLOUD_RESIDENT, SasError, cloud_keep_table, cloud_transforms

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import cloud_cases as cc  # noqa: E402
import cloud_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("index", "points", "colors", "labels", "count")


def _gpu(r, c, K, **kw):
    """sample_point_cloud on a case of cloud_cases, as host arrays."""
    kw = dict(kw)
    for name in ("rgb8", "labels"):
        if kw.get(name) is True:
            kw[name] = c[name]
    res = r.sample_point_cloud(c["depth"], c["viewmats"], c["Ks"], c["W"], c["H"], K, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _ref(c, K, **kw):
    kw = dict(kw)
    for name in ("rgb8", "labels"):
        if kw.get(name) is True:
            kw[name] = c[name]
    T = cloud_transforms(c["viewmats"], kw.pop("frame", None))
    keep = cloud_keep_table(kw.pop("keep_labels", None))
    return cr.cloud32(c["depth"], c["Ks"], T, K, keep=keep, voxel=kw.pop("voxel_size", 0.0), **kw)


def _equal(what, got, want):
    n = 0
    for name in NAMES:
        if name in want:
            assert name in got, (what, name)
            g, w = got[name], want[name]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
            bad = int((g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1)).sum())
            assert bad == 0, (what, name, f"{bad} bytes differ", g.reshape(-1)[:8], w.reshape(-1)[:8])
            n += g.nbytes
    return n


def _check(r, what, c, K, **kw):
    got, want = _gpu(r, c, K, **kw), _ref(c, K, **kw)
    n = _equal(what, got, want)
    print(f"  {what}: K={K}, M={want['count'].tolist()}, {n} bytes equal")
    return got, want


# ---- 1: wave and workgroup edges of the sampling kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_survivor_counts(rasterizer, M):
    c = cc.exact_count(M, seed=100 + M)
    for K in sorted({k for k in (1, 64, 65, M - 1, M, M + 1) if k > 0}):
        got, want = _check(rasterizer, f"M={M}", c, K, rgb8=True, labels=True)
        assert want["count"][0] == M and (got["index"][0, :min(K, M)] >= 0).all() and (got["index"][0, M:] == -1).all()


# ---- 2: the register-resident form, the streaming form and the hand-over ---------------------------------------------------------------
@pytest.mark.parametrize("M", [CLOUD_RESIDENT - 1, CLOUD_RESIDENT, CLOUD_RESIDENT + 1])
def test_resident_capacity(rasterizer, M):
    c = cc.exact_count(M, seed=7, C=2, H=86, W=97)
    got, want = _check(rasterizer, f"M={M}", c, 70, rgb8=True, labels=True)
    assert want["count"][0] == M and cr.fps_is_greedy(want["w"][0], want["picks"][0][:12])


# ---- 3: ties and duplicates ------------------------------------------------------------------------------------------------------------
def test_ties_and_duplicates(rasterizer):
    r = rasterizer
    eye = np.eye(4, dtype=np.float32)
    # points symmetric about pick 0: view 0 holds the centre alone, view 1 a row through it -- the lower pixel of each pair wins
    W, H = 9, 1
    depth = np.zeros((2, H, W), np.float32)
    depth[0, 0, 4] = 2.0
    depth[1, 0] = 2.0
    c = dict(depth=depth, viewmats=np.stack([eye, eye]), Ks=np.stack([cc.intrinsics(W, H, 4.0, cx=4.0, cy=0.0)] * 2), W=W, H=H)
    got, want = _check(r, "symmetric", c, 10)
    # x = (u - 4) / 2: the centre, then the two ends (4 away each: the lower pixel first), then u = 2 before u = 6 (1 away each)
    assert got["index"][0, :5].tolist() == [4, 9, 17, 11, 15] and cr.fps_is_greedy(want["w"][0], want["picks"][0])
    # coincident survivors: five views of one pixel at one place -- every distance 0, the ranks in order, K distinct ranks
    depth = np.zeros((5, 4, 4), np.float32)
    depth[:, 2, 1] = 1.5
    c = dict(depth=depth, viewmats=np.stack([eye] * 5), Ks=np.stack([cc.intrinsics(4, 4, 3.0)] * 5), W=4, H=4)
    for K in (1, 3, 5, 6):
        got, want = _check(r, "coincident", c, K)
        assert got["index"][0, :min(K, 5)].tolist() == [9 + 16 * v for v in range(min(K, 5))]
    # the dyadic cases: whole classes of equal distances, arithmetic exact -- alone, and with every view doubled: each point has a twin
    for seed in (1, 2, 3):
        d = cc.dyadic(seed)
        for v in range(d["C"]):
            F = np.eye(4)
            F[:3] = d["transform"][v].reshape(3, 4)          # (the map as the frame of identity views)
            for copies in (1, 2):
                cv = dict(depth=np.stack([d["depth"][v]] * copies), viewmats=np.stack([eye] * copies), Ks=np.stack([d["Ks"][v]] * copies),
                          W=d["W"], H=d["H"])
                got, want = _check(r, f"dyadic seed {seed} view {v} x{copies}", cv, 150, frame=F)
                k = min(150, int(want["count"][0]))
                assert len(set(got["index"][0, :k].tolist())) == k and cr.fps_is_greedy(want["w"][0], want["picks"][0])
                w64 = cr.cloud64(cv["depth"], cv["Ks"], cloud_transforms(cv["viewmats"], F), 150)
                assert np.array_equal(got["index"], w64["index"]) and np.array_equal(got["points"].astype(np.float64), w64["points"])


# ---- 4: strides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_strides(rasterizer, stride):
    c = cc.drawn_views(2, 11, 13, seed=40)
    got, want = _check(rasterizer, f"stride {stride}", c, 64, stride=stride, rgb8=True, labels=True)
    p = want["survivors"][0]
    assert ((p % 13) % stride == 0).all() and (((p // 13) % 11) % stride == 0).all() and 0 < len(p)


# ---- 5 and 6: crop and voxel edges -------------------------------------------------------------------------------------------------------
def _axis_camera(depth, f):
    """One camera looking down +z, principal point at pixel (0, 0): pixel (u, v) at depth d is (u d / f, v d / f, d)."""
    C, H, W = depth.shape
    return dict(depth=depth, viewmats=np.stack([np.eye(4, dtype=np.float32)] * C), Ks=np.stack([cc.intrinsics(W, H, f, cx=0.0, cy=0.0)] * C), W=W, H=H)


def test_crop_edges(rasterizer):
    lo, hi = np.float32(1.0), np.float32(2.0)
    depth = np.zeros((1, 2, 4), np.float32)
    depth[0, 0] = [np.nextafter(lo, np.float32(0)), lo, hi, np.nextafter(hi, np.float32(3))]
    depth[0, 1] = [1.5, 1.5, 1.5, 1.5]
    c = _axis_camera(depth, 1.0)
    got, want = _check(rasterizer, "z edges", c, 8, bounds=([-10, -10, lo], [10, 10, hi]))
    assert sorted(got["index"][0, :got["count"][0]].tolist()) == [1, 2, 4, 5, 6, 7]
    # x = u d: 0, 1.5, 3, 4.5 on the second row -- the edges exactly on two of them, then one float inside each
    got, want = _check(rasterizer, "x edges", c, 8, bounds=([1.5, 1.0, 0], [3.0, 2.0, 5]))
    assert sorted(got["index"][0, :got["count"][0]].tolist()) == [5, 6]
    up, down = float(np.nextafter(np.float32(1.5), np.float32(2))), float(np.nextafter(np.float32(3), np.float32(2)))
    got, want = _check(rasterizer, "x edges, one float inside", c, 8, bounds=([up, 1.0, 0], [down, 2.0, 5]))
    assert got["count"][0] == 0 and (got["index"] == -1).all()


def test_voxel_edges(rasterizer):
    r = rasterizer
    depth = np.zeros((1, 2, 4), np.float32)
    depth[0, 0] = [1.0, 1.25, 1.999, 2.0]        # cells 0, 1 (on the face: the upper cell), 3, 3 (w == hi: clamped into the last)
    depth[0, 1] = [1.2, 0, 0, 0]                   # cell 0 again: the lower p stays
    c = _axis_camera(depth, 2.0 ** 20)
    got, want = _check(r, "z cells", c, 8, bounds=([0, 0, 1], [0.25, 0.25, 2]), voxel_size=0.25)
    assert got["count"][0] == 3 and sorted(got["index"][0, :3].tolist()) == [0, 1, 2]
    # two views into the same cells: the first view's pixels survive; as clouds of their own, both do
    two = _axis_camera(np.concatenate([depth, depth]), 1.0)
    got, want = _check(r, "two views, one cloud", two, 8, bounds=([0, 0, 1], [8, 8, 2]), voxel_size=0.25)
    assert sorted(got["index"][0, :got["count"][0]].tolist()) == [0, 1, 2, 3, 4]
    got, want = _check(r, "two views, two clouds", two, 8, bounds=([0, 0, 1], [8, 8, 2]), voxel_size=0.25, clouds=[1, 0], n_clouds=2)
    assert sorted(got["index"][0, :5].tolist()) == [8, 9, 10, 11, 12] and sorted(got["index"][1, :5].tolist()) == [0, 1, 2, 3, 4]
    # drawn views on a grid fine enough that cells are shared and coarse enough that many are
    d = cc.drawn_views(3, 20, 24, seed=61)
    F = cc.similarity(1.2, (1, 1, 0), 25.0, (0.1, 0.0, -0.2))
    got, want = _check(r, "drawn, voxel 0.15", d, 200, frame=F, bounds=([-1.5, -1.5, -0.5], [1.5, 1.5, 2.5]), voxel_size=0.15, rgb8=True, labels=True)
    plain = _ref(d, 200, frame=F, bounds=([-1.5, -1.5, -0.5], [1.5, 1.5, 2.5]))
    print(f"  voxel 0.15: {plain['count'][0]} candidates, {want['count'][0]} cells taken")
    assert 0 < want["count"][0] < plain["count"][0]
    # a grid of exactly 2^24 cells is accepted, one more layer is refused
    got, want = _check(r, "2^24 cells", d, 16, bounds=([-128, -128, -128], [128, 128, 128]), voxel_size=1.0)
    with pytest.raises(SasError, match="2\\^24"):
        _gpu(r, d, 16, bounds=([-128, -128, -128], [129, 128, 128]), voxel_size=1.0)


# ---- 7: defined inputs ---------------------------------------------------------------------------------------------------------------
def test_defined_inputs(rasterizer):
    r = rasterizer
    c = cc.drawn_views(2, 12, 15, seed=70, holes=0.1)
    c["depth"], where = cc.with_undefined(c["depth"], 71)
    got, want = _check(r, "NaN / Inf / 0 / negative depths", c, 400, rgb8=True, labels=True)
    M = int(got["count"][0])
    assert not np.isin(where, got["index"][0, :M]).any() and np.isfinite(got["points"]).all() and M < 360
    # a transform that overflows some points to Inf: they drop out, the others stay
    F = np.diag([3e38, 1.0, 1.0, 1.0])
    got, want = _check(r, "overflowing frame", c, 400, frame=F)
    print(f"  overflowing frame: {got['count'][0]} of {M} candidates stay finite")
    assert 0 < got["count"][0] < M and np.isfinite(got["points"]).all()
    # keep drops labels; label 255 is a label like any other
    for keep in ([0], [1, 3], [255], [0, 1, 2, 3, 255], []):
        got, want = _check(r, f"keep {keep}", c, 50, labels=True, keep_labels=keep, rgb8=True)
        k = min(50, int(got["count"][0]))
        assert set(np.unique(got["labels"][0, :k]).tolist()) <= set(keep) and (k > 0) == bool(keep)


# ---- 8: clouds ----------------------------------------------------------------------------------------------------------------------
def test_clouds(rasterizer):
    r = rasterizer
    c = cc.drawn_views(5, 14, 18, seed=80)
    kw = dict(bounds=([-2, -2, -2], [2, 2, 3]), voxel_size=0.1, rgb8=True, labels=True)
    clouds = [2, 0, 2, 0, 2]                                     # cloud 1 has no view
    got, want = _check(r, "E=3", c, 90, clouds=clouds, n_clouds=3, **kw)
    assert got["count"][1] == 0 and (got["index"][1] == -1).all() and (got["points"][1] == 0).all()
    assert (got["colors"][1] == 0).all() and (got["labels"][1] == 255).all() and got["count"][0] > 90 and got["count"][2] > 90
    px = 14 * 18
    for e in (0, 2):                                            # byte-equal to the cloud's views in a call of their own
        views = [v for v in range(5) if clouds[v] == e]
        sub = dict(c, depth=c["depth"][views], rgb8=c["rgb8"][views], labels=c["labels"][views], viewmats=c["viewmats"][views], Ks=c["Ks"][views])
        one = _gpu(r, sub, 90, **kw)
        k = min(90, int(one["count"][0]))
        idx = one["index"][0].copy()
        idx[:k] = np.asarray(views)[idx[:k] // px] * px + idx[:k] % px      # (a pixel's p names its view's place in the call)
        assert np.array_equal(idx, got["index"][e]) and one["count"][0] == got["count"][e]
        for name in ("points", "colors", "labels"):
            assert one[name][0].tobytes() == got[name][e].tobytes(), (e, name)
    # the views permuted within the call: the survivors (no grid: all candidates) are the same pixels
    perm = [3, 0, 4, 2, 1]
    crop = dict(bounds=([-2, -2, -2], [2, 2, 3]))
    a = _gpu(r, c, 5 * px, **crop)
    pc = dict(c, depth=c["depth"][perm], viewmats=c["viewmats"][perm], Ks=c["Ks"][perm])
    b, _ = _check(r, "permuted views", pc, 5 * px, **crop)
    M = int(a["count"][0])
    back = np.asarray(perm)[b["index"][0, :M] // px] * px + b["index"][0, :M] % px
    assert b["count"][0] == M and np.array_equal(np.sort(back), np.sort(a["index"][0, :M]))


# ---- 9: prefix, repeat, device and host inputs ------------------------------------------------------------------------------------------
def test_prefix_and_determinism(rasterizer):
    r = rasterizer
    c = cc.drawn_views(2, 30, 40, seed=90)
    kw = dict(bounds=([-2, -2, -2], [2, 2, 3]), voxel_size=0.05, rgb8=True, labels=True, frame=cc.similarity(0.9, (0, 1, 0), 10.0, (0, 0.1, 0)))
    full, want = _check(r, "K=600", c, 600, **kw)
    assert want["count"][0] > 600
    for K in (1, 2, 64, 599):
        part = _gpu(r, c, K, **kw)
        for name in ("index", "points", "colors", "labels"):
            assert part[name][0].tobytes() == full[name][0, :K].tobytes(), (K, name)
    again = _gpu(r, c, 600, **kw)
    assert all(again[k].tobytes() == full[k].tobytes() for k in full)
    dev = dict(c, depth=torch.from_numpy(c["depth"]).to(r.device), rgb8=torch.from_numpy(c["rgb8"]).to(r.device),
               labels=torch.from_numpy(c["labels"]).to(r.device))
    on_device = _gpu(r, dev, 600, **dict(kw, rgb8=dev["rgb8"], labels=dev["labels"]))
    assert all(on_device[k].tobytes() == full[k].tobytes() for k in full)
    print(f"  prefix: 4 prefixes, a second call and device inputs equal {sum(v.nbytes for v in full.values())} bytes")


# ---- 10: the camera points are those of render_rgbd ---------------------------------------------------------------------------------------
def test_points_are_render_rgbd_points(rasterizer):
    import scene_cases as sc_kit
    r = rasterizer
    sc_kit.upload(r, sc_kit.synthetic(3000, 5, 0.03))
    W, H = 50, 38
    K = cc.intrinsics(W, H, 45.0, cx=24.3, cy=18.9)
    eye = np.eye(4, dtype=np.float32)
    o = r.render_rgbd(eye, K, W, H, max_depth=None, depth_fill_max=False)
    res = r.sample_point_cloud(o["depth"], eye[None], K[None], W, H, 300)
    M, idx = int(res["count"][0]), res["index"][0].cpu().numpy()
    pts = o["points"].reshape(-1, 3).cpu().numpy()
    k = min(300, M)
    print(f"  render_rgbd: {M} pixels with depth, {k} picked")
    assert M > 300 and res["points"][0, :k].cpu().numpy().tobytes() == pts[idx[:k]].tobytes()
    _equal("rgbd depth", {k_: v.cpu().numpy() for k_, v in res.items()}, cr.cloud32(o["depth"].cpu().numpy().reshape(1, H, W), K[None], cloud_transforms(eye[None]), 300))


# ---- 11: end to end -------------------------------------------------------------------------------------------------------------------
ICP = cc.similarity(0.8, (0, 0, 1), 30.0, (0.1, -0.2, 0.05))
CAMS = [((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 3.0)), ((0.0, 1.0, 0.0, 0.0), (0.3, 0.2, 2.6))]
INFO = {0: {"link_name": "world", "local_frame": CAMS[0], "type": "viewport", "render_size": [48, 64]},
        1: {"link_name": "world", "local_frame": CAMS[1], "type": "static", "render_size": [48, 64]}}


class _Env:
    visualize_robot_flag = False

    def reset(self, seed=None, reset_to_state=None):
        pass

    def step(self, action):
        return {}, 0.0, False, False, {}

    def render(self):
        pass

    def _get_obs(self):
        return {"robot_pos": np.zeros(2)}

    def _generate_draw_msg(self):
        return types.SimpleNamespace(num_links=2, robot_num=[3, 3], link_name=["plant::link0", "plant::link1"],
                                     quaternion=[[1.0, 0, 0, 0], [0.995, 0, 0, 0.0998]], position=[[0.0, 0, 0], [0.02, 0.0, 0.0]])

    def close(self):
        pass


@pytest.fixture(scope="module")
def handler():
    from sim_a_splat_amd.covariance import GSplatLoader
    from sim_a_splat_amd.handler import SplatHandler
    from sim_a_splat_amd.synthetic import make_scene
    sc = make_scene(4000, seed=12, log_scale_mean=float(np.log(0.03)), n_groups=3)
    L = GSplatLoader.from_arrays(sc.means, sc.quats, np.log(sc.scales), sc.sh[:, 0], np.log(sc.opacities / (1 - sc.opacities)))
    masks = {f"link{i}": sc.group_id == i + 1 for i in range(2)}
    h = SplatHandler.from_arrays(L.means.numpy(), L.covs.numpy(), np.clip(L.colors.numpy(), 0, 1), L.opacities.numpy(), masks, ICP,
                                 [np.eye(4)] * 2, device=0)
    v = np.array([[-0.4, -0.4, 0.9], [0.4, -0.4, 0.9], [0.4, 0.4, 0.9], [-0.4, 0.4, 0.9]])
    h.scene.add_mesh_simple("plate", v, np.array([[0, 1, 2], [0, 2, 3], [0, 2, 1], [0, 3, 2]]), (0.2, 0.7, 0.3))
    yield h
    h.scene.close()


def test_scene_point_clouds_end_to_end(handler):
    scene = handler.scene
    H, W, K = 48, 64, 256
    names = scene.row_names()
    kw = dict(bounds=([-1.2, -1.2, -1.2], [1.2, 1.2, 1.3]), voxel_size=0.04, stride=1, frame=cc.similarity(1.1, (0, 1, 0), 15.0, (0.05, 0, 0)))
    o = scene.get_point_clouds(H, W, CAMS, K, keep=[names[0], len(names) - 1, names[2]], **kw)
    fr = {k: v.cpu().numpy() for k, v in o["frames"].items()}
    q, p = np.array([c[0] for c in CAMS], float), np.array([c[1] for c in CAMS], float)
    V, Ks = scene._views_and_Ks(H, W, q, p, scene.camera.fov)
    rows = [0, len(names) - 1, 2]
    want = cr.cloud32(fr["depth"], Ks, cloud_transforms(V, kw["frame"]), K, rgb8=fr["rgb8"], labels=fr["labels"], keep=cloud_keep_table(rows),
                      bounds=kw["bounds"], voxel=kw["voxel_size"])
    got = {k: v.cpu().numpy() for k, v in o.items() if k != "frames"}
    n = _equal("scene", got, want)
    seen = sorted(set(got["labels"][0, :min(K, got["count"][0])].tolist()))
    print(f"  scene ({names}): M={got['count'][0]}, rows seen {seen}, {n} bytes equal")
    assert got["count"][0] > K and set(seen) <= set(rows) and len(seen) >= 2
    # two envs in one call (pose sets, one cloud per env) equal each env alone
    base = scene.group_pose_rows()
    sets = np.stack([base, base.copy()])
    sets[1, 0, 3] += 0.15
    sets[1, 1, 7] -= 0.1
    both = scene.get_point_clouds(H, W, CAMS + CAMS, K, pose_sets=sets, pose_set=[0, 0, 1, 1], clouds=[0, 0, 1, 1], n_clouds=2, **kw)
    for e in range(2):
        one = scene.get_point_clouds(H, W, CAMS, K, pose_sets=sets[e:e + 1], pose_set=[0, 0], **kw)
        for name in ("points", "colors", "labels"):
            assert torch.equal(one[name][0], both[name][e]), (e, name)
        k = min(K, int(one["count"][0]))
        assert one["count"][0] == both["count"][e] and torch.equal(one["index"][0, :k] + 2 * e * H * W, both["index"][e, :k])
    assert not torch.equal(both["points"][0], both["points"][1])
    print(f"  two envs in one call: M={both['count'].tolist()}, each equal to its env alone")


def test_handler_and_env_observation(handler):
    from sim_a_splat_amd.env_wrapper import SplatEnvWrapper
    scene = handler.scene
    K = 128
    cfg = dict(bounds=([-1.0, -1.0, -1.0], [1.0, 1.0, 1.2]), voxel_size=0.05, stride=2)
    sizes = [[48, 64], [48, 64]]
    o = handler.render_point_cloud(scene, CAMS, sizes, K, frame="robot", **cfg)
    assert o["points"].shape == (1, K, 3) and o["colors"].shape == (1, K, 3) and o["labels"].shape == (1, K) and o["index"].dtype == torch.int32
    same = scene.get_point_clouds(48, 64, CAMS, K, frame=handler.robot_frame(), **cfg)
    assert all(torch.equal(o[k], same[k]) for k in ("points", "index", "colors", "labels", "count"))
    # the robot frame is the scene's through the inverse ICP similarity: the same pixels' points, mapped
    raw = scene.get_point_clouds(48, 64, CAMS, K, stride=2)
    idx = o["index"][0, :int(min(K, o["count"][0]))].cpu().numpy()
    assert o["count"][0] > 0
    with pytest.raises(ValueError):
        handler.render_point_cloud(scene, CAMS, [[48, 64], [24, 32]], K)
    env = SplatEnvWrapper(_Env(), splat_handler=handler, obs_modes=("rgb", "pointcloud"), point_cloud=dict(n_points=K, frame="robot", **cfg))
    env._configure_cameras(INFO)
    env.reset()
    obs, *_ = env.step(None)
    pc = obs["point_cloud"]
    assert list(obs) == ["robot_pos", "camera_0", "camera_1", "point_cloud"] and pc.shape == (K, 6) and pc.dtype == np.float32
    now = handler.render_point_cloud(scene, CAMS, sizes, K, frame="robot", **cfg)     # (the step has posed the links: the cloud of now)
    k = int(min(K, now["count"][0]))
    assert np.array_equal(pc[:, :3], now["points"][0].cpu().numpy()) and np.array_equal(pc[:, 3:], now["colors"][0].cpu().numpy().astype(np.float32) / np.float32(255))
    assert (pc[k:] == 0).all() and pc[:k, 3:].min() >= 0 and pc[:k, 3:].max() <= 1
    lo, hi = np.asarray(cfg["bounds"], np.float32)
    assert (pc[:k, :3] >= lo).all() and (pc[:k, :3] <= hi).all()
    print(f"  env observation: point_cloud {pc.shape}, {k} points, xyz in [{pc[:k, :3].min(0).round(3).tolist()}, {pc[:k, :3].max(0).round(3).tolist()}]; "
          f"raw scene-frame M {int(raw['count'][0])}, {len(idx)} picked in the robot frame")
    with pytest.raises(ValueError):
        SplatEnvWrapper(_Env(), splat_handler=handler, obs_modes=("rgb", "pointcloud"))


# ---- 12: errors ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(rasterizer):
    r = rasterizer
    L = _capi.lib()
    C, H, W, K, E = 2, 6, 8, 5, 2
    c = cc.drawn_views(C, H, W, seed=120, holes=0.0)
    depth = torch.from_numpy(c["depth"]).to(r.device)
    rgb8 = torch.from_numpy(c["rgb8"]).to(r.device)
    labels = torch.from_numpy(c["labels"]).to(r.device)
    index = torch.full((E, K), 7, dtype=torch.int32, device=r.device)
    points = torch.zeros((E, K, 3), dtype=torch.float32, device=r.device)
    colors = torch.zeros((E, K, 3), dtype=torch.uint8, device=r.device)
    labels_out = torch.zeros((E, K), dtype=torch.uint8, device=r.device)
    count = torch.zeros((E,), dtype=torch.int32, device=r.device)
    Ks = np.ascontiguousarray(c["Ks"].reshape(C, 9))
    T = cloud_transforms(c["viewmats"])
    cloud = np.array([1, 0], np.int32)
    bounds = np.array([-5, -5, -5, 5, 5, 5], np.float32)
    keep = np.ones(256, np.uint8)
    ptr = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)

    def call(n_views=C, w=W, h=H, d=depth, c8=rgb8, lab=labels, ks=Ks, tr=T, cl=cloud, e=E, kp=keep, b=bounds, voxel=0.5, stride=1, k=K,
             flags=0, pts=points, idx=index, col=colors, lo=labels_out, cnt=count):
        rc = L.sas_sample_points(r._ctx, n_views, w, h, ptr(d), ptr(c8), ptr(lab), ptr(ks), ptr(tr), ptr(cl), e, ptr(kp), ptr(b),
                                 ctypes.c_float(voxel), stride, k, flags, ptr(pts), ptr(idx), ptr(col), ptr(lo), ptr(cnt), None)
        return rc, L.sas_last_error(r._ctx).decode()

    assert call()[0] == 0 and count.cpu().tolist() == [int(x) for x in cr.cloud32(c["depth"], Ks, T, K, bounds=bounds, voxel=0.5, clouds=cloud, n_clouds=E)["count"]]

    def changed(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    cases = {"negative n_views": dict(n_views=-1), "zero width": dict(w=0), "negative height": dict(h=-3),
             "more than 2^31 - 256 pixels": dict(n_views=2, w=32768, h=32768), "negative n_points": dict(k=-1), "stride 0": dict(stride=0),
             "no cloud": dict(e=0), "cloud index out of range": dict(cl=np.array([0, 2], np.int32)), "negative cloud index": dict(cl=np.array([-1, 0], np.int32)),
             "NaN transform": dict(tr=changed(T, 5, np.nan)), "Inf transform": dict(tr=changed(T, 15, np.inf)), "NaN K": dict(ks=changed(Ks, 2, np.nan)),
             "Inf K": dict(ks=changed(Ks, 14, -np.inf)), "fx 0": dict(ks=changed(Ks, 0, 0.0)), "fy negative": dict(ks=changed(Ks, 13, -1.0)),
             "lo above hi": dict(b=changed(bounds, 1, 6.0)), "NaN bound": dict(b=changed(bounds, 4, np.nan)), "NaN voxel": dict(voxel=float("nan")),
             "negative voxel": dict(voxel=-0.1), "infinite voxel": dict(voxel=float("inf")), "voxel without bounds": dict(b=None),
             "grid too large": dict(voxel=0.01), "grid overflowing int": dict(voxel=1e-30), "no depth": dict(d=None), "no index": dict(idx=None),
             "no Ks": dict(ks=None), "colors without rgb8": dict(c8=None), "labels_out without labels": dict(lab=None, kp=None),
             "unknown flag": dict(flags=2)}
    for what, kw in cases.items():
        rc, msg = call(**kw)
        print(f"  {what}: status {rc}, {msg!r}")
        assert rc == -1 and msg, what
    # allowed: no point, no view, every optional array left out
    assert call(k=0, idx=None, pts=None, col=None, lo=None)[0] == 0
    assert call(n_views=0, d=None, ks=None, tr=None, cl=None)[0] == 0 and count.cpu().tolist() == [0, 0] and (index.cpu().numpy() == -1).all()
    assert call(tr=None, cl=None, e=1, kp=None, b=None, voxel=0.0, pts=None, col=None, lo=None, cnt=None, c8=None, lab=None)[0] == 0
    # the Python method's own checks
    with pytest.raises(ValueError):
        r.sample_point_cloud(c["depth"][:1], c["viewmats"], c["Ks"], W, H, K)
    with pytest.raises(ValueError):
        r.sample_point_cloud(c["depth"], c["viewmats"], c["Ks"], W, H, K, keep_labels=[1])
    with pytest.raises(ValueError):
        r.sample_point_cloud(c["depth"], c["viewmats"], c["Ks"], W, H, K, clouds=[0])
    with pytest.raises(ValueError):
        r.sample_point_cloud(c["depth"], c["viewmats"], c["Ks"], W, H, K, bounds=[0, 1])
    with pytest.raises(SasError):
        r.sample_point_cloud(c["depth"], c["viewmats"], c["Ks"], W, H, K, voxel_size=0.1)
    with pytest.raises(SasError):
        r.sample_point_cloud(c["depth"], c["viewmats"], c["Ks"], W, H, K, stride=0)
    # the context still answers
    _check(r, "after the errors", c, K, rgb8=True, labels=True)


# ---- last: the bounds-checked build ------------------------------------------------------------------------------------------------------
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
