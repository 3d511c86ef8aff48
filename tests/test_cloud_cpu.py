"""CPU: point clouds above the C ABI ("Point clouds") -- the reference the GPU tests hold the kernels to
(tests/tools/cloud_ref.py) against its float64 form on the dyadic cases, where float32 arithmetic is exact; its sampling order against
a brute-force greedy check; the contract's rules (prefix, padding, voxel grid, crop edges) on it; the Python-side validation; and the
``"pointcloud"`` observation plumbing over a stand-in scene.  No GPU: the kernels' side is tests/test_gpu_p_cloud.py."""
import ctypes
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, build, rasterizer
from sim_a_splat_amd.handler import SplatHandler
from sim_a_splat_amd.env_wrapper import SplatEnvWrapper

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import cloud_cases as cc  # noqa: E402
import cloud_ref as cr  # noqa: E402


def test_entry_point_is_exported_and_declared():
    L = ctypes.CDLL(str(build.build()))
    assert "sas_sample_points" in _capi.EXPORTS and hasattr(L, "sas_sample_points")
    assert len(_capi.lib().sas_sample_points.argtypes) == 23
    assert rasterizer.CLOUD_RESIDENT == _capi.SAS_CLOUD_RESIDENT
    text = (Path(build.CSRC) / "sas_internal.h").read_text()
    assert f"#define SAS_CLOUD_RESIDENT {_capi.SAS_CLOUD_RESIDENT} " in text
    assert build.CSRC / "sas_cloud.hip" in build.SOURCES


# ---- the reference against its float64 form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", [False, True])
def test_dyadic_cases_are_exact(seed, grid):
    c = cc.dyadic(seed, C=2 + seed % 2)
    kw = dict(rgb8=c["rgb8"], labels=c["labels"], bounds=c["bounds"], voxel=c["voxel"] if grid else 0.0, stride=1 + (seed == 4))
    a = cr.cloud32(c["depth"], c["Ks"], c["transform"], 40, **kw)
    b = cr.cloud64(c["depth"], c["Ks"], c["transform"], 40, **kw)
    assert a["points"].dtype == np.float32 and b["points"].dtype == np.float64
    assert a["count"][0] > 40 and np.array_equal(a["count"], b["count"])
    assert np.array_equal(a["index"], b["index"])
    assert np.array_equal(a["points"].astype(np.float64), b["points"])
    assert np.array_equal(a["colors"], b["colors"]) and np.array_equal(a["labels"], b["labels"])
    assert np.array_equal(a["survivors"][0], b["survivors"][0])


@pytest.mark.parametrize("seed", [11, 12])
def test_sampling_is_greedy(seed):
    c = cc.drawn_views(2, 14, 17, seed)
    T = rasterizer.cloud_transforms(c["viewmats"], cc.similarity(1.3, (1, 2, 3), 20.0, (0.1, 0.2, -0.3)))
    r = cr.cloud32(c["depth"], c["Ks"], T, 60)
    assert r["count"][0] > 60 and cr.fps_is_greedy(r["w"][0], r["picks"][0])
    d = cc.dyadic(seed)                       # many equal distances: the lowest rank among them
    r = cr.cloud32(d["depth"], d["Ks"], d["transform"], 50)
    assert cr.fps_is_greedy(r["w"][0], r["picks"][0])
    assert not cr.fps_is_greedy(r["w"][0], r["picks"][0][::-1])
    # coincident survivors: every distance 0, the ranks in order
    w = np.zeros((5, 3), np.float32)
    assert cr.fps(w, 5).tolist() == [0, 1, 2, 3, 4] and cr.fps_is_greedy(w, [0, 1, 2, 3, 4]) and not cr.fps_is_greedy(w, [0, 2, 1])


def test_prefix_padding_and_counts():
    c = cc.drawn_views(2, 10, 11, 21)
    T = rasterizer.cloud_transforms(c["viewmats"])
    full = cr.cloud32(c["depth"], c["Ks"], T, 500, rgb8=c["rgb8"], labels=c["labels"])
    M = int(full["count"][0])
    assert 0 < M < 220 and M == int(((c["depth"] > 0)).sum())
    assert (full["index"][0, :M] >= 0).all() and len(set(full["index"][0, :M].tolist())) == M
    assert (full["index"][0, M:] == -1).all() and (full["points"][0, M:] == 0).all()
    assert (full["colors"][0, M:] == 0).all() and (full["labels"][0, M:] == 255).all()
    for k in (1, 7, M - 1, M):
        part = cr.cloud32(c["depth"], c["Ks"], T, k, rgb8=c["rgb8"], labels=c["labels"])
        for name in ("points", "index", "colors", "labels"):
            assert np.array_equal(part[name][0], full[name][0, :k]), (k, name)
    p = full["index"][0, :M]
    assert np.array_equal(full["colors"][0, :M], c["rgb8"].reshape(-1, 3)[p]) and np.array_equal(full["labels"][0, :M], c["labels"].reshape(-1)[p])
    zero = cr.cloud32(c["depth"], c["Ks"], T, 0)
    assert zero["index"].shape == (1, 0) and zero["count"][0] == M


def test_voxel_and_crop_rules():
    # one camera looking down +z with the principal point at the origin pixel: pixel (u, v) at depth d is (u d / f, v d / f, d).
    # f = 2^20 keeps x and y within 1e-5 of the axis (one cell); f = 1 spreads them
    K, Kbig = cc.intrinsics(4, 2, 1.0, cx=0.0, cy=0.0)[None], cc.intrinsics(4, 2, 2.0 ** 20, cx=0.0, cy=0.0)[None]
    depth = np.zeros((1, 2, 4), np.float32)
    lo, hi = np.float32(1.0), np.float32(2.0)
    depth[0, 0] = [np.nextafter(lo, np.float32(0)), lo, hi, np.nextafter(hi, np.float32(3))]
    bounds = [[-10, -10, lo], [10, 10, hi]]
    r = cr.cloud32(depth, K, None, 4, bounds=bounds)
    assert r["survivors"][0].tolist() == [1, 2]                                   # inclusive at both edges, nothing beyond
    # voxel 0.25 over z in [1, 2]: four cells; z = 1.25 lies on a face and belongs to the upper cell; z = 2 is clamped into the last
    depth[0, 0] = [1.0, 1.25, 1.999, 2.0]
    depth[0, 1] = [1.2, 0, 0, 0]                                                    # shares cell 0 with pixel 0: the lower p stays
    r = cr.cloud32(depth, Kbig, None, 8, bounds=[[0, 0, 1], [0.25, 0.25, 2]], voxel=0.25)
    assert r["count"][0] == 3 and r["survivors"][0].tolist() == [0, 1, 2]         # (2.0 shares the last cell with 1.999)
    # f = 1: (u d, v d) spreads the same depths over different cells
    r = cr.cloud32(depth, K, None, 8, bounds=[[0, 0, 1], [8, 8, 2]], voxel=0.25)
    assert r["survivors"][0].tolist() == [0, 1, 2, 3, 4]
    # two views into one cell: the first view's pixel survives
    two = np.stack([depth[0], depth[0]])
    r = cr.cloud32(two, np.concatenate([K, K]), None, 8, bounds=[[0, 0, 1], [8, 8, 2]], voxel=0.25)
    assert r["survivors"][0].tolist() == [0, 1, 2, 3, 4]
    r = cr.cloud32(two, np.concatenate([K, K]), None, 8, bounds=[[0, 0, 1], [8, 8, 2]], voxel=0.25, clouds=[1, 0], n_clouds=2)
    assert r["survivors"][0].tolist() == [8, 9, 10, 11, 12] and r["survivors"][1].tolist() == [0, 1, 2, 3, 4]


def test_undefined_depths_and_keep():
    c = cc.drawn_views(1, 9, 9, 31, holes=0.0)
    d, where = cc.with_undefined(c["depth"], 32)
    T = rasterizer.cloud_transforms(c["viewmats"])
    r = cr.cloud32(d, c["Ks"], T, 81)
    assert r["count"][0] == 81 - len(where) and not np.isin(where, r["survivors"][0]).any()
    assert np.isfinite(r["points"]).all()
    keep = rasterizer.cloud_keep_table([1, 255])
    r = cr.cloud32(c["depth"], c["Ks"], T, 81, labels=c["labels"], keep=keep)
    assert r["count"][0] == int(np.isin(c["labels"], [1, 255]).sum()) > 0
    assert set(np.unique(r["labels"][0, :r["count"][0]])) == {1, 255}


# ---- Python-side helpers and validation ----------------------------------------------------------------------------------------------
def test_transforms_keep_table_and_bounds():
    c = cc.drawn_views(3, 4, 5, 41)
    F = cc.similarity(0.7, (0, 1, 1), 33.0, (1, 2, 3))
    T = rasterizer.cloud_transforms(c["viewmats"], F)
    assert T.shape == (3, 12) and T.dtype == np.float32
    for v in range(3):
        want = (F @ np.linalg.inv(c["viewmats"][v].astype(np.float64)))[:3]
        assert np.abs(T[v].reshape(3, 4) - want).max() <= 1e-6
    assert np.array_equal(rasterizer.cloud_transforms(np.eye(4)[None])[0], np.eye(4, dtype=np.float32)[:3].reshape(12))
    with pytest.raises(ValueError):
        rasterizer.cloud_transforms(np.eye(4))
    with pytest.raises(ValueError):
        rasterizer.cloud_transforms(np.eye(4)[None], np.eye(3))
    assert rasterizer.cloud_keep_table(None) is None and rasterizer.cloud_keep_table([0, 3]).nonzero()[0].tolist() == [0, 3]
    with pytest.raises(ValueError):
        rasterizer.cloud_keep_table([256])
    assert rasterizer.cloud_bounds(([0, 1, 2], [3, 4, 5])).tolist() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        rasterizer.cloud_bounds([0, 1, 2])


# ---- observation plumbing over a stand-in scene ---------------------------------------------------------------------------------------
class _Scene:
    """Plays SplatScene: records the calls, returns a cloud whose values name the call."""

    def __init__(self):
        self.camera = types.SimpleNamespace(wxyz=np.array([1.0, 0, 0, 0]), position=np.zeros(3), fov=1.0)
        self.cloud_calls, self.obs_calls, self.rgb_calls, self.groups = [], [], [], []

    def add_gaussian_splats(self, name, centers, covariances, rgbs, opacities, wxyz=(1.0, 0, 0, 0), position=(0.0, 0, 0)):
        h = types.SimpleNamespace(name=name, n=len(centers), wxyz=np.asarray(wxyz, float), position=np.asarray(position, float))
        self.groups.append(h)
        return h

    def row_names(self):
        return [g.name for g in self.groups]

    def get_renders(self, height, width, cam_poses, fov=None):
        self.rgb_calls.append((height, width, len(cam_poses)))
        return np.stack([np.full((height, width, 3), 7, np.uint8) for _ in cam_poses])

    def get_observations(self, height, width, cam_poses, fov=None, pose_sets=None, pose_set=None, min_alpha=0.5, want=("labels",)):
        self.obs_calls.append((height, width, len(cam_poses), tuple(want)))
        C = len(cam_poses)
        table = {"labels": ((C, height, width), torch.uint8), "rgb8": ((C, height, width, 3), torch.uint8), "depth": ((C, height, width, 1), torch.float32)}
        return {n: torch.full(table[n][0], 3, dtype=table[n][1]) for n in dict.fromkeys(tuple(want) + ("labels",))}

    def get_point_clouds(self, height, width, cam_poses, n_points, **kw):
        self.cloud_calls.append((height, width, len(cam_poses), n_points, kw))
        K, M = n_points, min(n_points, 5)
        pts, col = torch.zeros((1, K, 3)), torch.zeros((1, K, 3), dtype=torch.uint8)
        pts[0, :M] = torch.arange(3 * M, dtype=torch.float32).reshape(M, 3)
        col[0, :M] = 255
        return {"points": pts, "colors": col, "index": torch.zeros((1, K), dtype=torch.int32), "count": torch.tensor([M], dtype=torch.int32)}

    def close(self):
        pass


class _Env:
    visualize_robot_flag = False
    package_path, package_name, urdf_name, weld_frame_transform = "/pkg", "robot/", "robot.urdf", None

    def reset(self, seed=None, reset_to_state=None):
        pass

    def step(self, action):
        return {"inner": 1}, 0.0, False, False, {}

    def render(self):
        pass

    def _get_obs(self):
        return {"robot_pos": np.zeros(2)}

    def _generate_draw_msg(self):
        return types.SimpleNamespace(num_links=2, robot_num=[3, 3], link_name=["plant::link0", "plant::eef"],
                                     quaternion=[[1.0, 0, 0, 0], [1.0, 0, 0, 0]], position=[[0.0, 0, 0], [0.1, 0.0, 0.0]])

    def close(self):
        pass


INFO = {0: {"link_name": "world", "local_frame": ((0.0, 1.0, 0, 0), (-0.15, -0.3, -0.05)), "type": "viewport", "render_size": [24, 32]},
        1: {"link_name": "eef", "local_frame": ((1.0, 0, 0, 0), (-0.1, 0, 0.033)), "type": "moving", "render_size": [24, 32]}}
ICP = cc.similarity(0.5, (0, 0, 1), 90.0, (1.0, 2.0, 3.0))


def _handler():
    n, rng, scene = 12, np.random.default_rng(0), _Scene()
    masks = {"link0": np.arange(n) < 3, "link1": (np.arange(n) >= 3) & (np.arange(n) < 5)}
    h = SplatHandler.from_arrays(rng.normal(size=(n, 3)), np.tile(np.eye(3), (n, 1, 1)), rng.uniform(size=(n, 3)), rng.uniform(size=n),
                                 masks, ICP, [np.eye(4), np.eye(4)], scene=scene)
    return h, scene


def test_robot_frame_inverts_the_icp_similarity():
    h, _ = _handler()
    F = h.robot_frame()
    assert np.abs(F @ ICP - np.eye(4)).max() <= 1e-12                 # x_scene = ICP x_robot (poses.decompose_icp: s, Ri, ti)
    x_robot = np.array([0.3, -0.2, 0.9, 1.0])
    assert np.abs(F @ (ICP @ x_robot) - x_robot).max() <= 1e-12


def test_render_point_cloud_plumbing():
    h, scene = _handler()
    cams = [((1.0, 0, 0, 0), (0.0, 0, 0)), ((1.0, 0, 0, 0), (0.1, 0, 0))]
    o = h.render_point_cloud(scene, cams, [[24, 32], [24, 32]], 9, frame="robot", bounds=([0, 0, 0], [1, 1, 1]), voxel_size=0.01, stride=2,
                             keep=["/scene_ohne_robot"])
    assert o["points"].shape == (1, 9, 3)
    H, W, C, K, kw = scene.cloud_calls[-1]
    assert (H, W, C, K) == (24, 32, 2, 9) and kw["stride"] == 2 and kw["voxel_size"] == 0.01 and kw["keep"] == ["/scene_ohne_robot"]
    assert np.array_equal(kw["frame"], h.robot_frame())
    h.render_point_cloud(scene, cams, [[24, 32], [24, 32]], 9)
    assert scene.cloud_calls[-1][4]["frame"] is None                    # the scene's own frame
    with pytest.raises(ValueError):
        h.render_point_cloud(scene, cams, [[24, 32], [8, 8]], 9)
    with pytest.raises(ValueError):
        h.render_point_cloud(scene, cams, [[24, 32], [24, 32]], 9, frame="world")
    with pytest.raises(ValueError):
        h.render_observations(scene, cams, [[24, 32], [24, 32]], ("rgb", "pointcloud"))
    assert "pointcloud" in SplatHandler.OBS_MODES


def test_env_wrapper_pointcloud_observation():
    h, scene = _handler()
    with pytest.raises(ValueError):
        SplatEnvWrapper(_Env(), splat_handler=h, obs_modes=("rgb", "pointcloud"))
    with pytest.raises(ValueError):
        SplatEnvWrapper(_Env(), splat_handler=h, obs_modes=("rgb", "pointcloud"), point_cloud=dict(bounds=None))
    with pytest.raises(ValueError):
        SplatEnvWrapper(_Env(), splat_handler=h, obs_modes=("rgb",), point_cloud=dict(n_points=8))
    env = SplatEnvWrapper(_Env(), splat_handler=h, obs_modes=("rgb", "depth", "pointcloud"),
                          point_cloud=dict(n_points=8, bounds=([-1, -1, 0], [1, 1, 1]), voxel_size=0.005, stride=2, keep=None, frame="robot"))
    env._configure_cameras(INFO)
    env.reset()
    obs, *_ = env.step(None)
    assert list(obs) == ["robot_pos", "camera_0", "camera_0_depth", "camera_1", "camera_1_depth", "point_cloud"]
    pc = obs["point_cloud"]
    assert pc.shape == (8, 6) and pc.dtype == np.float32
    assert np.array_equal(pc[:5, :3], np.arange(15, dtype=np.float32).reshape(5, 3)) and (pc[:5, 3:] == 1.0).all() and (pc[5:] == 0).all()
    assert len(scene.cloud_calls) == 1 and len(scene.obs_calls) == 1     # one label-frame call for the frames, one cloud call
    kw = scene.cloud_calls[-1][4]
    assert kw["voxel_size"] == 0.005 and kw["stride"] == 2 and np.array_equal(kw["frame"], h.robot_frame())
    # the cloud alone; and the modes without it are as before
    env = SplatEnvWrapper(_Env(), splat_handler=h, obs_modes=("pointcloud",), point_cloud=dict(n_points=3))
    env._configure_cameras(INFO)
    env.reset()
    assert list(env.step(None)[0]) == ["robot_pos", "point_cloud"]
    env = SplatEnvWrapper(_Env(), splat_handler=h, obs_modes=("rgb",))
    env._configure_cameras(INFO)
    env.reset()
    assert list(env.step(None)[0]) == ["robot_pos", "camera_0", "camera_1"]
