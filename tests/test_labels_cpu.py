"""CPU: label frames above the C ABI -- the exported symbols, the label rule L restated in NumPy against rasterizer.group_labels,
and the observation plumbing (SplatHandler.render_observations, CameraRig.get_obs, SplatEnvWrapper(obs_modes=...)) over a stand-in
scene that records what it is asked for.  No GPU: the kernels' side is tests/test_gpu_n_labels.py."""
import ctypes
import types

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, build
from sim_a_splat_amd.rasterizer import group_labels


def test_label_entry_points_are_exported_and_declared():
    L = ctypes.CDLL(str(build.build()))
    for name in ("sas_render_batch_labels", "sas_render_batch_labels_posed"):
        assert name in _capi.EXPORTS and hasattr(L, name), name
    B = _capi.lib()
    # as sas_render_batch[_posed], with min_alpha (float) in front of the flags and labels behind rgb8
    assert len(B.sas_render_batch_labels.argtypes) == len(B.sas_render_batch.argtypes) + 2
    assert len(B.sas_render_batch_labels_posed.argtypes) == len(B.sas_render_batch_posed.argtypes) + 2
    assert B.sas_render_batch_labels.argtypes[7] is ctypes.c_float and B.sas_render_batch_labels_posed.argtypes[10] is ctypes.c_float


# ---- the label rule ----------------------------------------------------------------------------------------------------------------
def label_rule(w, a, min_alpha):
    """L of include/sim_a_splat_amd.h, one pixel at a time: the running (best, arg) with a strict > in ascending channel order that
    the kernel keeps, the clamp to 255, and 255 where a < min_alpha in float32."""
    w = np.asarray(w, np.float32).reshape(-1, w.shape[-1])
    a = np.asarray(a, np.float32).reshape(-1)
    out = np.empty(w.shape[0], np.uint8)
    for p in range(w.shape[0]):
        best, arg = -np.inf, 255
        for g in range(w.shape[1]):
            if w[p, g] > best:
                best, arg = w[p, g], g
        out[p] = 255 if a[p] < np.float32(min_alpha) else min(arg, 255)
    return out


@pytest.mark.parametrize("G", [1, 3, 8, 9, 256])
def test_label_rule_equals_group_labels(G):
    rng = np.random.default_rng(100 + G)
    H, W = 6, 7
    w = rng.uniform(0, 1, size=(H, W, G)).astype(np.float32)
    w[0] = 0.0                                              # all channels tie at zero (an empty pixel): the lowest id
    w[1, :, :] = np.float32(0.25)                           # all tie above zero
    for x in range(W):                                      # exact ties of the maximum between two channels, the lower one wins
        g0, g1 = sorted(rng.choice(G, size=2, replace=G < 2))
        w[2, x, g0] = w[2, x, g1] = np.float32(2.0)
    if G == 256:
        w[3, :, :] = 0.0
        w[3, :, 255] = 1.0                                  # group 255 wins: reads as none
        w[4, :, :] = 0.0
        w[4, :, 254] = 1.0
    a = rng.uniform(0, 1, size=(H, W, 1)).astype(np.float32)
    a[0, 0], a[0, 1], a[0, 2], a[0, 3] = 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.0, 0.0
    for min_alpha in (0.0, 0.5, 1.0):
        want = label_rule(w, a, min_alpha).reshape(H, W)
        got = group_labels(torch.from_numpy(w), torch.from_numpy(a), min_alpha).numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (G, min_alpha)
    got = group_labels(torch.from_numpy(w), torch.from_numpy(a), 0.0).numpy()
    assert (got[0] == 0).all() and (got[1] == 0).all()
    if G == 256:
        assert (got[3] == 255).all() and (got[4] == 254).all()
    elif G > 1:
        assert (got != 255).all()                            # min_alpha 0: nothing is 255 by the alpha rule


# ---- observation plumbing over a stand-in scene ---------------------------------------------------------------------------------------
class _Scene:
    """Plays SplatScene: records the calls, returns frames whose values name the call and the camera."""

    def __init__(self):
        self.camera = types.SimpleNamespace(wxyz=np.array([1.0, 0, 0, 0]), position=np.zeros(3), fov=1.0)
        self.rgb_calls, self.obs_calls, self.groups = [], [], []

    def add_gaussian_splats(self, name, centers, covariances, rgbs, opacities, wxyz=(1.0, 0, 0, 0), position=(0.0, 0, 0)):
        h = types.SimpleNamespace(name=name, n=len(centers), wxyz=np.asarray(wxyz, float), position=np.asarray(position, float))
        self.groups.append(h)
        return h

    def row_names(self):
        return [g.name for g in self.groups]

    def get_renders(self, height, width, cam_poses, fov=None):
        self.rgb_calls.append((height, width, len(cam_poses)))
        return np.stack([np.full((height, width, 3), 10 * len(self.rgb_calls) + i, np.uint8) for i in range(len(cam_poses))])

    def get_observations(self, height, width, cam_poses, fov=None, pose_sets=None, pose_set=None, min_alpha=0.5, want=("labels",)):
        self.obs_calls.append((height, width, len(cam_poses), tuple(want)))
        C, k = len(cam_poses), 10 * len(self.obs_calls)
        per = lambda shape, dt: torch.stack([torch.full(shape, k + i, dtype=dt) for i in range(C)])
        table = {"labels": ((height, width), torch.uint8), "rgb8": ((height, width, 3), torch.uint8), "depth": ((height, width, 1), torch.float32)}
        return {n: per(*table[n]) for n in dict.fromkeys(tuple(want) + ("labels",))}

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
        1: {"link_name": "eef", "local_frame": ((1.0, 0, 0, 0), (-0.1, 0, 0.033)), "type": "moving", "render_size": [24, 32]},
        2: {"link_name": "world", "local_frame": ((1.0, 0, 0, 0), (0.0, 0.0, 2.0)), "type": "static", "render_size": [8, 8]}}


def _handler():
    from sim_a_splat_amd.handler import SplatHandler
    n, rng, scene = 12, np.random.default_rng(0), _Scene()
    masks = {"link0": np.arange(n) < 3, "link1": (np.arange(n) >= 3) & (np.arange(n) < 5)}
    h = SplatHandler.from_arrays(rng.normal(size=(n, 3)), np.tile(np.eye(3), (n, 1, 1)), rng.uniform(size=(n, 3)), rng.uniform(size=n),
                                 masks, np.eye(4), [np.eye(4), np.eye(4)], scene=scene)
    return h, scene


def test_render_observations_groups_same_sized_cameras():
    h, scene = _handler()
    cams = [((1.0, 0, 0, 0), (0.0, 0, k)) for k in range(3)]
    sizes = [[24, 32], [8, 8], [24, 32]]
    out = h.render_observations(scene, cams, sizes, modes=("rgb", "depth", "segmentation"))
    # cameras 0 and 2 in one call, camera 1 in another; nothing went through the rgb-only path
    assert scene.obs_calls == [(24, 32, 2, ("rgb8", "depth", "labels")), (8, 8, 1, ("rgb8", "depth", "labels"))] and scene.rgb_calls == []
    assert [list(d) for d in out] == [["rgb", "depth", "segmentation"]] * 3
    for i, (hw, val) in enumerate((((24, 32), 10), ((8, 8), 20), ((24, 32), 11))):
        d = out[i]
        assert d["rgb"].shape == hw + (3,) and d["rgb"].dtype == np.uint8 and (d["rgb"] == val).all()
        assert d["depth"].shape == hw and d["depth"].dtype == np.float32 and (d["depth"] == val).all()
        assert d["segmentation"].shape == hw and d["segmentation"].dtype == np.uint8 and (d["segmentation"] == val).all()
    # only what is asked for is rendered; rgb alone keeps render's path
    scene.obs_calls.clear()
    out = h.render_observations(scene, cams[:1], sizes[:1], modes=("segmentation",))
    assert scene.obs_calls == [(24, 32, 1, ("labels",))] and list(out[0]) == ["segmentation"]
    scene.obs_calls.clear()
    out = h.render_observations(scene, cams, sizes, modes=("rgb",))
    assert scene.obs_calls == [] and len(scene.rgb_calls) == 2 and out[1]["rgb"].shape == (8, 8, 3)
    with pytest.raises(ValueError):
        h.render_observations(scene, cams, sizes, modes=("rgb", "normals"))


def test_camera_rig_obs_modes():
    from sim_a_splat_amd.handler import CameraRig
    h, scene = _handler()
    rig = CameraRig(INFO)
    msg = _Env()._generate_draw_msg()
    obs = rig.get_obs(h, msg)
    assert list(obs) == ["camera_0", "camera_1", "camera_2"] and scene.obs_calls == []
    assert obs["camera_0"].shape == (3, 24, 32) and obs["camera_2"].shape == (3, 8, 8) and obs["camera_0"].dtype == np.uint8
    obs = rig.get_obs(h, msg, obs_modes=("rgb", "depth", "segmentation"))
    assert list(obs) == [f"camera_{i}{s}" for i in range(3) for s in ("", "_depth", "_segmentation")]
    assert [(c[0], c[1], c[2]) for c in scene.obs_calls] == [(24, 32, 2), (8, 8, 1)]
    assert obs["camera_1"].shape == (3, 24, 32) and obs["camera_1"].dtype == np.uint8
    assert obs["camera_1_depth"].shape == (1, 24, 32) and obs["camera_1_depth"].dtype == np.float32
    assert obs["camera_2_segmentation"].shape == (1, 8, 8) and obs["camera_2_segmentation"].dtype == np.uint8
    with pytest.raises(ValueError):
        rig.get_obs(h, msg, obs_modes=("rgb", "flow"))


def test_env_wrapper_obs_modes():
    from sim_a_splat_amd.env_wrapper import SplatEnvWrapper
    h, scene = _handler()
    env = SplatEnvWrapper(_Env(), splat_handler=h)
    env._configure_cameras(INFO)
    env.reset()
    obs = env.step(np.zeros(2))[0]
    assert list(obs) == ["robot_pos", "camera_0", "camera_1", "camera_2"] and scene.obs_calls == []      # the default: as before
    assert obs["camera_0"].shape == (3, 24, 32) and obs["camera_0"].dtype == np.uint8
    h2, scene2 = _handler()
    env = SplatEnvWrapper(_Env(), splat_handler=h2, obs_modes=("rgb", "depth", "segmentation"))
    env._configure_cameras(INFO)
    env.reset()
    obs = env.step(np.zeros(2))[0]
    assert list(obs) == ["robot_pos"] + [f"camera_{i}{s}" for i in range(3) for s in ("", "_depth", "_segmentation")]
    assert obs["camera_0"].shape == (3, 24, 32) and obs["camera_0"].dtype == np.uint8
    assert obs["camera_0_depth"].shape == (1, 24, 32) and obs["camera_0_depth"].dtype == np.float32
    assert obs["camera_2_segmentation"].shape == (1, 8, 8) and obs["camera_2_segmentation"].dtype == np.uint8
    assert [(c[0], c[1], c[2]) for c in scene2.obs_calls] == [(24, 32, 2), (8, 8, 1)] and scene2.rgb_calls == []
    env = SplatEnvWrapper(_Env(), splat_handler=h2, obs_modes=("depth",))
    env._configure_cameras(INFO)
    env.reset()
    assert list(env.step(np.zeros(2))[0]) == ["robot_pos", "camera_0_depth", "camera_1_depth", "camera_2_depth"]
    with pytest.raises(ValueError):
        SplatEnvWrapper(_Env(), splat_handler=h2, obs_modes=("rgb", "thermal"))


# ---- the drawn mesh cases of the GPU label test stay inside the kit's cap, for the reference alone -----------------------------------------
def test_drawn_label_seeds_meet_the_cap():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import mesh_cases as mc
    import mesh_feature_cases as mf
    from test_gpu_n_labels import DRAWN_SEEDS
    assert len(DRAWN_SEEDS) == 2
    for case in [mf.case_labels()] + [mf.drawn_case(s) for s in DRAWN_SEEDS]:
        e = mc.expected(case, 0)
        want = mf.expected_labels(case, e)["labels"]
        assert e["excluded"] <= mc.MAX_EXCLUDED, (case.get("describe"), e["excluded"])
        assert case["sc"]["G"] >= 3 and case["mesh"]["groups"] is not None
        shown = set(np.unique(want[e["stable"]]).tolist()) - {255}
        assert len(shown) >= 2 and shown & set(np.unique(case["mesh"]["groups"]).tolist()), shown   # splat rows and a mesh row show
