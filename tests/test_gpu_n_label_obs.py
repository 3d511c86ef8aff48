"""GPU: rgb, depth and segmentation per camera from one label-frame call (SplatHandler.render_observations, the obs_modes of
CameraRig / SplatEnvWrapper), on the handler of mesh_cases.handler_setup() with the task block and the robot's meshes.  Each
modality must equal, per camera and on every pixel, what the single-modality doors deliver: SplatHandler.render,
SplatScene.get_render_float(..., mesh_surface=True)["depth"] and SplatHandler.render_segmentation."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import mesh_smooth_cases as ms  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("rgb", "depth", "segmentation")
H, W = 48, 64


class _Inner:
    """The members of the simulator env the wrapper touches, around one fixed draw message."""
    visualize_robot_flag = False

    def __init__(self, msg):
        self.msg = msg

    def reset(self, seed=None, reset_to_state=None):
        pass

    def step(self, action):
        return {}, 0.0, False, False, {}

    def render(self):
        pass

    def _get_obs(self):
        return {"robot_pos": np.zeros(2)}

    def _generate_draw_msg(self):
        return self.msg

    def close(self):
        pass


def test_observations_equal_the_single_modality_doors():
    from sim_a_splat_amd.env_wrapper import SplatEnvWrapper
    from sim_a_splat_amd.handler import SplatHandler
    hs = mc.handler_setup()
    h = SplatHandler.from_arrays(*hs["args"], device=0, meshes={"task": None, "robot": ms.robot_links()}, task_assets_path=str(mc.GOLDEN),
                                 task_assets_name="tblock_paper.obj")
    try:
        h.draw_handler(hs["msg"])
        q, p = hs["cam"]
        cams = [(q, p), (q, p + np.array([0.1, 0.05, -0.1]))]
        sizes = [[H, W], [H, W]]
        obs = h.render_observations(h.scene, cams, sizes, modes=MODES)
        rgb = h.render(h.scene, cams, sizes)
        seg = h.render_segmentation(h.scene, cams, sizes)
        names = h.scene.row_names()
        assert len(obs) == 2 and len(names) == 6
        for i, cam in enumerate(cams):
            d = obs[i]
            assert list(d) == list(MODES)
            assert d["rgb"].dtype == np.uint8 and d["rgb"].shape == (H, W, 3) and np.array_equal(d["rgb"], rgb[i])
            depth = h.scene.get_render_float(H, W, cam[0], cam[1], mesh_surface=True)["depth"].cpu().numpy()[..., 0]
            assert d["depth"].dtype == np.float32 and d["depth"].shape == (H, W)
            assert np.array_equal(d["depth"].view(np.uint32), depth.view(np.uint32))
            assert d["segmentation"].dtype == np.uint8 and d["segmentation"].shape == (H, W) and np.array_equal(d["segmentation"], seg[i])
            shown = set(np.unique(d["segmentation"]).tolist()) - {255}
            assert shown and shown <= set(range(6)), shown
            splats_only = h.scene.get_render_float(H, W, cam[0], cam[1])["depth"].cpu().numpy()[..., 0]
            assert i > 0 or (splats_only != depth).any()           # camera 0 faces the task block: the depth closes on a mesh somewhere
            print(f"camera {i}: rows shown {sorted(shown)}, meshes close the depth on {int((splats_only != depth).sum())} pixels")
        assert not np.array_equal(obs[0]["segmentation"], obs[1]["segmentation"])
        # the batched labels door by itself
        both = h.scene.get_segmentations(H, W, cams).cpu().numpy()
        assert both.shape == (2, H, W) and np.array_equal(both[0], seg[0]) and np.array_equal(both[1], seg[1])
        # the env wrapper's dict carries the same arrays, channels first
        info = {0: {"link_name": "world", "local_frame": cams[0], "type": "viewport", "render_size": [H, W]},
                1: {"link_name": "world", "local_frame": cams[1], "type": "static", "render_size": [H, W]}}
        env = SplatEnvWrapper(_Inner(hs["msg"]), splat_handler=h, obs_modes=MODES)
        env._configure_cameras(info)
        env.reset()
        o = env.step(None)[0]
        assert list(o) == ["robot_pos"] + [f"camera_{i}{s}" for i in range(2) for s in ("", "_depth", "_segmentation")]
        for i in range(2):
            assert o[f"camera_{i}"].shape == (3, H, W) and np.array_equal(np.moveaxis(o[f"camera_{i}"], 0, -1), rgb[i])
            assert o[f"camera_{i}_depth"].shape == (1, H, W) and np.array_equal(o[f"camera_{i}_depth"][0], obs[i]["depth"])
            assert o[f"camera_{i}_segmentation"].shape == (1, H, W) and np.array_equal(o[f"camera_{i}_segmentation"][0], seg[i])
        plain = SplatEnvWrapper(_Inner(hs["msg"]), splat_handler=h)
        plain._configure_cameras(info)
        plain.reset()
        o = plain.step(None)[0]
        assert list(o) == ["robot_pos", "camera_0", "camera_1"] and np.array_equal(np.moveaxis(o["camera_1"], 0, -1), rgb[1])
    finally:
        h.scene.close()
