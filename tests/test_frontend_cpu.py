"""CPU: the Python front end's shared pieces -- the message reader of SplatHandler (mesh and link entries), the camera packer and
row registration of SplatScene, and Rasterizer._outputs -- held to restatements written here with the same operations, so that
every comparison is exact."""
import types

import numpy as np
import pytest
import torch

from sim_a_splat_amd import poses
from sim_a_splat_amd.handler import SplatHandler


def _msg(robot_num, q, p):
    return types.SimpleNamespace(num_links=len(robot_num), robot_num=list(robot_num), quaternion=q, position=p)


def _row(wxyz, t) -> np.ndarray:
    """The float32 pose row of a handle holding (wxyz, t): what SplatScene writes into its block."""
    row = np.zeros((3, 4), np.float32)
    row[:, :3] = poses.quat_wxyz_to_matrix(wxyz)
    row[:, 3] = t
    return row.reshape(12)


def _rotation(rng) -> np.ndarray:
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


# ---- 1. mesh pose rows, bit for bit --------------------------------------------------------------------------------------------
def test_mesh_pose_rows_are_the_reference_operations_bit_for_bit():
    rng = np.random.default_rng(11)
    h = SplatHandler.__new__(SplatHandler)
    h.rbt_idx, h.blk_idx, h.scale_factor = 3, 2, 1.37
    h.Ri, h.ti, h.weld_translation = _rotation(rng), rng.normal(size=3), np.array([0.05, -0.02, 0.11])
    h.task_mesh_frame_handle = types.SimpleNamespace(index=5)
    h.mesh_frame_handles = [types.SimpleNamespace(index=6), types.SimpleNamespace(index=7)]
    robot_num = [3, 2, 3, 2, 3]                        # interleaved; two task entries (the last counts), a surplus robot entry
    q, p = rng.normal(size=(5, 4)) * 3.0, rng.normal(size=(5, 3))
    idx, rows = h.mesh_pose_rows(_msg(robot_num, q, p))
    assert idx.tolist() == [5, 6, 7] and rows.shape == (3, 12) and rows.dtype == np.float32

    def want(i, welded):
        qn = q[i] / np.linalg.norm(q[i])
        R = h.Ri @ poses.quat_wxyz_to_matrix(qn)
        t = h.Ri @ ((p[i] + h.weld_translation) * h.scale_factor) + h.ti if welded else h.Ri @ (p[i] * h.scale_factor) + h.ti
        return _row(poses.matrix_to_quat_wxyz(R), t)

    assert np.array_equal(rows[0], want(3, False))
    assert np.array_equal(rows[1], want(0, True)) and np.array_equal(rows[2], want(2, True))
    assert not np.array_equal(rows[0], want(1, False))             # the first task entry is not the one
    h.mesh_frame_handles = []
    assert h.mesh_pose_rows(_msg(robot_num, q, p))[0].tolist() == [5]


# ---- 2. draw_handler's NumPy path writes the rows link_pose_rows / mesh_pose_rows report ------------------------------------------
class _PlainScene:
    """Plays SplatScene with plain handles (no lock, no link fast path): draw_handler takes its NumPy path."""

    def __init__(self):
        self.handles = []

    def add_gaussian_splats(self, name, centers, covariances, rgbs, opacities, wxyz=(1.0, 0, 0, 0), position=(0.0, 0, 0)):
        h = types.SimpleNamespace(name=name, index=len(self.handles), wxyz=np.asarray(wxyz, float), position=np.asarray(position, float))
        self.handles.append(h)
        return h

    def add_mesh_simple(self, name, vertices, faces, color=(0.5, 0.5, 0.5), wxyz=(1.0, 0, 0, 0), position=(0.0, 0, 0), scale=1.0,
                        vertex_normals=None, vertex_colors=None):
        return self.add_gaussian_splats(name, (), None, None, None, wxyz, position)


@pytest.mark.parametrize("robot_num", [[3, 3, 2, 3, 3, 2], [3, 3, 3, 3, 2]], ids=["gather", "leading"])
def test_draw_handler_writes_the_rows_the_row_functions_report(robot_num):
    rng = np.random.default_rng(5)
    n, K = 20, 3
    icp = np.eye(4)
    icp[:3, :3], icp[:3, 3] = 1.7 * _rotation(rng), rng.normal(size=3)
    fk = []
    for _ in range(K):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = _rotation(rng), rng.normal(size=3)
        fk.append(T)
    tetra = (np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
    h = SplatHandler.from_arrays(rng.normal(size=(n, 3)), np.tile(np.eye(3), (n, 1, 1)), rng.uniform(size=(n, 3)), rng.uniform(size=n),
                                 {f"link{j}": np.arange(n) % (K + 1) == j for j in range(K)}, icp, fk, weld_translation=(0.1, -0.2, 0.3),
                                 scene=_PlainScene(), meshes={"task": tetra, "robot": [tetra + ((0.2, 0.3, 0.4),)] * 2})
    assert not h._fast
    m = len(robot_num)
    msg = _msg(robot_num, (rng.normal(size=(m, 4)) * 3.0).tolist(), rng.normal(size=(m, 3)).tolist())
    groups, link_rows = h.link_pose_rows(msg)
    midx, mesh_rows = h.mesh_pose_rows(msg)
    assert groups.tolist() == [0, 1, 2] and midx.tolist() == [K + 1, K + 2, K + 3]        # a surplus robot entry drives nothing
    before = [(g.wxyz.copy(), g.position.copy()) for g in h.scene.handles]
    h.draw_handler(msg)
    by_index = {g.index: g for g in h.scene.handles}
    for g, row in list(zip(groups, link_rows)) + list(zip(midx, mesh_rows)):
        assert np.array_equal(_row(by_index[g].wxyz, by_index[g].position), row), g
    rest = by_index[K]                                                                   # "/scene_ohne_robot" is nobody's link
    assert np.array_equal(rest.wxyz, before[K][0]) and np.array_equal(rest.position, before[K][1])


# ---- 3. the 256 pose rows are shared by splat groups and meshes, and checked where a row is registered ------------------------------
def test_the_257th_row_is_refused_at_the_call(monkeypatch):
    from sim_a_splat_amd import scene as scene_mod
    monkeypatch.setattr(scene_mod, "Rasterizer", lambda device: types.SimpleNamespace(close=lambda: None))
    sc = scene_mod.SplatScene(0)
    tri = (np.eye(3), [[0, 1, 2]])
    gauss = (np.zeros((1, 3)), np.eye(3)[None], np.ones((1, 3)), np.ones(1))
    for k in range(200):
        sc.add_mesh_simple(f"m{k}", *tri)
    for k in range(56):
        sc.add_gaussian_splats(f"g{k}", *gauss)
    assert len(sc._handles) == 256 and sc._Rt.shape == (256, 3, 4) and sc._groups[-1]["row"] == 255
    with pytest.raises(RuntimeError, match="at most 256 splat groups and meshes"):
        sc.add_gaussian_splats("one too many", *gauss)
    with pytest.raises(RuntimeError, match="at most 256 splat groups and meshes"):
        sc.add_mesh_simple("one too many", *tri)
    assert len(sc._handles) == 256 and len(sc._groups) == 56 and len(sc._meshes) == 200 and sc._Rt.shape == (256, 3, 4)


# ---- 4. Rasterizer._outputs: a table entry without a channel axis -----------------------------------------------------------------
def test_outputs_without_a_channel_axis():
    from sim_a_splat_amd.rasterizer import Rasterizer
    r = types.SimpleNamespace(device=torch.device("cpu"))
    table = Rasterizer._LABEL_SHAPES
    C, H, W = 3, 5, 7
    res, ptrs = Rasterizer._outputs(r, ("rgb8", "labels"), table, H, W, None, C)
    assert res["labels"].shape == (C, H, W) and res["labels"].dtype == torch.uint8 and res["rgb8"].shape == (C, H, W, 3)
    assert ptrs["labels"] == res["labels"].data_ptr() and ptrs["depth"] is None
    assert Rasterizer._outputs(r, ("labels",), table, H, W, None)[0]["labels"].shape == (H, W)
    mine = torch.zeros((C, H, W), dtype=torch.uint8)
    res, ptrs = Rasterizer._outputs(r, ("labels",), table, H, W, {"labels": mine}, C)
    assert res["labels"] is mine and ptrs["labels"] == mine.data_ptr()
    for bad in (torch.zeros((C, H, W), dtype=torch.int8), torch.zeros((C, H, W, 1), dtype=torch.uint8), torch.zeros((C, H, W + 1), dtype=torch.uint8),
                torch.zeros((C, W, H), dtype=torch.uint8).transpose(1, 2)):
        with pytest.raises(ValueError, match=r"out\['labels'\] must be a contiguous torch.uint8 tensor \(3, 5, 7\) on cpu"):
            Rasterizer._outputs(r, ("labels",), table, H, W, {"labels": bad}, C)
    assert "labels" not in Rasterizer._SHAPES                      # render / render_batch still refuse it (KeyError)


# ---- 5. camera packing ------------------------------------------------------------------------------------------------------------
def test_camera_arrays_and_the_views_a_posed_batch_passes(monkeypatch):
    from sim_a_splat_amd import scene as scene_mod
    rng = np.random.default_rng(8)
    cams = [((0.5, 0.5, -0.5, 0.5), (1.0, 2.0, 3.0)), ([0.0, 2.0, 0.0, 0.0], [0.25, -1.0, 0.5]),
            (rng.normal(size=4).astype(np.float32), rng.normal(size=3).astype(np.float32)), (rng.normal(size=4), (0, 0, 1))]
    C = len(cams)
    q0, p0 = np.empty((C, 4), np.float64), np.empty((C, 3), np.float64)
    for c, (w, x) in enumerate(cams):
        q0[c], p0[c] = w, x
    q, p = scene_mod._camera_arrays(cams)
    assert q.dtype == p.dtype == np.float64 and np.array_equal(q, q0) and np.array_equal(p, p0)
    assert scene_mod._camera_arrays([])[0].shape == (0, 4)

    class _Raster:
        def __init__(self, device):
            self.calls = []

        def upload(self, *a, **k):
            pass

        def render_batch_host(self, V, K, W, H, bg, out=None, pose_sets=None, pose_set=None):
            self.calls.append((V, K, W, H))
            return torch.zeros((V.shape[0], H, W, 3), dtype=torch.uint8)

        def close(self):
            pass

    monkeypatch.setattr(scene_mod, "Rasterizer", _Raster)
    sc = scene_mod.SplatScene(0)
    H, W, fov = 24, 32, 1.1
    sc.get_renders_posed(H, W, cams, np.zeros((1, 0, 12), np.float32), [0] * C, fov=fov)
    V, K, w_, h_ = sc._raster.calls[0]
    Vw, Kw = sc._views_and_Ks(H, W, q0, p0, fov)
    assert (w_, h_) == (W, H) and V.dtype == np.float32 and np.array_equal(V, Vw) and np.array_equal(K, Kw)
    sc.get_renders_posed(H, W, cams, np.zeros((1, 0, 12), np.float32), [0] * C)        # the client's own field of view
    assert np.array_equal(sc._raster.calls[1][1], sc._views_and_Ks(H, W, q0, p0, sc.camera.fov)[1])
    # one camera is the batch of one: the single-view form written out (camera-to-world R, t -> world-to-camera; vertical fov)
    for c in range(C):
        R = poses.quat_wxyz_to_matrix(q0[c])
        V1 = np.eye(4)
        V1[:3, :3] = R.T
        V1[:3, 3] = -poses.mv3(R.T, p0[c])
        f = 0.5 * H / np.tan(0.5 * fov)
        K1 = np.array([[f, 0, 0.5 * W], [0, f, 0.5 * H], [0, 0, 1]])
        Vs, Ks = sc._view_and_K(H, W, cams[c][0], cams[c][1], fov)
        assert np.array_equal(Vs, V1.astype(np.float32)) and np.array_equal(Ks, K1.astype(np.float32))
        assert np.array_equal(Vs, Vw[c]) and np.array_equal(Ks, Kw[c])
