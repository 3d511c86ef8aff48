"""CPU: the mesh readers of sim_a_splat_amd.mesh_io (OBJ, binary and ASCII STL) and the C ABI's mesh symbol."""
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from sim_a_splat_amd import _capi
from sim_a_splat_amd.mesh_io import load_mesh, load_obj, load_stl


def test_tblock_fixture():
    v, f = load_obj(GOLDEN / "tblock_paper.obj")
    assert v.shape == (16, 3) and f.shape == (28, 3)
    assert np.allclose(v.min(0), [-0.1, -0.175, 0.0]) and np.allclose(v.max(0), [0.1, 0.025, 0.04])
    assert f.min() == 0 and f.max() == 15
    v2, f2 = load_mesh(GOLDEN / "tblock_paper.obj")
    assert np.array_equal(v, v2) and np.array_equal(f, f2)


def test_obj_forms_fans_and_negative_indices(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# quad + pentagon\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
                 "f 1/1 2/1/1 3//1 4\n"
                 "v 2 0 0\nv 3 0 0\nv 3 1 0\nv 2.5 2 0\nv 2 1 0\n"
                 "f -5 -4 -3 -2 -1\n")
    v, f = load_obj(p)
    assert v.shape == (9, 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [4, 7, 8]]


def test_obj_bad_index(tmp_path):
    p = tmp_path / "bad.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        load_obj(p)


def _tris(seed=0, n=7):
    return np.random.default_rng(seed).normal(size=(n, 3, 3)).astype(np.float32)


def test_stl_binary_and_ascii_read_equal(tmp_path):
    t = _tris()
    b = tmp_path / "m.stl"
    with open(b, "wb") as fh:
        fh.write(b"binary header".ljust(80, b"\0"))
        fh.write(struct.pack("<I", len(t)))
        for tri in t:
            fh.write(struct.pack("<3f", 0, 0, 1) + tri.astype("<f4").tobytes() + b"\0\0")
    a = tmp_path / "m_ascii.STL"
    lines = ["solid m"]
    for tri in t:
        lines += ["facet normal 0 0 1", " outer loop"] + [f"  vertex {x!r} {y!r} {z!r}" for x, y, z in tri.tolist()]
        lines += [" endloop", "endfacet"]
    a.write_text("\n".join(lines + ["endsolid m"]) + "\n")
    vb, fb = load_stl(b)
    va, fa = load_mesh(a)
    assert vb.shape == (21, 3) and np.array_equal(fb, np.arange(21).reshape(7, 3))
    assert np.array_equal(vb, t.reshape(-1, 3).astype(np.float64))
    assert np.array_equal(va, vb) and np.array_equal(fa, fb)


def test_load_mesh_rejects_unknown_suffix(tmp_path):
    p = tmp_path / "m.ply"
    p.write_text("ply\n")
    with pytest.raises(ValueError):
        load_mesh(p)


def test_mesh_symbol_bound():
    assert "sas_scene_meshes" in _capi.EXPORTS
    assert hasattr(_capi.lib(), "sas_scene_meshes")


# ---- the task mesh's pose (SplatHandler.mesh_pose_rows) against a float64 restatement of splat_handler.py:296-314 ---------
class _Msg:
    def __init__(self, robot_num, quaternion, position):
        self.num_links = len(robot_num)
        self.robot_num, self.quaternion, self.position = robot_num, quaternion, position


def _quat_matrix(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_mesh_pose_rows_restate_reference():
    from sim_a_splat_amd.handler import SplatHandler, _mesh_arrays
    rng = np.random.default_rng(3)
    h = SplatHandler.__new__(SplatHandler)
    h.blk_idx = 2
    h.scale_factor = 1.37
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    h.Ri = Q * np.sign(np.linalg.det(Q))
    h.ti = rng.normal(size=3)

    class _H:
        index = 5
    h.task_mesh_frame_handle = _H()
    qs = rng.normal(size=(4, 4)) * 3.0       # not unit: the reference normalises
    ps = rng.normal(size=(4, 3))
    msg = _Msg([3, 2, 3, 2], qs, ps)
    idx, rows = h.mesh_pose_rows(msg)
    assert idx.tolist() == [5] and rows.shape == (1, 12) and rows.dtype == np.float32
    # icp o SE3(q/|q|, p s), the LAST entry of robot_num == blk_idx (the loop assigns every one in turn)
    R = h.Ri @ _quat_matrix(qs[3])
    t = h.Ri @ (ps[3] * h.scale_factor) + h.ti
    want = np.concatenate([R, t[:, None]], 1).reshape(12)
    assert np.abs(rows[0].astype(np.float64) - want).max() < 1e-6
    assert h.mesh_pose_rows(_Msg([3, 3], qs[:2], ps[:2]))[0].size == 0
    h.task_mesh_frame_handle = None
    assert h.mesh_pose_rows(msg)[0].size == 0
    # meshes as names or arrays
    m = _mesh_arrays(("task",), str(GOLDEN), "tblock_paper.obj")
    assert m["task"][0].shape == (16, 3) and m["task"][1].shape == (28, 3)
    v, f = load_obj(GOLDEN / "tblock_paper.obj")
    assert np.array_equal(_mesh_arrays({"task": (v, f)})["task"][1], f)
    with pytest.raises(NotImplementedError):
        _mesh_arrays(("robot",))
    with pytest.raises(ValueError):
        _mesh_arrays(("task",))
