"""CPU: smooth-shaded meshes (DESIGN.md 3 "Meshes", rule 2b) -- the reference and the caps of the fixed cases the GPU tests render
(oracle/mesh_ref.py, tests/tools/mesh_smooth_cases.py), mesh welding and vertex normals, URDF material colours, and the robot
meshes of SplatHandler over a stand-in scene."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import mesh_smooth_cases as ms  # noqa: E402
from oracle import mesh_ref  # noqa: E402

from sim_a_splat_amd import mesh_io, poses, urdf_fk  # noqa: E402

_EXPECTED = {}


def _expected(name, view=0):
    """Every case's reference is computed once and shared, unchanged, by the tests below."""
    if (name, view) not in _EXPECTED:
        case = ms.FIXED_CASES[name]()
        _EXPECTED[(name, view)] = (case, mc.expected(case, view))
    return _EXPECTED[(name, view)]


# ---- the cases' caps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ms.FIXED_CASES))
def test_caps_hold(name):
    for view in range(2 if name == "mixed" else 1):
        case, e = _expected(name, view)
        print(mc.report(f"{name}[{view}]", case, e))
        assert e["excluded"] <= mc.MAX_EXCLUDED and e["driven"] >= mc.MIN_DRIVEN, mc.report(name, case, e)
        sp = e["ref"]["smooth_pixel"] & e["stable"]
        assert sp.sum() >= 150, (name, int(sp.sum()))
        # the smooth frame is not the flat one: the new tests can tell them apart
        flat = mc.expected(case, view, attributes=False)["frame"]
        assert np.abs(e["frame"]["rgb"].astype(np.float64) - flat["rgb"])[sp].max() > 1e-3
    if name == "sphere_dense":       # sub-pixel triangles, tile lists of thousands of records (bounding-box count)
        assert len(case["mesh"]["tris"]) == 16128
    if name == "mixed":
        w = e["ref"]["winner"][e["stable"]]
        assert (e["ref"]["smooth"][w[w >= 0]]).any() and (~e["ref"]["smooth"][w[w >= 0]]).any()     # flat and smooth winners in one frame


def test_sphere_triangle_counts():
    for name, tris in (("sphere_qvga", 2208), ("sphere_small", 224), ("sphere_ragged", 120), ("sphere_dense", 16128)):
        v, f, n = ms.uv_sphere(*ms.SPHERES[name][5:])
        assert len(f) == tris and np.allclose(np.linalg.norm(n, axis=1), 1.0) and f.max() == len(v) - 1


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_reference_reproduces_an_affine_field_at_the_hit_point():
    """Independent check of the perspective correction: attributes that are an affine function of position, interpolated with the
    reference's beta, equal that function at X(p) = z(p) * ray(p) -- z from mesh_ref's own depth, not from beta."""
    case, e = _expected("near_clip")
    ref = e["ref"]
    V, K, W, H = case["cams"][0]
    Km = np.asarray(K, np.float32).astype(np.float64)
    Vd = np.asarray(V, np.float64)
    hit = ref["winner"] >= 0
    ys, xs = np.mgrid[0:H, 0:W]
    D = np.stack([((xs + 0.5) - Km[0, 2]) / Km[0, 0], ((ys + 0.5) - Km[1, 2]) / Km[1, 1], np.ones((H, W))], -1)
    to_world = lambda pc: (pc - Vd[:3, 3]) @ Vd[:3, :3]
    field_at_hit = ms.near_clip_field(to_world(D[hit] * ref["z"][hit][:, None]))
    corners = ms.near_clip_field(to_world(ref["camera_vertices"].astype(np.float64)))         # [T,3,3]
    got = np.einsum("pk,pkc->pc", ref["beta"][hit], corners[ref["winner"][hit]])
    assert hit.sum() > 3000 and np.abs(got - field_at_hit).max() <= 1e-12
    assert np.abs(ref["beta"][hit].sum(1) - 1.0).max() <= 1e-12
    # ... and with the float32 colours the case uploads, the frame's colour is that field to float32 rounding (ka 1, kd 0)
    assert np.abs(ref["color64"][hit] - field_at_hit).max() <= 1e-6
    # the clipped triangles are really clipped: a corner behind the near plane, and both triangles win pixels
    assert (ref["camera_vertices"][:, :, 2] < 0.01).any(axis=1).all() and set(np.unique(ref["winner"][hit])) == {0, 1}


def test_zero_normals_give_the_flat_reference_bit_for_bit():
    case, e = _expected("sphere_small")
    m = case["mesh"]
    V, K, W, H = case["cams"][0]
    args = (m["verts"], m["tris"], m["cols"], m["groups"], case["poses"][0], m["ka"], m["kd"], V, K, W, H)
    flat = mesh_ref.reference(*args)
    zero = mesh_ref.reference(*args, vertex_normals=np.zeros_like(m["normals"]), vertex_colors=m["vcols"])
    assert not zero["smooth"].any() and np.array_equal(zero["color"].view(np.uint8), flat["color"].view(np.uint8))
    # one missing (or non-finite) normal keeps every triangle around that vertex flat, and only those
    n = m["normals"].copy()
    n[5] = np.nan
    part = mesh_ref.reference(*args, vertex_normals=n, vertex_colors=m["vcols"])
    around = (m["tris"] == 5).any(1)
    assert np.array_equal(part["smooth"], ~around) and around.sum() >= 4


# ---- welding and normals ------------------------------------------------------------------------------------------------------------
def _soup(v, f):
    """Every face with three private vertices, as load_stl returns a mesh."""
    return np.asarray(v, np.float64)[np.asarray(f).reshape(-1)], np.arange(3 * len(f)).reshape(-1, 3)


def test_weld_and_vertex_normals_on_a_cube_and_an_octahedron():
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    cf = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    of = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    for v, f, nv in ((cube, cf, 8), (octa, of, 6)):
        sv, sf = _soup(v, f)
        assert len(sv) == 3 * len(f)
        wv, wf = mesh_io.weld(sv, sf)
        assert wv.shape == (nv, 3) and wf.shape == f.shape and np.array_equal(wv[wf], sv[sf])      # same triangles on shared vertices
        assert {tuple(r) for r in wv} == {tuple(r) for r in v}
        n = mesh_io.vertex_normals(wv, wf)
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15
        assert np.abs(n - wv / np.linalg.norm(wv, axis=1, keepdims=True)).max() < 1e-12               # radial, by symmetry (angle weights)
    # bit-equal float32 positions merge, the nearest other float32 does not; degenerate input gives a zero normal
    a = np.float32(0.1)
    v = np.array([[a, 0, 0], [0, 1, 0], [0, 0, 1], [np.float64(a) + 1e-12, 0, 0], [np.nextafter(a, np.float32(1)), 0, 0]], np.float64)
    wv, wf = mesh_io.weld(v, [[0, 1, 2], [3, 1, 2], [4, 1, 2]])
    assert len(wv) == 4 and wf.tolist() == [[0, 1, 2], [0, 1, 2], [3, 1, 2]]
    n = mesh_io.vertex_normals([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5]], [[0, 1, 2]])
    assert np.array_equal(n, np.zeros((4, 3)))
    assert mesh_io.weld(np.zeros((0, 3)), np.zeros((0, 3), int))[0].shape == (0, 3)


def test_golden_xarm6_base_loads_and_welds():
    v, f = mesh_io.load_mesh(mc.GOLDEN / "xarm6_base.stl")
    assert f.shape == (2464, 3) and v.shape == (7392, 3)
    wv, wf = mesh_io.weld(v, f)
    assert len(wv) < 3 * 2464 and len(wv) < 2000 and np.array_equal(wv[wf].astype(np.float32), v[f].astype(np.float32))
    n = mesh_io.vertex_normals(wv, wf)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-12


# ---- URDF materials ------------------------------------------------------------------------------------------------------------------
URDF = """<robot name="two">
  <material name="Silver"><color rgba="0.753 0.753 0.753 1.0"/></material>
  <material name="Textured"><texture filename="x.png"/></material>
  <link name="base"><visual><origin xyz="0 0 0.5"/><geometry><mesh filename="package://two_description/meshes/base.obj" scale="2 2 2"/></geometry>
      <material name="Silver"/></visual></link>
  <link name="arm">
    <visual><geometry><mesh filename="package://two_description/meshes/arm.stl"/></geometry><material name="own"><color rgba="0.1 0.2 0.3 0.5"/></material></visual>
    <visual><geometry><box size="1 1 1"/></geometry><material name="Silver"/></visual>
    <visual><geometry><mesh filename="package://two_description/meshes/base.obj"/></geometry></visual>
    <visual><geometry><mesh filename="package://two_description/meshes/base.obj"/></geometry><material name="Textured"/></visual>
  </link>
  <joint name="j" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 0.2"/><axis xyz="0 0 1"/></joint>
</robot>"""


def test_urdf_material_colours_inline_and_named():
    rb = urdf_fk.load(URDF)
    assert np.allclose(rb.visuals["base"][0].color, [0.753, 0.753, 0.753])          # by name, from the robot-level table
    arm = rb.visuals["arm"]
    assert np.allclose(arm[0].color, [0.1, 0.2, 0.3])                               # inline rgba: RGB only
    assert np.allclose(arm[1].color, [0.753, 0.753, 0.753]) and arm[1].mesh is None
    assert arm[2].color is None and arm[3].color is None                            # no material; a named one without a colour
    assert len(urdf_fk.visual_mesh_fk(rb, [0.3])) == 4                              # the forward kinematics are what they were


# ---- SplatHandler(meshes=("robot",)) over a stand-in scene ----------------------------------------------------------------------------
class _Scene:
    """Plays SplatScene: keeps what it is given; handles with settable wxyz / position."""

    def __init__(self):
        self.handles, self.meshes = [], []

    def _handle(self, name, wxyz, position):
        h = types.SimpleNamespace(name=name, index=len(self.handles), wxyz=np.asarray(wxyz, float), position=np.asarray(position, float))
        self.handles.append(h)
        return h

    def add_gaussian_splats(self, name, centers, covariances, rgbs, opacities, wxyz=(1.0, 0, 0, 0), position=(0.0, 0, 0)):
        return self._handle(name, wxyz, position)

    def add_mesh_simple(self, name, vertices, faces, color=(0.5, 0.5, 0.5), wxyz=(1.0, 0, 0, 0), position=(0.0, 0, 0), scale=1.0,
                        vertex_normals=None, vertex_colors=None):
        h = self._handle(name, wxyz, position)
        self.meshes.append(dict(name=name, v=np.asarray(vertices), f=np.asarray(faces), color=color, scale=scale, n=vertex_normals, vc=vertex_colors,
                                handle=h))
        return h


def _write_obj(path, v, f):
    path.write_text("".join(f"v {a} {b} {c}\n" for a, b, c in v) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f))


def _write_stl(path, v, f):
    import struct
    tri = np.asarray(v, np.float32)[np.asarray(f)]
    path.write_bytes(b"\0" * 80 + struct.pack("<I", len(tri)) + b"".join(struct.pack("<12fH", 0, 0, 0, *t.reshape(-1), 0) for t in tri))


def test_handler_robot_meshes_over_a_synthesised_urdf(tmp_path):
    from sim_a_splat_amd import io
    from sim_a_splat_amd.handler import ROBOT_MESH_DEFAULT_COLOR, SplatHandler
    import torch
    rng = np.random.default_rng(3)
    n = 30
    assets = tmp_path / "assets" / "scene"
    mdir = assets / "masks" / "two-1"
    mdir.mkdir(parents=True)
    gid = rng.integers(0, 3, size=n)
    io.save_link_masks(mdir / "link_masks_global_dict.npz", {f"link{i}": gid == i for i in range(2)})
    ang = 0.3
    icp = np.eye(4)
    icp[:3, :3] = 2.5 * np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    icp[:3, 3] = (0.2, -0.1, 0.05)
    np.save(mdir / "icp_transformation.npy", icp)
    np.save(mdir / "joint_config.npy", np.array([0.4]))
    run = assets / "splatfacto" / "run"
    (run / "nerfstudio_models").mkdir(parents=True)
    (run / "config.yml").write_text("sh_degree: 3\n")
    sd = {"pipeline": {f"_model.gauss_params.{k}": torch.from_numpy(v.astype(np.float32)) for k, v in dict(
        means=rng.normal(size=(n, 3)), scales=rng.normal(-4, 0.3, size=(n, 3)), quats=rng.normal(size=(n, 4)),
        features_dc=rng.normal(size=(n, 3)), features_rest=rng.normal(size=(n, 15, 3)), opacities=rng.normal(size=(n, 1))).items()}}
    torch.save(sd, run / "nerfstudio_models" / "step-000000001.ckpt")
    pkg = tmp_path / "ros"
    desc = pkg / "two_description"
    (desc / "urdf").mkdir(parents=True)
    (desc / "meshes").mkdir()
    (desc / "urdf" / "two.urdf").write_text(URDF)
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.1
    of = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    _write_obj(desc / "meshes" / "base.obj", octa, of)
    _write_stl(desc / "meshes" / "arm.stl", octa * 0.5, of)
    scene = _Scene()
    weld = np.array([0.0, 0.02, 0.1])
    h = SplatHandler(str(assets), "two-1", "run/config.yml", str(pkg), "two_description/", "two.urdf",
                     sim_robot_weld_frame_transform=types.SimpleNamespace(translation=lambda: weld), server=scene, meshes=("robot",))
    # for every link in URDF order, every visual with a mesh: base.obj, arm.stl, base.obj, base.obj -- one smooth mesh each
    assert [m["name"] for m in scene.meshes] == [f"two-1/mesh_robot/link{i}" for i in range(4)]
    assert [len(m["f"]) for m in scene.meshes] == [8, 8, 8, 8] and [len(m["v"]) for m in scene.meshes] == [6, 6, 6, 6]   # the STL's 24 welded to 6
    assert all(abs(m["scale"] - h.scale_factor) < 1e-15 for m in scene.meshes) and abs(h.scale_factor - 2.5) < 1e-12
    # neither the visual's <origin> nor the mesh scale is applied (the reference's behaviour); the triangles are the files'
    assert np.allclose(scene.meshes[0]["v"][scene.meshes[0]["f"]], octa[of]) and np.allclose(scene.meshes[1]["v"][scene.meshes[1]["f"]], 0.5 * octa[of])
    assert np.allclose(scene.meshes[0]["color"], [0.753] * 3) and np.allclose(scene.meshes[1]["color"], [0.1, 0.2, 0.3])
    assert tuple(scene.meshes[2]["color"]) == ROBOT_MESH_DEFAULT_COLOR == (0.5, 0.5, 0.5)
    for m in scene.meshes:
        assert m["vc"] is None and np.abs(m["n"] - m["v"] / np.linalg.norm(m["v"], axis=1, keepdims=True)).max() < 1e-6
    assert h.task_mesh_frame_handle is None and len(h.mesh_frame_handles) == 4
    # draw: the k-th message link of the robot poses mesh k with icp o SE3(q / |q|, (p + weld) s); surplus links are ignored
    q = rng.normal(size=(6, 4))
    p = rng.normal(size=(6, 3))
    msg = types.SimpleNamespace(num_links=6, robot_num=[3, 2, 3, 3, 3, 3], quaternion=list(q), position=list(p))
    idx, rows = h.mesh_pose_rows(msg)
    assert idx.tolist() == [m["handle"].index for m in scene.meshes] == [3, 4, 5, 6] and rows.shape == (4, 12) and rows.dtype == np.float32
    s, Ri, ti = poses.decompose_icp(icp)
    for k, link in enumerate((0, 2, 3, 4)):
        R = Ri @ poses.quat_wxyz_to_matrix(q[link] / np.linalg.norm(q[link]))
        t = Ri @ ((p[link] + weld) * s) + ti
        want = np.concatenate([R, t[:, None]], 1)
        assert np.abs(rows[k].reshape(3, 4) - want).max() < 1e-6
    h.draw_handler(msg)
    for k, m in enumerate(scene.meshes):
        got = np.concatenate([poses.quat_wxyz_to_matrix(m["handle"].wxyz), np.asarray(m["handle"].position)[:, None]], 1)
        assert np.array_equal(got.astype(np.float32), rows[k].reshape(3, 4))
    # arrays instead of names; an unknown name; "robot" by name without a URDF
    h2 = SplatHandler.from_arrays(h.means, h.covs, h.colors, h.opacities, {f"link{i}": gid == i for i in range(2)}, icp, [np.eye(4)] * 2,
                                  scene=_Scene(), meshes={"robot": [(octa, of, (0.2, 0.3, 0.4))]})
    assert [hh.name for hh in h2.mesh_frame_handles] == ["robot/mesh_robot/link0"]
    with pytest.raises(NotImplementedError):
        SplatHandler.from_arrays(h.means, h.covs, h.colors, h.opacities, {}, icp, [], scene=_Scene(), meshes=("robot",))
    with pytest.raises(ValueError):
        SplatHandler.from_arrays(h.means, h.covs, h.colors, h.opacities, {}, icp, [], scene=_Scene(), meshes=("gripper",))
