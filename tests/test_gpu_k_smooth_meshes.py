"""GPU: smooth-shaded meshes (DESIGN.md 3 "Meshes", rule 2b) against the float64 reference of oracle/mesh_ref.py + the
depth-limited oracle, on the cases of tests/tools/mesh_smooth_cases.py (their caps are settled on the CPU: test_smooth_meshes_cpu.py).

On the reference's stable pixels: alpha and depth bit-equal to the expected frame, rgb within 1e-4 (the project's parity gate: the
kernel interpolates float32 attribute planes, the reference float64 barycentrics), rgb8 within 1 LSB; where the winner is a flat
triangle or none, every output bit-equal.  Each check prints the measured maximum.  Every test fails without the feature: the
keywords and the entry point do not exist, and SplatHandler refuses "robot".  They run unchanged under the bounds-checked build.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

from sim_a_splat_amd.rasterizer import Rasterizer

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import mesh_smooth_cases as ms  # noqa: E402

pytestmark = pytest.mark.gpu
OUTS = mc.OUTS


@pytest.fixture
def rasterizer():
    r = Rasterizer(0)
    yield r
    r.close()


_expect, _single = mc.expect, mc.single


def _check(got, e, what):
    probs, err, err8 = mc.compare(got, e)
    n = int((e["stable"] & e["ref"]["smooth_pixel"]).sum())
    print(f"  {what}: {n} stable smooth pixels, max |rgb - reference| = {err:.3e}, max rgb8 difference = {err8:.0f} LSB")
    assert not probs, (what, probs)
    assert n > 0


# ---- the spheres ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ms.SPHERES))
def test_smooth_sphere_among_the_splats(rasterizer, name):
    case = ms.FIXED_CASES[name]()
    mc.upload_case(rasterizer, case)
    rasterizer.set_group_poses(case["poses"][0])
    _check(_single(rasterizer, case), _expect(name, case), name)


def test_real_link_xarm6_base(rasterizer):
    case = ms.case_xarm6_base()
    assert len(case["mesh"]["verts"]) < 3 * len(case["mesh"]["tris"]) and case["mesh"]["vcols"] is None
    mc.upload_case(rasterizer, case)
    rasterizer.set_group_poses(case["poses"][0])
    _check(_single(rasterizer, case), _expect("xarm6_base", case), "xarm6_base")


# ---- flat and smooth meshes in one upload --------------------------------------------------------------------------------------------
def test_mixed_flat_block_and_smooth_sphere(rasterizer):
    case = ms.case_mixed()
    V, K, W, H = case["cams"][0]
    sets = np.stack(case["poses"]).astype(np.float32)
    mc.upload_case(rasterizer, case)
    es = [_expect("mixed", case, v) for v in range(2)]
    for v in range(2):
        w = es[v]["ref"]["winner"][es[v]["stable"]]
        sm = es[v]["ref"]["smooth"][w[w >= 0]]
        assert sm.any() and not sm.all()                     # flat and smooth winners in the frame
        rasterizer.set_group_poses(sets[v])
        _check(_single(rasterizer, case, v), es[v], f"mixed, pose set {v}")
    order = [1, 0, 1]
    b = mc.to_numpy(rasterizer.render_batch(np.stack([V] * 3), np.stack([K] * 3), W, H, case["bg"], want=OUTS, pose_sets=sets, pose_set=order))
    for k, s in enumerate(order):
        _check({q: b[q][k] for q in b}, es[s], f"mixed, render_batch view {k} pose set {s}")


# ---- a smooth quad across the near plane --------------------------------------------------------------------------------------------
def test_near_clipped_quad_shows_the_affine_field(rasterizer):
    case = ms.case_near_clip()
    V, K, W, H = case["cams"][0]
    mc.upload_case(rasterizer, case)
    e = _expect("near_clip", case)
    got = _single(rasterizer, case)
    _check(got, e, "near_clip")
    # ka = 1, kd = 0, colours affine in the world position: where nothing lies in front (T = 1) the pixel IS the field at its hit point
    ref = e["ref"]
    clear = e["stable"] & ref["smooth_pixel"] & (e["frame"]["alpha"][..., 0] == 0.0)
    assert clear.sum() >= 500 and set(np.unique(ref["winner"][clear])) == {0, 1}
    Km, Vd = np.asarray(K, np.float32).astype(np.float64), np.asarray(V, np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    D = np.stack([((xs + 0.5) - Km[0, 2]) / Km[0, 0], ((ys + 0.5) - Km[1, 2]) / Km[1, 1], np.ones((H, W))], -1)
    field = ms.near_clip_field((D[clear] * ref["z"][clear][:, None] - Vd[:3, 3]) @ Vd[:3, :3])
    err = float(np.abs(got["rgb"][clear].astype(np.float64) - field).max())
    print(f"  near_clip: {int(clear.sum())} pixels with T = 1, max |rgb - affine field| = {err:.3e}")
    assert err <= ms.RGB_TOL


# ---- every entry point -----------------------------------------------------------------------------------------------------------------
def test_entry_points(rasterizer):
    r = rasterizer
    case = ms.FIXED_CASES["entry_points"]()
    V, K, W, H = case["cams"][0]
    p0 = case["poses"][0]
    p1 = ms.pose_rows(case["sc"], 2, (0.2, -0.5, 1.1), (0.1, 0.0, 0.2))
    bg = case["bg"]
    mc.upload_case(r, case)
    r.set_group_poses(p0)
    e0, e1 = _expect("entry_points", case), _expect("entry_points", dict(case, poses=[p1]))
    assert not np.array_equal(e0["frame"]["rgb8"], e1["frame"]["rgb8"])
    _check(_single(r, case), e0, "render")
    g = mc.to_numpy(r.render_rgbd(V, K, W, H, bg, max_depth=None, depth_fill_max=False))
    _check({k: g[k] for k in ("rgb", "alpha", "depth")}, e0, "render_rgbd")
    Vs, Ks = np.stack([V, V]), np.stack([K, K])
    b = mc.to_numpy(r.render_batch(Vs, Ks, W, H, bg, want=OUTS))
    for k in range(2):
        _check({q: b[q][k] for q in b}, e0, f"render_batch view {k}")
    b = mc.to_numpy(r.render_batch(Vs, Ks, W, H, bg, want=OUTS, pose_sets=np.stack([p0, p1]), pose_set=[1, 0]))
    for k, e in enumerate((e1, e0)):
        _check({q: b[q][k] for q in b}, e, f"posed batch view {k}")
    hb = np.asarray(r.render_batch_host(Vs, Ks, W, H, bg, pose_sets=np.stack([p0, p1]), pose_set=[0, 1]))
    for k, e in enumerate((e0, e1)):
        _check({"rgb8": hb[k]}, e, f"posed host batch view {k}")
    # render_features(mesh_surface=True): rgb is the smooth frame's; features, alpha and depth are those of the same meshes drawn flat
    T = len(case["mesh"]["tris"])
    rng = np.random.default_rng(2)
    r.upload_features(rng.uniform(0, 1, (r.n, 5)).astype(np.float32))
    fm = rng.uniform(0, 1, (T, 5)).astype(np.float32)
    r.upload_mesh_features(fm)
    want = ("rgb", "alpha", "depth", "features")
    sm = mc.to_numpy(r.render_features(V, K, W, H, bg, want=want, mesh_surface=True))
    _check({"rgb": sm["rgb"]}, e0, "render_features(mesh_surface=True)")
    covered = e0["stable"] & (e0["ref"]["winner"] >= 0)
    assert (sm["alpha"][covered] == 1.0).all()
    r.upload_mesh_vertex_attributes(None, None)
    flat = mc.to_numpy(r.render_features(V, K, W, H, bg, want=want, mesh_surface=True))
    mc.same(sm, flat, keys=("alpha", "depth", "features"))
    assert not np.array_equal(sm["rgb"], flat["rgb"])


# ---- the state of the attributes ---------------------------------------------------------------------------------------------------------
def test_attributes_are_set_cleared_and_forgotten(rasterizer):
    r = rasterizer
    case = ms.FIXED_CASES["sphere_small"]()
    m = case["mesh"]
    mc.upload_case(r, case, attributes=False)
    r.set_group_poses(case["poses"][0])
    e = _expect("sphere_small", case)
    assert not r.mesh_vertex_attributes and r.n_mesh_vertices == len(m["verts"])
    flat = _single(r, case)
    assert not mc.compare_stable(flat, mc.expected(case, attributes=False)["frame"], e["stable"])
    # all-zero normals: the flat frame, bit for bit
    r.upload_mesh_vertex_attributes(np.zeros_like(m["normals"]), m["vcols"])
    assert r.mesh_vertex_attributes
    mc.same(_single(r, case), flat)
    # normals alone: a smooth triangle takes its own colour at its three vertices
    r.upload_mesh_vertex_attributes(m["normals"])
    own = dict(case, mesh=dict(m, vcols=None))
    _check(_single(r, case), _expect("sphere_small, own colours", own), "normals without vertex colours")
    # normals and colours; a smooth frame differs from the flat one in rgb / rgb8 only
    r.upload_mesh_vertex_attributes(m["normals"], m["vcols"])
    smooth = _single(r, case)
    _check(smooth, e, "normals and colours")
    mc.same(smooth, flat, keys=("alpha", "depth"))
    assert not np.array_equal(smooth["rgb"], flat["rgb"])
    # a vertex-count mismatch is refused with the library's text, and leaves the attributes in place
    with pytest.raises(RuntimeError, match=r"attributes for \d+ vertices, the meshes have \d+"):
        r.upload_mesh_vertex_attributes(m["normals"][:-1], m["vcols"][:-1])
    with pytest.raises(ValueError):
        r.upload_mesh_vertex_attributes(m["normals"], m["vcols"][:-1])
    assert r.mesh_vertex_attributes
    mc.same(_single(r, case), smooth)
    # clearing restores the flat frame
    r.upload_mesh_vertex_attributes(None, None)
    assert not r.mesh_vertex_attributes
    mc.same(_single(r, case), flat)
    # a new upload_meshes forgets them
    r.upload_mesh_vertex_attributes(m["normals"], m["vcols"])
    r.upload_meshes(m["verts"], m["tris"], m["cols"], groups=m["groups"], ambient=m["ka"], diffuse=m["kd"])
    assert not r.mesh_vertex_attributes
    mc.same(_single(r, case), flat)
    # ... and so does clear_meshes; attributes without meshes are refused
    r.upload_mesh_vertex_attributes(m["normals"], m["vcols"])
    r.clear_meshes()
    assert not r.mesh_vertex_attributes and r.n_mesh_vertices == 0
    with pytest.raises(RuntimeError, match="no meshes"):
        r.upload_mesh_vertex_attributes(m["normals"], m["vcols"])


# ---- the robot's meshes through SplatHandler ---------------------------------------------------------------------------------------------
def test_task_and_robot_meshes_through_handler():
    from sim_a_splat_amd.handler import SplatHandler
    hs = mc.handler_setup()
    h = SplatHandler.from_arrays(*hs["args"], device=0, meshes={"task": None, "robot": ms.robot_links()}, task_assets_path=str(mc.GOLDEN),
                                 task_assets_name="tblock_paper.obj")
    try:
        assert h.scene.row_names()[3:] == ["robot/mesh_task/task", "robot/mesh_robot/link0", "robot/mesh_robot/link1"]
        h.draw_handler(hs["msg"])
        H, W = hs["size"]
        got = h.render(h.scene, [hs["cam"]], [[H, W]])[0]
        rows = h.scene.group_pose_rows()
        want_rows = mc.handler_predicted_rows(hs, robot=True)
        # the poses the CPU caps were settled with are the poses the scene holds; mesh_pose_rows gives the meshes' without the scene
        assert rows.shape == (6, 12) and np.abs(rows - want_rows).max() < 1e-5
        idx, mrows = h.mesh_pose_rows(hs["msg"])
        assert idx.tolist() == [3, 4, 5] and np.array_equal(mrows, rows[3:])
        V, K = h.scene._view_and_K(H, W, hs["cam"][0], hs["cam"][1], h.scene.camera.fov)
        e = _expect("handler", mc.case_handler(hs, rows, V, K, robot=True))
        assert len(np.unique(e["ref"]["winner"][e["stable"] & e["ref"]["smooth_pixel"]])) > 20
        _check({"rgb8": np.asarray(got)}, e, "SplatHandler.render, meshes=('task', 'robot')")
        fl = mc.to_numpy(h.scene.get_render_float(H, W, hs["cam"][0], hs["cam"][1]))
        _check(fl, e, "SplatScene.get_render_float")
        # segmentation names the robot meshes with no further work
        wts = h.scene.get_segmentation(H, W, hs["cam"][0], hs["cam"][1])["weights"].cpu().numpy()
        assert wts.shape == (H, W, 6) and wts[..., 4].max() > 0.0 and wts[..., 5].max() > 0.0
    finally:
        h.scene.close()
