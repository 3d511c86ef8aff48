"""GPU: mesh frames against the float64 mesh reference + the depth-limited oracle (oracle/mesh_ref.py, oracle.render(zlim=,
bgmap=)), bit for bit on the pixels the reference calls stable ("Meshes").

The cases (tests/tools/mesh_cases.py) give every pixel of a tile its own depth limit: tilted planes through the cloud, the
T-block among the splats, a triangle soup, ragged sizes with mesh edges in the ragged tiles, a 1920x1080 frame with a few
thousand triangles, every entry point.  Unstable pixels are counted, printed and held to the 10 % cap (a miss fails); the caps
themselves are settled on the CPU (tests/test_mesh_ref_cpu.py).  These run unchanged under the bounds-checked build.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle
from sim_a_splat_amd.rasterizer import Rasterizer

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
OUTS = mc.OUTS


_expect, _single = mc.expect, mc.single


def _check(got, e, what, fill=False):
    diffs = mc.compare(got, e, fill=fill)[0]
    assert not diffs, (what, diffs)


def _run_single_view_case(name, case):
    r = Rasterizer(0)
    try:
        mc.upload_case(r, case)
        e = _expect(name, case)
        _check(_single(r, case), e, name)
        return e
    finally:
        r.close()


# ---- tilted planes through the cloud ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", mc.PLANE_SCENES)
def test_tilted_plane_through_the_cloud(scene):
    e = _run_single_view_case(f"plane_{scene}", mc.case_plane(scene))
    if scene == "dense":     # the carrier of the 256-entry batch logic: pixels of one long tile stop inside the first batch and after it
        assert e["tiles_cut_in_both_batches"] >= 1 and e["longest_list"] > 512


# ---- the T-block in the scene --------------------------------------------------------------------------------------------------
def test_tblock_inside_the_cloud():
    case = mc.case_tblock()
    V, K, W, H = case["cams"][0]
    sets = np.stack(case["poses"]).astype(np.float32)
    r = Rasterizer(0)
    try:
        mc.upload_case(r, case)
        es = [_expect("tblock", case, v) for v in range(2)]
        assert not np.array_equal(es[0]["ref"]["winner"], es[1]["ref"]["winner"])
        for v in range(2):
            r.set_group_poses(sets[v])
            _check(_single(r, case, v), es[v], f"render, pose {v}")
        Vs, Ks = np.stack([V, V, V]), np.stack([K, K, K])
        order = [1, 0, 1]
        b = mc.to_numpy(r.render_batch(Vs, Ks, W, H, case["bg"], want=OUTS, pose_sets=sets, pose_set=order))
        for k, s in enumerate(order):
            _check({q: b[q][k] for q in b}, es[s], f"render_batch view {k} pose set {s}")
        hb = np.asarray(r.render_batch_host(Vs, Ks, W, H, case["bg"], pose_sets=sets, pose_set=order))
        for k, s in enumerate(order):
            _check({"rgb8": hb[k]}, es[s], f"render_batch_host view {k} pose set {s}")
    finally:
        r.close()


def test_tblock_through_handler():
    from sim_a_splat_amd.handler import SplatHandler
    hs = mc.handler_setup()
    h = SplatHandler.from_arrays(*hs["args"], device=0, meshes=("task",), task_assets_path=str(mc.GOLDEN), task_assets_name="tblock_paper.obj")
    try:
        h.draw_handler(hs["msg"])
        H, W = hs["size"]
        got = h.render(h.scene, [hs["cam"]], [[H, W]])[0]
        rows = h.scene.group_pose_rows()
        # the poses the CPU caps were settled with are the poses the scene holds
        assert rows.shape == (4, 12) and np.abs(rows - mc.handler_predicted_rows(hs)).max() < 1e-5
        V, K = h.scene._view_and_K(H, W, hs["cam"][0], hs["cam"][1], h.scene.camera.fov)
        case = mc.case_handler(hs, rows, V, K)
        e = _expect("handler", case)
        _check({"rgb8": np.asarray(got)}, e, "SplatHandler.render")
    finally:
        h.scene.close()


# ---- triangle soup, sizes --------------------------------------------------------------------------------------------------------
def test_triangle_soup_over_a_scene():
    e = _run_single_view_case("soup", mc.case_soup())
    assert len(np.unique(e["ref"]["winner"][e["stable"]])) > 10


@pytest.mark.parametrize("size", [(250, 187), (17, 33)])
def test_ragged_sizes(size):
    _run_single_view_case(f"size_{size[0]}x{size[1]}", mc.case_size(*size))


def test_full_hd_thousands_of_triangles():
    _run_single_view_case("full_hd", mc.case_1080p())


# ---- entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points():
    case = mc.case_entry_points()
    p0, p1 = case["poses"]
    same_pose = dict(case, poses=[p0, p0])
    (V0, K0, W, H), (V1, K1, _, _) = case["cams"]
    Vs, Ks = np.stack([V0, V1]), np.stack([K0, K1])
    bg = case["bg"]
    r = Rasterizer(0)
    try:
        mc.upload_case(r, case)
        r.set_group_poses(p0)
        e00, e10, e11 = _expect("entry_points", same_pose, 0), _expect("entry_points", same_pose, 1), _expect("entry_points", case, 1)
        assert not np.array_equal(e10["frame"]["rgb8"], e11["frame"]["rgb8"])
        _check(_single(r, case), e00, "single")
        _check(_single(r, case, depth_fill_max=True), e00, "single, depth fill", fill=True)
        b = mc.to_numpy(r.render_batch(Vs, Ks, W, H, bg, want=OUTS))
        for k, e in enumerate((e00, e10)):
            _check({q: b[q][k] for q in b}, e, f"batch view {k}")
        b = mc.to_numpy(r.render_batch(Vs, Ks, W, H, bg, want=OUTS, pose_sets=np.stack([p0, p1]), pose_set=[0, 1]))
        for k, e in enumerate((e00, e11)):
            _check({q: b[q][k] for q in b}, e, f"posed batch view {k}")
        hb = np.asarray(r.render_batch_host(Vs, Ks, W, H, bg))
        for k, e in enumerate((e00, e10)):
            _check({"rgb8": hb[k]}, e, f"host batch view {k}")
        # RGB-D: points and mask are the oracle's unprojection of the depth image
        ed, a = e00["frame"]["depth"][..., 0], e00["frame"]["alpha"][..., 0]
        md = float(np.quantile(ed[a > 0], 0.6))
        for fill in (False, True):
            g = mc.to_numpy(r.render_rgbd(V0, K0, W, H, bg, max_depth=md, depth_fill_max=fill))
            _check({k: g[k] for k in ("rgb", "alpha", "depth")}, e00, f"rgbd fill={fill}", fill=fill)
            pts, mask = oracle.unproject(g["depth"], K0, md)          # the consumer's arithmetic on the delivered depth ...
            assert np.array_equal(g["points"].view(np.uint8), pts.view(np.uint8)) and np.array_equal(g["mask"], mask)
            want = np.where(a > 0, ed, ed.max()) if fill else ed      # ... and on the reference's, where it is comparable
            where = e00["stable"] & ((a > 0) | bool(not fill or e00["stable"][ed == ed.max()].all()))
            pts, mask = oracle.unproject(want.astype(np.float32), K0, md)
            assert np.array_equal(g["points"][where].view(np.uint8), pts[where].view(np.uint8)) and np.array_equal(g["mask"][where], mask[where])
            assert mask[where].any() and not mask[where].all()
        # a non-blocking frame keeps the pose it was submitted with
        out = r.render(V0, K0, W, H, bg, want=OUTS, block=False)
        r.set_group_poses(p1)
        other = r.render(V1, K1, W, H, bg, want=OUTS, block=False)
        r.wait()
        torch.cuda.synchronize()
        _check(mc.to_numpy(out), e00, "non-blocking frame")
        _check(mc.to_numpy(other), e11, "non-blocking frame, next pose")
    finally:
        r.close()
