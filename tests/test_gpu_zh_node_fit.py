"""GPU: the node driver (sas_nodes_fit_rigid; Rasterizer.node_fit_rigid, deform.NodeDriver, SplatScene.deform_positions; DESIGN.md 3,
"Deformation") against tests/tools/node_fit_ref.py.  The kernel's float64 rows are held to the np.longdouble restatement within FOUR times the
float64 restatement's own error (the measured ratios are printed, and how many entries differ in bits from the float64 restatement is recorded);
its properties -- rounded once, a proper rotation, the node lands, the least rotation, the identity, poisoned positions, padded tables, time
steps, the same bits twice -- on every case of the kit at kn = 0, 1, 6 and 8; NodeDriver.drive to the skin restatement under the host's fits
within the deform test's four-float32-errors bound; Door B bit for bit."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import node_fit_child as nfc  # noqa: E402
import node_fit_ref as nf  # noqa: E402
import skin_grad_ref as sg  # noqa: E402
import skin_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nf.CASES))
def test_fit_kernel_within_four_yardsticks_and_its_properties(rasterizer, name):
    for kn in nf.KNS:
        nfc.check_case(rasterizer, name, kn)


def test_refusals(rasterizer):
    from sim_a_splat_amd import deform
    r, L = rasterizer, _capi.lib()
    c = nf.case("grid9", 6)
    g, b, nb = nfc._dev(r, c["nodes"]), nfc._dev(r, c["moved"]), nfc._dev(r, c["nb"])
    T64 = torch.zeros((9, 3, 4), dtype=torch.float64, device=r.device)
    T32 = torch.zeros((9, 3, 4), dtype=torch.float32, device=r.device)
    p = lambda t: None if t is None else t.data_ptr()
    call = lambda steps=1, m=9, kn=6, nodes=g, moved=b, table=nb, o64=T64, o32=T32: \
        L.sas_nodes_fit_rigid(r._ctx, steps, m, p(nodes), p(moved), kn, p(table), p(o64), p(o32), None)
    assert call() == 0 and call(o64=None) == 0 and call(kn=0, table=None) == 0
    torch.cuda.synchronize(r.device)
    before = T32.clone()
    for bad in (dict(steps=0), dict(steps=-1), dict(m=0), dict(m=65537), dict(kn=9), dict(kn=-1), dict(nodes=None), dict(moved=None), dict(o32=None),
                dict(table=None), dict(steps=(1 << 30) // 9 + 1)):
        assert call(**bad) == -1, bad
    assert call(kn=9) == -1 and b"kn=9" in L.sas_last_error(r._ctx)
    torch.cuda.synchronize(r.device)
    assert torch.equal(T32, before)   # a refused call changes nothing
    with pytest.raises(ValueError, match="out of"):
        r.node_fit_rigid(torch.zeros((0, 3), device=r.device), torch.zeros((0, 3), device=r.device))
    with pytest.raises(ValueError, match="kn <= 8"):
        r.node_fit_rigid(g, b, torch.zeros((9, 9), dtype=torch.int32, device=r.device))
    with pytest.raises(ValueError, match="moved"):
        r.node_fit_rigid(g, b[:5], nb)
    with pytest.raises(ValueError, match="moved"):
        r.node_fit_rigid(g, b.double(), nb)
    with pytest.raises(ValueError, match="out64"):
        r.node_fit_rigid(g, b, nb, out64=T32)
    with pytest.raises(ValueError, match="neighbours=9"):
        deform.NodeDriver(r, c["nodes"], neighbours=9)
    with pytest.raises(ValueError, match=r"moved must be \[9,3\]"):
        deform.NodeDriver(r, c["nodes"]).drive(np.zeros((2, 9, 3), np.float32))
    single = deform.NodeDriver(r, c["nodes"][:1])   # one node: no neighbours, no table
    assert single.k == 0 and single.table is None
    T = single.fit(c["moved"][:1])["transforms64"].cpu().numpy()
    assert (T[:, :, :3] == np.eye(3)).all()


# ---- NodeDriver -----------------------------------------------------------------------------------------------------------------------------------
def _sheet_moved(c):
    moved = c["nodes"].astype(np.float64)
    moved[:, 2] += 0.15 * np.sin(2.5 * moved[:, 0]) + 0.05 * moved[:, 1]
    moved[:, 0] *= 0.97
    return moved.astype(np.float32)


def test_node_driver_drives_the_skin_as_the_host_fits_do(rasterizer):
    """The skin kit's 300-Gaussian sheet under its 3x3 nodes: read_scene() after drive(moved) against skin_ref.deform_ref under the HOST's
    transforms (transforms_from_positions(table=)) in float64, within the deform test's bound: four times the float32 restatement's error."""
    from sim_a_splat_amd import deform
    r = rasterizer
    c = sg.recovery_case()
    r.upload(**c["upload"])
    r.set_skin(c["indices"], c["weights"])
    opt = deform.NodeOptimizer(r, c["nodes"])
    driver = deform.NodeDriver(r, c["nodes"], graph=opt)
    assert driver.table is opt.table and driver.nodes is opt.nodes and driver.k == 6 and driver.m == 9
    own = deform.NodeDriver(r, c["nodes"])
    assert torch.equal(own.table, opt.table)
    assert deform.NodeDriver(r, None, graph=own).table is own.table
    with pytest.raises(ValueError, match="graph is over"):
        deform.NodeDriver(r, c["nodes"][:5], graph=own)
    res = r.node_fit_rigid(own.nodes, own.nodes, own.table, want64=False)
    assert res["transforms64"] is None and torch.equal(res["transforms"], torch.from_numpy(sr.identity_transforms(9)).to(r.device))
    moved = _sheet_moved(c)
    out = driver.drive(moved)
    assert out is driver.transforms
    got = r.read_scene()
    T_host = driver.transforms.cpu().numpy().copy()
    G = deform.transforms_from_positions(c["nodes"], moved, table=driver.table.cpu().numpy())
    print(f"  drive: the device's float32 transforms differ from the host's by up to {np.abs(T_host - G).max():.2e}")
    r32, r64 = (sr.deform_ref(c["rest"], c["indices"], c["weights"], G, dt) for dt in (np.float32, np.float64))
    for a in r64:
        e32, e = sr.rel_err(r32[a], r64[a]), sr.rel_err(got[a].cpu().numpy(), r64[a])
        print(f"  drive {a}: device {e:.3e}, float32 restatement {e32:.3e}, ratio {e / e32:.2f}")
        assert e <= 4.0 * e32, (a, e, e32)
    assert np.abs(r64["means"] - c["rest"]["means"]).max() > 0.01
    # a device tensor and the same host array: the same bits, in the transforms and in the scene
    means_host = got["means"].clone()
    driver.transforms.zero_()
    assert driver.drive(torch.from_numpy(moved).to(r.device)) is driver.transforms
    assert np.array_equal(driver.transforms.cpu().numpy().view(np.uint32), T_host.view(np.uint32))
    assert torch.equal(r.read_scene()["means"], means_host)
    # fit: the same transforms without a deform, and time steps in one launch
    res = driver.fit(np.stack([moved, c["nodes"]]))
    assert res["transforms"].shape == (2, 9, 3, 4) and res["transforms64"].dtype == torch.float64
    assert np.array_equal(res["transforms"][0].cpu().numpy().view(np.uint32), T_host.view(np.uint32))
    assert torch.equal(res["transforms"][1], torch.from_numpy(sr.identity_transforms(9)).to(r.device))
    # a poisoned row: that node keeps [I | 0], and drive does not refuse it
    bad = moved.copy()
    bad[4, 1] = np.nan
    T = driver.drive(bad).cpu().numpy()
    assert np.array_equal(T[4], sr.identity_transforms(1)[0]) and np.isfinite(T).all()
    r.clear_skin()


def _look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    from sim_a_splat_amd.poses import matrix_to_quat_wxyz
    p = np.asarray(position, np.float64)
    z = np.asarray(target, np.float64) - p
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return tuple(matrix_to_quat_wxyz(np.stack([x, np.cross(z, x), z], axis=1))), tuple(p)


def test_door_b_deforms_its_group_from_positions():
    """A two-group scene: the frame after deform_positions(moved) is the frame after deform(driver.transforms) bit for bit, the other group's
    Gaussians keep their bits, and a new bind_deformable drops the driver."""
    from sim_a_splat_amd.scene import SplatScene
    W, H = 64, 48
    c = sg.recovery_case()
    rng = np.random.default_rng(97)
    n0 = 150
    static = ((rng.normal(0.0, 0.08, (n0, 3)) + (0.0, 0.62, 0.0)).astype(np.float32), np.tile(np.eye(3, dtype=np.float32) * 2e-3, (n0, 1, 1)),
              rng.uniform(0, 1, (n0, 3)).astype(np.float32), rng.uniform(0.5, 0.9, n0).astype(np.float32))
    M = sr.quat_to_matrix(c["rest"]["quats"]) * c["scales"].astype(np.float64)[:, None, :]
    cov = (M @ np.swapaxes(M, 1, 2)).astype(np.float32)
    scene = SplatScene(0, background=(0.0, 0.0, 0.0))
    try:
        scene.add_gaussian_splats("static", *static)
        cloth = scene.add_gaussian_splats("cloth", c["rest"]["means"], cov, c["colors"], c["op"], position=(0.0, -0.05, 0.0))
        with pytest.raises(RuntimeError, match="bind_deformable first"):
            scene.deform_positions(c["nodes"])
        scene.bind_deformable(cloth, c["nodes"], k=4)
        cam = _look_at((0.0, -0.5, 1.4))
        rest_frame = scene.get_render(H, W, *cam, fov=0.9).copy()
        before = {k: v.clone() for k, v in scene._raster.read_scene().items()}
        moved = _sheet_moved(c)
        T = scene.deform_positions(torch.from_numpy(moved).to(scene._raster.device))
        driver = scene._driver
        assert T is driver.transforms and driver.m == 9
        frame = scene.get_render(H, W, *cam, fov=0.9).copy()
        after = {k: v.clone() for k, v in scene._raster.read_scene().items()}
        assert np.abs(frame.astype(int) - rest_frame.astype(int)).max() > 0
        for k in before:   # the static group keeps its bits; the cloth moved
            assert torch.equal(before[k][:n0], after[k][:n0]), k
        assert not torch.equal(before["means"][n0:], after["means"][n0:])
        kept = driver.transforms.clone()
        scene.deform(sr.identity_transforms(9))
        assert np.array_equal(scene.get_render(H, W, *cam, fov=0.9), rest_frame)
        scene.deform(kept)
        assert np.array_equal(scene.get_render(H, W, *cam, fov=0.9), frame)
        # the handle's pose is still applied on top
        cloth.position = (0.0, 0.1, 0.0)
        scene.deform_positions(moved)
        assert scene._driver is driver
        assert not np.array_equal(scene.get_render(H, W, *cam, fov=0.9), frame)
        scene.bind_deformable(cloth, c["nodes"], k=4)
        assert scene._driver is None
    finally:
        scene.close()


# ---- once more under the bounds-checked build -------------------------------------------------------------------------------------------------------
def test_every_case_in_a_child_process_under_the_bounds_checked_build():
    """tests/tools/node_fit_child.py runs every kernel check above in a fresh process under variants/lib_bounds.so, where every index the kernel
    computes is range-checked (codes 1607 to 1609), and reads the counter: no report.  The variant is the one ``build()`` makes
    (sim_a_splat_amd.build.bounds_variant); where it is missing, or was built from other sources by its stamp, it is built here -- once, a
    minute and a half of compiling -- and a build that fails fails the test."""
    from sim_a_splat_amd import build
    lib = build.bounds_variant()
    env = dict(os.environ, SAS_LIB_PATH=str(lib))
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "node_fit_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout[-1500:])
    assert p.returncode == 0 and "node fit child ok (bounds-checked)" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


# ---- last: the bounds-checked build -----------------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    rep = nfc.bounds_report()
    assert rep is None or rep[0] == 0
