"""GPU: point matching (sas_match_points / Rasterizer.match_points; DESIGN.md 3, "Point matching") and the registration around it
(sim_a_splat_amd/register.py) against tests/tools/match_ref.py, which tests/test_register_cpu.py holds to its float64 form.

``index`` and ``dist2`` are BIT-EQUAL to ``match32``, the contract restated in NumPy float32.  The 18 moments are float64 sums whose
order is the kernel's own: each is within ``n eps64 sum |term|`` of ``moments64`` (match_ref.moment_bound: the bound of a sum of n
terms in any order).  No output depends on the slice count, and two calls return the same bytes.  The free registration loop is
held to the float64 loop within 4 e32 + 8 eps32 L, e32 = what float32 matching costs the NumPy loop on the same case (the formula of
the mesh-query tests).  Every check prints what it measured.  Every test fails without the feature: the entry point, the method and
the module do not exist.  The file runs unchanged under the bounds-checked build, and its last test reads that build's counter.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

from sim_a_splat_amd import _capi, register, segment
from sim_a_splat_amd.rasterizer import MATCH_CHUNK, Rasterizer

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import match_cases as mc  # noqa: E402
import match_ref as mr  # noqa: E402
import mesh_query_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def rz():
    r = Rasterizer(0)
    yield r
    r.close()


def _gpu(rz, source, target, transform=None, max_distance=INF, slices=None):
    res = rz.match_points(source, target, transform, max_distance, slices)
    return res["index"].cpu().numpy(), res["dist2"].cpu().numpy(), res["moments"]


def _check(what, got, want, target):
    """index and dist2 bit-equal to ``want`` (match32's result), the moments within the any-order bound of moments64."""
    index, dist2, moments = got
    assert index.dtype == np.int32 and dist2.dtype == np.float32 and moments.dtype == np.float64 and moments.shape == (18,)
    assert not np.isnan(dist2).any() and np.isfinite(moments).all()
    assert (index == want["index"]).all(), (what, "index", int((index != want["index"]).sum()))
    assert dist2.tobytes() == want["dist2"].tobytes(), (what, "dist2")
    assert (np.isinf(dist2) == (index < 0)).all()
    bound = mr.moment_bound(want["moved"], target, want["dist2"], want["index"])
    err = np.abs(moments - want["moments"])
    worst = int(np.argmax(err - bound))
    print(f"  {what}: {len(index)} source points, {int((index >= 0).sum())} held; moments |gpu - ref| max {err.max():.3e}, "
          f"closest to its bound: moment {worst}, {err[worst]:.3e} of {bound[worst]:.3e}")
    assert moments[0] == (index >= 0).sum()
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


# ---- 1: wave and workgroup edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_source_counts(rz, n):
    src, tgt = mc.drawn(257, 300, seed=41)
    src = src[:n]
    for md in (INF, 0.4):
        _check(f"n={n} md={md}", _gpu(rz, src, tgt, None, md), mr.match32(src, tgt, None, md), tgt)
    held = mr.match32(src, tgt, None, 0.4)["index"] >= 0
    assert n < 63 or 0 < held.sum() < n          # the threshold both holds and drops


# ---- 2: chunk and slice edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_target", [1, MATCH_CHUNK - 1, MATCH_CHUNK, MATCH_CHUNK + 1, 2 * MATCH_CHUNK + 1])
def test_chunk_and_slice_edges(rz, n_target):
    src, tgt = mc.drawn(300, 2 * MATCH_CHUNK + 1, seed=43)
    tgt = tgt[:n_target]
    T = mc.similarity(1.1, (0.2, 0.9, -0.4), 25.0, (0.05, -0.1, 0.02))
    want = mr.match32(src, tgt, T, 0.5)
    first = None
    for slices in (0, 1, 2, 3, 1000):            # (1000 is clamped to the number of chunks)
        got = _gpu(rz, src, tgt, T, 0.5, slices)
        _check(f"T={n_target} slices={slices}", got, want, tgt)
        blob = got[0].tobytes() + got[1].tobytes() + got[2].tobytes()
        first = first or blob
        assert blob == first, (n_target, slices)


# ---- 3: ties and the threshold -------------------------------------------------------------------------------------------------------------
def test_ties_and_threshold(rz):
    # duplicated targets and targets symmetric about the source: the lowest index, within a chunk and across chunks and slices
    tgt = np.full((2 * MATCH_CHUNK + 44, 3), 50.0, np.float32)
    tgt[5] = tgt[300] = tgt[2 * MATCH_CHUNK + 40] = (1, 0, 0)
    tgt[7] = (-1, 0, 0)
    tgt[260] = (0, 1, 0)
    tgt[20] = tgt[21] = (8, 8, 9)
    tgt[600 - 256] = (8, 8, 7)
    src = np.array([[0, 0, 0], [8, 8, 8]], np.float32)
    for slices in (None, 1, 2, 3):
        index, dist2, m = _gpu(rz, src, tgt, None, INF, slices)
        assert index.tolist() == [5, 20] and dist2.tolist() == [1.0, 1.0] and m[0] == 2, slices
    _check("ties", _gpu(rz, src, tgt), mr.match32(src, tgt), tgt)
    # d2 == md2 holds the match; the next float above does not
    up = np.nextafter(np.float32(3), np.float32(4))
    src = np.array([[0, 0, 0], [0, 64, 0]], np.float32)
    tgt = np.array([[3, 0, 0], [up, 64, 0]], np.float32)
    index, dist2, m = _gpu(rz, src, tgt, None, 3.0)
    print(f"  threshold: index {index.tolist()}, dist2 {dist2.tolist()}, moments n {m[0]}, sum q {m[4:7].tolist()}, sum d2 {m[17]}")
    assert index.tolist() == [0, -1] and dist2[0] == 9.0 and dist2[1] == np.inf
    assert m[0] == 1 and m[4:7].tolist() == [3.0, 0.0, 0.0] and m[1:4].tolist() == [0.0, 0.0, 0.0] and m[17] == 9.0 and m[16] == 0.0
    index, dist2, m = _gpu(rz, src, tgt, None, float(up))
    assert index.tolist() == [0, 1] and m[0] == 2
    _check("threshold", _gpu(rz, src, tgt, None, 3.0), mr.match32(src, tgt, None, 3.0), tgt)


# ---- 4: defined inputs -----------------------------------------------------------------------------------------------------------------------
def test_defined_inputs(rz):
    src, tgt = mc.drawn(70, 300, seed=47)
    src, tgt = src.copy(), tgt.copy()
    src[3] = (np.nan, 0, 0)
    src[4] = (0, np.inf, 0)
    src[5] = (0, 0, -np.inf)
    src[6] = (1e30, 0, 0)
    src[7] = (1e30, 1e30, 1e30)
    tgt[0] = (np.nan, 0, 0)
    tgt[1] = (0, np.inf, 0)
    tgt[2] = (np.nan, np.nan, np.nan)
    tgt[299] = (1e30, 1e30, 1e30)
    tgt[MATCH_CHUNK] = (-np.inf, 0, 0)
    for md in (INF, 1.0):
        got = _gpu(rz, src, tgt, None, md)
        _check(f"defined inputs md={md}", got, mr.match32(src, tgt, None, md), tgt)
        index, dist2, m = got
        assert (index[3:6] == -1).all() and index[6] == -1 and index[7] == 299 and dist2[7] == 0.0
        assert not np.isin(index, [0, 1, 2, MATCH_CHUNK]).any()
    # no target: every index -1, n = 0
    index, dist2, m = _gpu(rz, src, tgt[:0])
    assert (index == -1).all() and np.isinf(dist2).all() and (m == 0).all()
    # no source
    res = rz.match_points(src[:0], tgt)
    assert res["index"].shape == (0,) and res["dist2"].shape == (0,) and (res["moments"] == 0).all()
    # transform=None is the identity, bit for bit; a 3x4 is the 4x4's upper rows; device tensors are read where they are
    import torch
    a = _gpu(rz, src, tgt, None, 1.0)
    b = _gpu(rz, src, tgt, np.eye(4), 1.0)
    c = _gpu(rz, torch.from_numpy(src).to(rz.device), torch.from_numpy(tgt).to(rz.device), np.eye(4)[:3], 1.0)
    for other in (b, c):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, other))


# ---- 5: a similarity transform ---------------------------------------------------------------------------------------------------------------
def test_similarity_transform(rz):
    src, tgt = mc.drawn(700, 700, seed=1400)
    a = _gpu(rz, src, tgt, mc.TRUTH, 0.5)
    _check("similarity 700x700", a, mr.match32(src, tgt, mc.TRUTH, 0.5), tgt)
    b = _gpu(rz, src, tgt, mc.TRUTH, 0.5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert 0 < (a[0] >= 0).sum() < 700
    # a point's result does not depend on the other points of the call
    part = _gpu(rz, src[100:431], tgt, mc.TRUTH, 0.5)
    assert part[0].tobytes() == a[0][100:431].tobytes() and part[1].tobytes() == a[1][100:431].tobytes()


# ---- 6: the registration loop ------------------------------------------------------------------------------------------------------------
def test_lock_step_and_free_loop(rz):
    c = mc.noisy_case()
    l32, l64, e32 = mc.loops("noisy")
    # lock step: the reference loop's transform of every iteration
    for k, (T, want) in enumerate(zip(l32["transforms"], l32["matches"])):
        _check(f"lock step {k}", _gpu(rz, c["source"], c["target"], T, mc.THRESHOLD), want, c["target"])
    # the free loop
    res = register.register_similarity(c["source"], c["target"], c["init"], rasterizer=rz)
    tol = 4 * e32 + 8 * mc.EPS32 * c["L"]
    err = float(np.abs(res.transformation - l64["T"]).max())
    print(f"  free loop, noisy case: {res.iterations} iterations (float64 loop {l64['iterations']}), |T - T64| max {err:.3e} "
          f"(tol {tol:.3e}, e32 {e32:.3e}), fitness {res.fitness:.4f}, rmse {res.inlier_rmse:.4e}")
    assert err <= tol
    assert len(res.history) == res.iterations + 1


def test_free_loop_clean_case(rz):
    c = mc.clean_case()
    res = register.register_similarity(c["source"], c["target"], c["init"], rasterizer=rz)
    esr = float(np.abs(res.transformation[:3, :3] - mc.TRUTH[:3, :3]).max())
    et = float(np.abs(res.transformation[:3, 3] - mc.TRUTH[:3, 3]).max())
    print(f"  free loop, clean case: {res.iterations} iterations, |sR - sR_true| max {esr:.3e}, |t - t_true| {et:.3e} (L {c['L']:.3f}), "
          f"fitness {res.fitness:.4f}, rmse {res.inlier_rmse:.3e}")
    assert res.iterations < 30 and esr <= 1e-5 and et <= 1e-5 * c["L"] and res.fitness == 1.0


# ---- 7: end to end -----------------------------------------------------------------------------------------------------------------------------
def test_register_then_segment_end_to_end(rz):
    from sim_a_splat_amd.handler import SplatHandler
    c = mc.scene_case()
    means, meshes = c["means"], c["meshes"]
    ref = register.register_similarity(c["source"], means, c["init"], matcher=mr.match64)          # the float64 reference
    res = register.register_similarity(c["source"], means, c["init"], rasterizer=rz)
    T_ref, T_gpu = ref.transformation, res.transformation
    delta = float(np.abs(mc.apply(T_gpu, c["vertices"]) - mc.apply(T_ref, c["vertices"])).max())
    print(f"  end to end: {res.iterations} iterations (reference {ref.iterations}), fitness {res.fitness:.4f}, rmse {res.inlier_rmse:.4e}, "
          f"|T_gpu - T_ref| max {np.abs(T_gpu - T_ref).max():.3e}, delta {delta:.3e}, |T_ref - shipped| max {np.abs(T_ref - c['truth']).max():.3e}")
    masks = segment.link_masks_from_meshes(means, meshes, [T_gpu @ S for S in c["local"]], distance=0.015, rasterizer=rz)
    assert list(masks) == ["link0", "link1"]
    placed = [qc.moved(m, T_ref @ S) for m, S in zip(meshes, c["local"])]
    r64, r32 = qc.reference("register_e2e", means, placed, 0.015)
    for k, (tol_d, tol_w, _, _) in enumerate(qc.tolerances(means, placed, r64, r32)):
        want = (r64["winding"][k] > 0.5) | (r64["distance"][k] < 0.015)
        undecidable = (np.abs(r64["distance"][k] - 0.015) <= tol_d + delta) | (np.abs(r64["winding"][k] - 0.5) <= tol_w)
        got = masks[f"link{k}"]
        print(f"  end to end link{k}: mask {int(got.sum())} (reference {int(want.sum())}), flipped {int((got != want).sum())}, "
              f"undecidable {int(undecidable.sum())} (tol_d {tol_d:.3e}, tol_w {tol_w:.3e})")
        assert not ((got != want) & ~undecidable).any()
        assert undecidable.sum() <= 0.01 * len(means)
        assert 1000 < got.sum() <= 1500 + 50
    # the result builds a handler, and both links show in a label image
    n = len(means)
    rng = np.random.default_rng(32)
    covs = np.tile(np.eye(3, dtype=np.float32) * 1e-4, (n, 1, 1))
    colors = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
    h = SplatHandler.from_arrays(means, covs, colors, np.full(n, 0.9, np.float32), masks, T_gpu, [np.eye(4)] * 2, device=0)
    try:
        c0, c1 = c["centres"]
        cam = (np.array([1.0, 0.0, 0.0, 0.0]), 0.5 * (c0 + c1) + np.array([0.0, 0.0, -0.6]))     # looks along +z at both links
        labels, = h.render_segmentation(h.scene, [cam], [[120, 160]])
        names = h.scene.row_names()
        seen = {names[r] for r in np.unique(labels) if r != 255}
        print(f"  end to end labels: {sorted(seen)}")
        assert labels.shape == (120, 160) and {"robot/splat_robot/link0", "robot/splat_robot/link1"} <= seen
    finally:
        h.scene.close()


def test_command_line_writes_the_whole_masks_directory(rz, tmp_path, golden_dir, capsys):
    """python -m sim_a_splat_amd.register --masks: registration and segmentation in one command, and the directory loads."""
    from sim_a_splat_amd import io, poses
    (tmp_path / "meshes").mkdir()
    (tmp_path / "meshes" / "base.stl").write_bytes((golden_dir / "xarm6_base.stl").read_bytes())
    (tmp_path / "meshes" / "t.obj").write_bytes((golden_dir / "tblock_paper.obj").read_bytes())
    urdf = tmp_path / "r.urdf"
    urdf.write_text("""<robot name="r">
  <link name="base"><visual><geometry><mesh filename="package://pkg/meshes/base.stl"/></geometry></visual></link>
  <link name="arm"><visual><origin xyz="0 0 0.1"/><geometry><mesh filename="package://pkg/meshes/t.obj"/></geometry></visual></link>
  <joint name="j" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 0.2"/><axis xyz="0 0 1"/></joint>
</robot>""")
    truth = mc.similarity(0.93, (0.0, 0.0, 1.0), 4.0, (0.4, 0.3, -0.05))
    rng = np.random.default_rng(8)
    on = mc.apply(truth, register.robot_surface_points(urdf, [0.5], str(tmp_path), "pkg", n_points=900, seed=2)) + rng.normal(0, 0.001, (900, 3))
    splat = np.concatenate([on, rng.uniform(-3, -2, (200, 3))]).astype(np.float32)
    np.save(tmp_path / "means.npy", splat)
    lo, hi = splat[:900, :2].min(0) - 0.02, splat[:900, :2].max(0) + 0.02
    np.save(tmp_path / "poly.npy", np.array([[lo[0], lo[1], 0], [hi[0], lo[1], 0], [hi[0], hi[1], 0], [lo[0], hi[1], 0]]))
    out = tmp_path / "masks" / "r"
    rc = register.main(["--splat", str(tmp_path / "means.npy"), "--urdf", str(urdf), "--joint-config", "0.5", "--robot-description-dir",
                        str(tmp_path), "--package-name", "pkg", "--polygon", str(tmp_path / "poly.npy"), "--axis-min", "-1", "--axis-max",
                        "1", "--points", "600", "--seed", "1", "--scale", "0.95", "--out", str(out), "--masks"])
    text = capsys.readouterr().out
    print(text)
    assert rc == 0 and "link1:" in text and "fitness" in text
    T = io.load_icp_transformation(out / "icp_transformation.npy")
    s, _, _ = poses.decompose_icp(T)
    # the same inputs through the NumPy matcher (tests/test_register_cpu.py::test_command_line_round_trip holds that one to the truth)
    want, init = register.register_robot(splat, urdf, [0.5], str(tmp_path), "pkg", polygon=np.load(tmp_path / "poly.npy"), axis_min=-1,
                                         axis_max=1, scale=0.95, n_points=600, seed=1, matcher=mr.match64)
    tol = 4 * float(np.abs(register.register_robot(splat, urdf, [0.5], str(tmp_path), "pkg", polygon=np.load(tmp_path / "poly.npy"), axis_min=-1,
                                                   axis_max=1, scale=0.95, n_points=600, seed=1, matcher=mr.match32)[0].transformation
                           - want.transformation).max()) + 8 * mc.EPS32 * mc.coordinate_scale(splat[:900])
    err = float(np.abs(T - want.transformation).max())
    print(f"  command line: scale {s:.5f}, |T - T64| max {err:.3e} (tol {tol:.3e})")
    assert err <= tol and (np.load(out / "trans_init.npy") == init).all()
    masks = io.load_link_masks(out / "link_masks_global_dict.npz")
    assert list(masks) == ["link0", "link1"] and all(m.shape == (1100,) for m in masks.values())
    assert masks["link0"][:900].sum() > 300 and masks["link1"][:900].sum() > 50 and not masks["link0"][900:].any() and not masks["link1"][900:].any()
    assert (io.load_joint_config(out / "joint_config.npy") == [0.5]).all() and (out / "polygon_bounds.npy").exists()


# ---- 8: errors -------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(rz):
    import torch
    L = _capi.lib()
    src = np.zeros((4, 3), np.float32)
    tgt = np.ones((5, 3), np.float32)
    index = torch.full((4,), 7, dtype=torch.int32, device=rz.device)
    eye = np.ascontiguousarray(np.eye(4, dtype=np.float32)[:3]).reshape(12)
    moments = np.zeros(18)
    S, T, I, M, E = src.ctypes.data, tgt.ctypes.data, index.data_ptr(), moments.ctypes.data, eye.ctypes.data

    def call(ns=4, s=S, nt=5, t=T, tr=E, md=1.0, slices=0, idx=I, d2=None, mom=M):
        if isinstance(tr, np.ndarray):
            tr = tr.ctypes.data
        rc = L.sas_match_points(rz._ctx, ns, s, nt, t, tr, ctypes.c_float(md), slices, idx, d2, mom, None)
        return rc, L.sas_last_error(rz._ctx).decode()

    assert call()[0] == 0 and moments[0] == 0 and (index.cpu().numpy() == -1).all()      # (sqrt(3) > 1: nothing matches)
    assert call(md=2.0)[0] == 0 and moments[0] == 4 and (index.cpu().numpy() == 0).all()
    bad_nan, bad_inf = eye.copy(), eye.copy()
    bad_nan[5], bad_inf[3] = np.nan, np.inf
    for what, kw in {"negative n_source": dict(ns=-1), "negative n_target": dict(nt=-1), "n_source beyond 2^31 - 256": dict(ns=2 ** 31 - 255),
                     "n_target beyond 2^31 - 256": dict(nt=2 ** 31 - 255), "no source": dict(s=None), "no target": dict(t=None),
                     "max_distance -1": dict(md=-1.0), "max_distance NaN": dict(md=float("nan")), "NaN transform": dict(tr=bad_nan),
                     "Inf transform": dict(tr=bad_inf), "slices -1": dict(slices=-1), "all outputs NULL": dict(idx=None, mom=None)}.items():
        rc, msg = call(**kw)
        print(f"  {what}: status {rc}, {msg!r}")
        assert rc == -1 and msg, what
    assert call(ns=0)[0] == 0 and call(nt=0, t=None)[0] == 0 and call(tr=None, md=2.0)[0] == 0
    with pytest.raises(_capi.SasError):
        rz.match_points(src, tgt, None, -1.0)
    with pytest.raises(ValueError):
        rz.match_points(src, tgt, np.eye(3))
    # the context still answers
    index, dist2, m = _gpu(rz, np.array([[0.0, 0, 0]]), np.array([[0.0, 3, 4], [0, 0, 6]]))
    assert index.tolist() == [0] and dist2.tolist() == [25.0] and m[0] == 1


# ---- last: the bounds-checked build ------------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rz):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
