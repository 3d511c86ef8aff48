"""GPU: point-to-mesh queries (sas_query_meshes / Rasterizer.query_meshes; DESIGN.md 3, "Mesh queries") against the float64 NumPy
reference of tests/tools/mesh_query_ref.py, which tests/test_segment_cpu.py holds to closed forms.

Tolerances are computed per case, per mesh (mesh_query_cases.tolerances): e32 = the largest float32-against-float64 difference of
the NumPy reference on the case, tol_d = 4 e32_d + 8 eps32 L (L the largest absolute coordinate), tol_w = 4 e32_w + eps32 (T + 8)
(T triangles).  The GPU is within tol of the float64 reference on every pair that is not culled; culled pairs read exactly +inf / 0
and are the box rule's; a mask decision may differ from the reference's only where |d64 - threshold| <= tol_d or |w64 - 0.5| <=
tol_w, and such undecidable pairs are at most 1 % of a case.  Every check prints what it measured.  Every test fails without the
feature: the entry point, the method and the module do not exist.  The file runs unchanged under the bounds-checked build.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

from sim_a_splat_amd import _capi, mesh_io, segment
from sim_a_splat_amd.rasterizer import MESH_QUERY_CHUNK, Rasterizer

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_query_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def rz():
    r = Rasterizer(0)
    yield r
    r.close()


def _query(rz, points, meshes, max_distance=INF):
    res = rz.query_meshes(points, meshes, max_distance)
    return res["distance"].cpu().numpy(), res["winding"].cpu().numpy()


def _check(what, got, key, points, meshes, max_distance=INF, threshold=None):
    """The rules of the module docstring for one call; returns the per-mesh masks (GPU) when ``threshold`` is given."""
    d, w = got
    r64, r32 = qc.reference(key, points, meshes, max_distance)
    tols = qc.tolerances(points, meshes, r64, r32)
    assert d.shape == w.shape == r64["distance"].shape
    assert not np.isnan(d).any() and np.isfinite(w).all()
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    masks = []
    for m, ((v, f), (tol_d, tol_w, e_d, e_w)) in enumerate(zip(meshes, tols)):
        culled = r64["culled"][m]
        live = ~culled
        # which pairs are culled: the box rule, asserted on the points further than tol_d from the inflated box's faces
        gpu_culled = np.isinf(d[m])
        if live.any() and np.isfinite(max_distance):
            used = np.asarray(v, np.float32)[qc.ref.kept_faces(v, f).reshape(-1)]
            faces = np.concatenate([used.min(0) - np.float32(max_distance), used.max(0) + np.float32(max_distance)])
            clear = (np.abs(np.concatenate([p32, p32], axis=1) - faces) > tol_d).all(axis=1)
        else:
            clear = np.ones(len(p32), bool)
        assert (gpu_culled[clear] == culled[clear]).all(), (what, m, "culled set")
        assert (gpu_culled == culled).all(), (what, m, "culled set at the box's faces")   # (the same float32 comparison on both sides)
        assert (w[m][gpu_culled] == 0).all() and (d[m][gpu_culled] == np.inf).all(), (what, m)
        err_d = float(np.abs(d[m][live] - r64["distance"][m][live]).max()) if live.any() else 0.0
        err_w = float(np.abs(w[m][live] - r64["winding"][m][live]).max()) if live.any() else 0.0
        line = (f"  {what} mesh {m}: {len(f)} triangles, {int(live.sum())} of {len(p32)} pairs evaluated, |d - d64| max {err_d:.3e} "
                f"(tol {tol_d:.3e}, e32 {e_d:.3e}), |w - w64| max {err_w:.3e} (tol {tol_w:.3e}, e32 {e_w:.3e})")
        if threshold is not None:
            want = (r64["winding"][m] > 0.5) | (r64["distance"][m] < threshold)
            mask = (w[m] > 0.5) | (d[m] < threshold)
            undecidable = (np.abs(r64["distance"][m] - threshold) <= tol_d) | (np.abs(r64["winding"][m] - 0.5) <= tol_w)
            line += (f"; inside {int((r64['winding'][m] > 0.5).sum())}, within {int((r64['distance'][m] < threshold).sum())}, "
                     f"mask {int(want.sum())}, flipped {int((mask != want).sum())}, undecidable {int(undecidable.sum())}")
            masks.append(mask)
        print(line)
        assert err_d <= tol_d, (what, m, err_d, tol_d)
        assert err_w <= tol_w, (what, m, err_w, tol_w)
        if threshold is not None:
            assert not ((mask != want) & ~undecidable).any(), (what, m)
            assert undecidable.sum() <= 0.01 * len(p32), (what, m, int(undecidable.sum()))
    return masks


# ---- 1: wave and workgroup edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_box_point_counts(rz, n):
    mesh = qc.box_mesh()
    pts = qc.box_points(257)[:n]
    got = _query(rz, pts, [mesh])
    _check(f"box n={n}", got, ("box", n), pts, [mesh])
    assert np.isfinite(got[0]).all()
    inside = (np.abs(pts) < [0.5, 0.3, 0.2]).all(axis=1)
    assert ((got[1][0] > 0.5) == inside).all()


# ---- 2: one triangle, and the inputs outside the range ---------------------------------------------------------------------------------
def test_triangle_regions_and_defined_inputs(rz):
    pts = np.array([q for q, _ in qc.SEVEN_REGIONS.values()])
    want = np.array([x for _, x in qc.SEVEN_REGIONS.values()])
    d, w = _query(rz, pts, [qc.TRIANGLE])
    _check("seven regions", (d, w), "seven", pts, [qc.TRIANGLE])
    print(f"  seven regions: |d - closed form| max {np.abs(d[0] - want).max():.3e}")
    assert np.abs(d[0] - want).max() <= 8 * qc.EPS32 * 1.375
    # the zero-area triangle: its edges as segments, no solid angle
    d, w = _query(rz, qc.ZERO_AREA_POINTS, [qc.ZERO_AREA])
    assert np.abs(d[0] - qc.ZERO_AREA_DISTANCE).max() <= 8 * qc.EPS32 * 3.0 and (w == 0).all()
    # a triangle with a NaN vertex beside a good one is dropped; a NaN point reads +inf / 0
    bad = qc.nan_vertex_mesh()
    mixed = np.concatenate([pts, [[np.nan, 0.0, 0.0], [0.1, np.inf, 0.0]]])
    d, w = _query(rz, mixed, [bad, qc.TRIANGLE])
    assert (d[0] == d[1]).all() and (w[0] == w[1]).all()
    assert np.isfinite(d[0][:7]).all() and (d[0][7:] == np.inf).all() and (w[0][7:] == 0).all() and np.isfinite(w).all()
    _check("nan vertex", (d, w), "nanvertex", mixed, [bad, qc.TRIANGLE])
    only_bad = (bad[0], bad[1][:1])
    d, w = _query(rz, pts, [only_bad])
    assert (d == np.inf).all() and (w == 0).all()


# ---- 3: the LDS chunk's edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_chunk_edges(rz, delta):
    v, f = qc.base_mesh()
    mesh = (v, f[:MESH_QUERY_CHUNK + delta])
    pts = qc.raw_base_points()[0][::6][:300]
    assert len(pts) == 300 and len(mesh[1]) == MESH_QUERY_CHUNK + delta
    _check(f"chunk{delta:+d}", _query(rz, pts, [mesh]), ("chunk", delta), pts, [mesh])


# ---- 4, 5, 7: the robot's base -------------------------------------------------------------------------------------------------------------
def test_robot_base_raw_stl(rz):
    mesh = mesh_io.load_stl(qc.GOLDEN / "xarm6_base.stl")
    pts, extent = qc.raw_base_points()
    mask, = _check("raw STL", _query(rz, pts, [mesh]), "raw", pts, [mesh], threshold=0.1 * extent)
    r64, _ = qc.reference("raw", pts, [mesh])
    assert int((r64["winding"] > 0.5).sum()) == 461 and int((r64["distance"] < 0.1 * extent).sum()) == 884


def test_robot_base_similarity_and_culling(rz):
    mesh, pts = qc.similarity_points()
    got = _query(rz, pts, [mesh], 0.015)
    mask, = _check("similarity 0.015", got, "sim", pts, [mesh], 0.015, threshold=0.015)
    r64, _ = qc.reference("sim", pts, [mesh], 0.015)
    assert int((r64["winding"] > 0.5).sum()) == 59 and int((r64["distance"] < 0.015).sum()) == 241 and int(mask.sum()) == 246
    assert 0 < int(np.isinf(got[0]).sum()) < len(pts)
    # culling never changes a decision: the same masks without it, and the same distance bits wherever both are finite
    full = _query(rz, pts, [mesh], INF)
    mask_inf, = _check("similarity inf", full, "sim_inf", pts, [mesh], INF, threshold=0.015)
    assert (mask_inf == mask).all()
    both = np.isfinite(got[0]) & np.isfinite(full[0])
    assert both.sum() > 100 and (got[0][both] == full[0][both]).all() and (got[1][both] == full[1][both]).all()
    assert np.isfinite(full[0]).all()


# ---- 6: several meshes in one call ---------------------------------------------------------------------------------------------------------
def test_several_meshes_rows_are_single_mesh_calls(rz):
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    meshes = [qc.tblock_mesh(), empty, qc.base_mesh(), qc.box_mesh((0.05, 0.04, 0.03), (0.1, 0.1, 0.1))]
    rng = np.random.default_rng(21)
    pts = rng.uniform(-0.25, 0.25, (700, 3))
    for md in (0.05, INF):
        d, w = _query(rz, pts, meshes, md)
        d2, w2 = _query(rz, pts, meshes, md)
        assert d.tobytes() == d2.tobytes() and w.tobytes() == w2.tobytes()
        for m, mesh in enumerate(meshes):
            ds, ws = _query(rz, pts, [mesh], md)
            assert ds[0].tobytes() == d[m].tobytes() and ws[0].tobytes() == w[m].tobytes(), (md, m)
        assert (d[1] == np.inf).all() and (w[1] == 0).all()
        _check(f"four meshes md={md}", (d, w), ("four", md), pts, meshes, md, threshold=0.02)
    assert rz.query_meshes(pts[:0], meshes)["winding"].shape == (4, 0)


# ---- 8: end to end ---------------------------------------------------------------------------------------------------------------------------
def test_link_masks_end_to_end(rz):
    from sim_a_splat_amd.handler import SplatHandler
    rng = np.random.default_rng(31)
    icp = qc.shipped_similarity()
    shift = np.eye(4)
    shift[:3, 3] = (0.35, 0.0, 0.0)
    meshes, transforms = [qc.tblock_mesh(), qc.base_mesh()], [icp @ shift, icp]
    placed = [qc.moved(m, T) for m, T in zip(meshes, transforms)]
    c0, c1 = placed[0][0].mean(0), placed[1][0].mean(0)
    lo, hi = np.minimum(c0, c1) - 0.4, np.maximum(c0, c1) + 0.4
    lo[2] = max(placed[0][0][:, 2].max(), placed[1][0][:, 2].max()) + 0.1      # the background lies behind both links (+z)
    hi[2] = lo[2] + 0.5
    means = np.concatenate([qc.surface_points(placed[0], 2000, 0.006, rng), qc.surface_points(placed[1], 2000, 0.006, rng),
                            rng.uniform(lo, hi, (2000, 3))]).astype(np.float32)
    masks = segment.link_masks_from_meshes(means, meshes, transforms, distance=0.015, rasterizer=rz)
    assert list(masks) == ["link0", "link1"]
    # the reference masks under the decision rule
    r64, r32 = qc.reference("e2e", means, placed, 0.015)
    tols = qc.tolerances(means, placed, r64, r32)
    for k, (tol_d, tol_w, _, _) in enumerate(tols):
        want = (r64["winding"][k] > 0.5) | (r64["distance"][k] < 0.015)
        undecidable = (np.abs(r64["distance"][k] - 0.015) <= tol_d) | (np.abs(r64["winding"][k] - 0.5) <= tol_w)
        got = masks[f"link{k}"]
        print(f"  end to end link{k}: mask {int(got.sum())} (reference {int(want.sum())}), flipped {int((got != want).sum())}, undecidable {int(undecidable.sum())}")
        assert not ((got != want) & ~undecidable).any() and undecidable.sum() <= 60
        assert 1000 < got.sum() <= 2000 + 50
    # without a rasterizer of the caller's the call makes its own
    own = segment.link_masks_from_meshes(means[:300], meshes, transforms, distance=0.015)
    assert all((own[k] == masks[k][:300]).all() for k in masks)
    # the masks build a handler, whose groups are the masks', and both links show in a label image
    n = len(means)
    covs = np.tile(np.eye(3, dtype=np.float32) * 1e-4, (n, 1, 1))
    colors = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
    h = SplatHandler.from_arrays(means, covs, colors, np.full(n, 0.9, np.float32), masks, icp, [np.eye(4)] * 2, device=0)
    try:
        sizes = [g["centers"].shape[0] for g in h.scene._groups]
        rest = ~(masks["link0"] | masks["link1"])
        assert sizes == [int(masks["link0"].sum()), int(masks["link1"].sum()), int(rest.sum())]
        mid = 0.5 * (c0 + c1)
        cam = (np.array([1.0, 0.0, 0.0, 0.0]), mid + np.array([0.0, 0.0, -0.6]))     # looks along +z at both links
        labels, = h.render_segmentation(h.scene, [cam], [[120, 160]])
        names = h.scene.row_names()
        seen = {names[r] for r in np.unique(labels) if r != 255}
        print(f"  end to end labels: {sorted(seen)}")
        assert labels.shape == (120, 160) and {"robot/splat_robot/link0", "robot/splat_robot/link1"} <= seen
    finally:
        h.scene.close()


# ---- 9: errors -----------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(rz):
    import torch
    L = _capi.lib()
    v = np.ascontiguousarray(qc.TRIANGLE[0], np.float32)
    pts = np.zeros((4, 3), np.float32)
    out = torch.full((1, 4), 7.0, dtype=torch.float32, device=rz.device)

    def call(tri, offsets, md, dist, wind, n_meshes=1):
        t = np.ascontiguousarray(tri, np.int32)
        o = np.ascontiguousarray(offsets, np.int64)
        rc = L.sas_query_meshes(rz._ctx, 4, pts.ctypes.data, 3, v.ctypes.data, t.shape[0], t.ctypes.data, n_meshes, o.ctypes.data,
                                ctypes.c_float(md), dist, wind, None)
        return rc, L.sas_last_error(rz._ctx).decode()

    good = [[0, 1, 2]]
    assert call(good, [0, 1], 1.0, out.data_ptr(), None)[0] == 0
    for what, args in {"index out of range": ([[0, 1, 3]], [0, 1], 1.0, out.data_ptr(), None),
                       "negative index": ([[0, -1, 2]], [0, 1], 1.0, out.data_ptr(), None),
                       "offsets do not end at n_triangles": (good, [0, 2], 1.0, out.data_ptr(), None),
                       "offsets do not start at 0": (good, [1, 1], 1.0, out.data_ptr(), None),
                       "offsets decrease": ([[0, 1, 2], [0, 1, 2]], [0, 2, 1, 2], 1.0, out.data_ptr(), None, 3),
                       "max_distance -1": (good, [0, 1], -1.0, out.data_ptr(), None),
                       "max_distance NaN": (good, [0, 1], float("nan"), out.data_ptr(), None),
                       "both outputs NULL": (good, [0, 1], 1.0, None, None),
                       "no mesh": (good, [0, 1], 1.0, out.data_ptr(), None, 0)}.items():
        rc, msg = call(*args)
        print(f"  {what}: status {rc}, {msg!r}")
        assert rc == -1 and msg, what
    with pytest.raises(_capi.SasError):
        rz.query_meshes(pts, [qc.TRIANGLE], -1.0)
    # the context still answers
    d, w = _query(rz, np.array([[0.25, 0.25, 0.5]]), [qc.TRIANGLE])
    assert d[0, 0] == 0.5
