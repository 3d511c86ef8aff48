"""CPU: the float64 form of the mesh-query reference (tests/tools/mesh_query_ref.py) against closed forms, the crop volume of
sim_a_splat_amd/segment.py against a brute-force crossing count, and the masks' round trip through the files SplatHandler reads.
The GPU is held to this reference in tests/test_gpu_l_mesh_query.py."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_query_cases as qc  # noqa: E402
import mesh_query_ref as ref  # noqa: E402

from sim_a_splat_amd import io, segment  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


# ---- the reference against closed forms ------------------------------------------------------------------------------------------------
def test_committed_meshes_are_closed():
    v, f = qc.base_mesh()
    assert (len(v), len(f)) == (1222, 2464) and qc.unmatched_edges(f) == 0
    v, f = qc.tblock_mesh()
    assert (len(v), len(f)) == (16, 28) and qc.unmatched_edges(f) == 0
    assert qc.unmatched_edges(qc.box_mesh()[1]) == 0


def test_box_distance_and_winding_closed_form():
    h = np.array([0.5, 0.3, 0.2])
    v, f = qc.box_mesh(h)
    p = qc.box_points(400, h=h).astype(np.float32).astype(np.float64)
    d, w = ref.query_mesh(p, v.astype(np.float32), f, np.float64)
    h32 = h.astype(np.float32).astype(np.float64)
    inside = (np.abs(p) < h32).all(axis=1)
    want = np.where(inside, (h32 - np.abs(p)).min(axis=1), np.linalg.norm(np.maximum(np.abs(p) - h32, 0.0), axis=1))
    assert inside.sum() > 20 and (~inside).sum() > 20
    assert np.abs(d - want).max() <= 1e-12
    assert np.abs(w - inside).max() <= 1e-12


def test_tblock_inside_is_the_t_polygon_times_z():
    v, f = qc.tblock_mesh()
    rng = np.random.default_rng(5)
    p = rng.uniform([-0.15, -0.22, -0.03], [0.15, 0.07, 0.07], (600, 3)).astype(np.float32).astype(np.float64)
    # keep clear of the surface: inside / outside is then decided
    d, w = ref.query_mesh(p, v, f, np.float64)
    clear = d > 1e-6
    inside = qc.tblock_inside(p)
    assert inside[clear].sum() > 20
    assert np.abs(w[clear] - inside[clear]).max() <= 1e-9


def test_single_triangle_seven_regions():
    v, f = qc.TRIANGLE
    p = np.array([q for q, _ in qc.SEVEN_REGIONS.values()])
    want = np.array([d for _, d in qc.SEVEN_REGIONS.values()])
    assert (p.astype(np.float32) == p).all()
    d, w = ref.query_mesh(p, v, f, np.float64)
    assert np.abs(d - want).max() <= 1e-12
    assert np.isfinite(w).all() and np.abs(w).max() < 0.5


def test_zero_area_triangle_reads_segment_distance_and_no_solid_angle():
    v, f = qc.ZERO_AREA
    for dtype in (np.float64, np.float32):
        d, w = ref.query_mesh(qc.ZERO_AREA_POINTS, v, f, dtype)
        assert np.abs(d - qc.ZERO_AREA_DISTANCE).max() <= (1e-12 if dtype is np.float64 else 1e-6)
        assert (w == 0).all()
    # two coincident vertices as well
    d, w = ref.query_mesh(qc.ZERO_AREA_POINTS, v, np.array([[0, 0, 2]]), np.float64)
    assert np.abs(d - qc.ZERO_AREA_DISTANCE).max() <= 1e-12 and (w == 0).all()


def test_non_finite_inputs_are_defined():
    v, f = qc.nan_vertex_mesh()
    p = np.array([[0.25, 0.25, 0.5], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    r = ref.query(p, [(v, f)], np.inf)
    assert r["culled"][0].tolist() == [False, True, True]
    assert r["distance"][0, 0] == 0.5 and np.isinf(r["distance"][0, 1:]).all() and (r["winding"][0, 1:] == 0).all()
    assert len(ref.kept_faces(v, f)) == 1
    empty = ref.query(p, [(v, np.zeros((0, 3), np.int64))], np.inf)
    assert empty["culled"].all() and np.isinf(empty["distance"]).all() and (empty["winding"] == 0).all()


def test_cull_rule_is_the_inflated_box():
    v, f = qc.box_mesh((0.5, 0.3, 0.2))
    p = np.array([[0.6, 0.0, 0.0], [0.61, 0.0, 0.0], [0.0, -0.41, 0.0], [0.0, 0.0, 0.29], [0.59, 0.39, 0.29]])
    assert ref.culled(p, v, f, 0.1).tolist() == [False, True, True, False, False]
    assert not ref.culled(p, v, f, np.inf).any()
    # the mask rule with culling and without it agree (a culled point is further than the threshold and outside)
    pts = qc.box_points(300)
    a = ref.link_masks(pts, [(v, f)], 0.05)
    r = ref.query(pts, [(v, f)], np.inf)
    assert (a == ((r["winding"] > 0.5) | (r["distance"] < 0.05))).all()


def test_float32_yardstick_is_close_to_the_reference():
    mesh, pts = qc.similarity_points(200)
    r64, r32 = qc.reference("cpu_similarity_200", pts, [mesh], 0.015)
    (tol_d, tol_w, e_d, e_w), = qc.tolerances(pts, [mesh], r64, r32)
    print(f"  e32_d = {e_d:.2e}, e32_w = {e_w:.2e}, tol_d = {tol_d:.2e}, tol_w = {tol_w:.2e}")
    assert e_d < 1e-5 and e_w < 1e-3
    assert (r64["culled"] == r32["culled"]).all() and r64["culled"].any() and not r64["culled"].all()


# ---- the crop volume ---------------------------------------------------------------------------------------------------------------------
def _crossings(p, poly, u, v):
    """Brute force, one point and one edge at a time."""
    out = np.zeros(len(p), bool)
    for i, q in enumerate(p):
        n = 0
        for k in range(len(poly)):
            (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % len(poly)]
            if (y0 > q[v]) != (y1 > q[v]) and q[u] < x0 + (q[v] - y0) * (x1 - x0) / (y1 - y0):
                n += 1
        out[i] = n % 2 == 1
    return out


def _clear_of(p, poly, u, v, w, lo, hi, eps=1e-6):
    """Points at least ``eps`` from every edge of the outline and from both end faces."""
    ok = (np.abs(p[:, w] - lo) > eps) & (np.abs(p[:, w] - hi) > eps)
    for k in range(len(poly)):
        a, b = poly[k], poly[(k + 1) % len(poly)]
        e = b - a
        t = np.clip(((p[:, [u, v]] - a) @ e) / (e @ e), 0, 1)
        ok &= np.linalg.norm(p[:, [u, v]] - (a + t[:, None] * e), axis=1) > eps
    return ok


@pytest.mark.parametrize("axis", ["Z", "X", "Y"])
def test_polygon_volume_mask_concave(axis):
    poly = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [1.0, 0.5], [0.0, 2.0]])   # an "M": concave at (1, 0.5)
    u, v, w = segment.AXES[axis]
    rng = np.random.default_rng(2)
    p = rng.uniform(-0.5, 2.5, (800, 3))
    p = p[_clear_of(p, poly, u, v, w, 0.2, 1.7)]
    got = segment.polygon_volume_mask(p, poly, 0.2, 1.7, axis)
    want = _crossings(p, poly, u, v) & (p[:, w] >= 0.2) & (p[:, w] <= 1.7)
    assert (got == want).all() and 50 < got.sum() < len(p) - 50
    # the notch of the M is outside, its legs inside
    probe = np.zeros((2, 3))
    probe[:, w] = 1.0
    probe[0, [u, v]], probe[1, [u, v]] = (1.0, 1.5), (0.3, 1.0)
    assert segment.polygon_volume_mask(probe, poly, 0.2, 1.7, axis).tolist() == [False, True]


def test_polygon_volume_mask_shipped_bounds(golden_dir):
    poly3 = np.load(golden_dir / "scene_assets_divar113vhw.npz")["polygon_bounds"]   # [4,3], the reference's crop (match_splat.py:154-163)
    rng = np.random.default_rng(4)
    p = rng.uniform([-0.5, 0.0, -0.5], [0.7, 0.9, 0.3], (1000, 3))
    p = p[_clear_of(p, poly3[:, :2], 0, 1, 2, -0.3, 0.1)]
    got = segment.polygon_volume_mask(p, poly3, -0.3, 0.1, "Z")
    want = _crossings(p, poly3[:, :2], 0, 1) & (p[:, 2] >= -0.3) & (p[:, 2] <= 0.1)
    assert (got == want).all()
    box = (p[:, 0] > -0.25) & (p[:, 0] < 0.42) & (p[:, 1] > 0.2) & (p[:, 1] < 0.62) & (p[:, 2] > -0.3) & (p[:, 2] < 0.1)
    assert (got == box).all() and got.sum() > 50
    assert (segment.polygon_volume_mask(p, poly3[:, :2], -0.3, 0.1) == got).all()


# ---- masks: from a query to the files ------------------------------------------------------------------------------------------------------
class _StubRasterizer:
    """query_meshes by the NumPy reference: what link_masks_from_meshes asks of a Rasterizer."""

    def __init__(self):
        self.calls = []

    def query_meshes(self, points, meshes, max_distance=np.inf):
        self.calls.append((len(points), len(meshes), max_distance))
        r = ref.query(points, meshes, max_distance, np.float64)
        return {"distance": r["distance"].astype(np.float32), "winding": r["winding"].astype(np.float32)}


def test_link_masks_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    T = qc.shipped_similarity()
    box = qc.box_mesh((0.05, 0.04, 0.03))
    shift = np.eye(4)
    shift[:3, 3] = (0.3, 0.0, 0.1)
    meshes, transforms = [qc.tblock_mesh(), box], [T, T @ shift]
    centre = [segment.transform_vertices(v, X).mean(0) for (v, _), X in zip(meshes, transforms)]
    means = np.concatenate([rng.normal(centre[0], 0.03, (150, 3)), rng.normal(centre[1], 0.02, (150, 3)), rng.uniform(-1, 1, (100, 3))])
    crop = np.ones(len(means), bool)
    crop[::7] = False
    stub = _StubRasterizer()
    masks = segment.link_masks_from_meshes(means, meshes, transforms, distance=0.015, crop=crop, rasterizer=stub)
    assert stub.calls == [(int(crop.sum()), 2, 0.015)]
    assert list(masks) == ["link0", "link1"] and all(m.dtype == bool and m.shape == (400,) for m in masks.values())
    want = ref.link_masks(means, [qc.moved(m, X) for m, X in zip(meshes, transforms)], 0.015) & crop
    for k in range(2):
        assert (masks[f"link{k}"] == want[k]).all() and 10 < masks[f"link{k}"].sum() < 300
    assert not (masks["link0"] & ~crop).any()
    d = segment.write_masks_dir(tmp_path / "masks", masks, np.arange(6.0), T)
    back = io.load_link_masks(d / "link_masks_global_dict.npz")
    assert list(back) == list(masks) and all((back[k] == masks[k]).all() for k in masks)
    assert (io.load_joint_config(d / "joint_config.npy") == np.arange(6.0)).all()
    assert (io.load_icp_transformation(d / "icp_transformation.npy") == T).all()
    # no crop, no rasterizer call for an empty crop
    none = segment.link_masks_from_meshes(means, meshes, transforms, crop=np.zeros(400, bool), rasterizer=stub)
    assert len(stub.calls) == 1 and not any(m.any() for m in none.values())


def _two_link_robot(root, golden_dir):
    """A URDF of two links (the base mesh, the T-block on a revolute joint) with its mesh files under ``root``; returns its path."""
    (root / "meshes").mkdir()
    (root / "meshes" / "base.stl").write_bytes((golden_dir / "xarm6_base.stl").read_bytes())
    (root / "meshes" / "t.obj").write_bytes((golden_dir / "tblock_paper.obj").read_bytes())
    urdf = root / "r.urdf"
    urdf.write_text("""<robot name="r">
  <link name="base"><visual><geometry><mesh filename="package://pkg/meshes/base.stl"/></geometry></visual></link>
  <link name="arm"><visual><origin xyz="0 0 0.1"/><geometry><mesh filename="package://pkg/meshes/t.obj"/></geometry></visual></link>
  <joint name="j" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 0.2"/><axis xyz="0 0 1"/></joint>
</robot>""")
    return urdf


def test_robot_link_meshes_pairs_visuals_with_their_fk(tmp_path, golden_dir):
    urdf = _two_link_robot(tmp_path, golden_dir)
    icp = qc.shipped_similarity()
    meshes, transforms = segment.robot_link_meshes(urdf, [np.pi / 2], icp, str(tmp_path), "pkg", n_links=7)
    assert [len(f) for _, f in meshes] == [2464, 28] and len(meshes[0][0]) == 1222      # welded, URDF order
    arm = np.eye(4)
    arm[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    arm[:3, 3] = (0, 0, 0.3)
    assert np.allclose(transforms[0], icp) and np.allclose(transforms[1], icp @ arm)
    one = segment.robot_link_meshes(urdf, [0.0], icp, str(tmp_path), "pkg", n_links=1)
    assert len(one[0]) == 1 and len(one[1]) == 1


def test_command_line_writes_the_masks_directory(tmp_path, golden_dir, monkeypatch, capsys):
    """python -m sim_a_splat_amd.segment, with the NumPy reference where the GPU would answer."""
    import sim_a_splat_amd.rasterizer as rasterizer_module

    class Stub(_StubRasterizer):
        def __init__(self, device):
            super().__init__()

        def close(self):
            pass

    monkeypatch.setattr(rasterizer_module, "Rasterizer", Stub)
    urdf = _two_link_robot(tmp_path, golden_dir)
    icp = qc.shipped_similarity()
    meshes, transforms = segment.robot_link_meshes(urdf, [0.5], icp, str(tmp_path), "pkg")
    rng = np.random.default_rng(12)
    means = np.concatenate([qc.surface_points(qc.moved(m, T), 60, 0.004, rng) for m, T in zip(meshes, transforms)]
                           + [rng.uniform(-1, 1, (80, 3))]).astype(np.float32)
    np.save(tmp_path / "means.npy", means)
    np.save(tmp_path / "icp.npy", icp)
    lo, hi = means[:120, :2].min(0) - 0.01, means[:120, :2].max(0) + 0.01
    np.save(tmp_path / "poly.npy", np.array([[lo[0], lo[1], 0], [hi[0], lo[1], 0], [hi[0], hi[1], 0], [lo[0], hi[1], 0]]))
    out = tmp_path / "masks" / "r"
    rc = segment.main(["--splat", str(tmp_path / "means.npy"), "--urdf", str(urdf), "--joint-config", "0.5", "--icp", str(tmp_path / "icp.npy"),
                       "--robot-description-dir", str(tmp_path), "--package-name", "pkg", "--out", str(out), "--polygon",
                       str(tmp_path / "poly.npy"), "--axis-min", "-10", "--axis-max", "10"])
    assert rc == 0 and "link1:" in capsys.readouterr().out
    masks = io.load_link_masks(out / "link_masks_global_dict.npz")
    crop = segment.polygon_volume_mask(means, np.load(tmp_path / "poly.npy"), -10, 10)
    want = ref.link_masks(means, [qc.moved(m, T) for m, T in zip(meshes, transforms)], 0.015) & crop
    assert list(masks) == ["link0", "link1"] and all((masks[f"link{k}"] == want[k]).all() for k in range(2))
    assert masks["link0"].sum() > 30 and masks["link1"].sum() > 30 and crop[:120].all() and not crop.all()
    assert (io.load_joint_config(out / "joint_config.npy") == [0.5]).all() and (io.load_icp_transformation(out / "icp_transformation.npy") == icp).all()


def test_query_chunk_constant_matches_the_kernel():
    from sim_a_splat_amd import _capi
    text = (ROOT / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()
    assert int(re.search(r"#define SAS_QUERY_CHUNK (\d+)", text).group(1)) == _capi.SAS_QUERY_CHUNK


def test_pack_query_meshes():
    from sim_a_splat_amd.rasterizer import pack_query_meshes
    v, f, off = pack_query_meshes([qc.tblock_mesh(), (np.zeros((0, 3)), np.zeros((0, 3), int)), qc.box_mesh()])
    assert v.dtype == np.float32 and f.dtype == np.int32 and off.tolist() == [0, 28, 28, 40]
    assert v.shape == (24, 3) and f[28:].min() == 16 and f[28:].max() == 23
    with pytest.raises(ValueError):
        pack_query_meshes([(np.zeros((3, 3)), np.array([[0, 1, 3]]))])
    with pytest.raises(ValueError):
        pack_query_meshes([])
