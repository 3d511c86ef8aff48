"""CPU: the restatement of the deformable splats (tests/tools/skin_ref.py; DESIGN.md 3, "Deformation") against first principles, and the
host-side conveniences of sim_a_splat_amd.deform.  The GPU tests (tests/test_gpu_zd_skin.py) hold the kernels to this restatement."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import knn_ref as kr  # noqa: E402
import skin_ref as sr  # noqa: E402

from sim_a_splat_amd import deform  # noqa: E402


def _rigid(seed, angle=1.1):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R = sr.quat_to_matrix(np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis]))
    return R, rng.uniform(-0.5, 0.5, 3)


def _one_node_skin(n, index=0):
    return np.full((n, 1), index, np.int32), np.ones((n, 1), np.float32)


@pytest.mark.parametrize("form", ("quats", "covariances"))
def test_one_node_with_weight_one_is_the_rigid_transform(form):
    kw = sr.scene(form)
    R, t = _rigid(1)
    G = np.concatenate([R, t[:, None]], axis=1)[None].astype(np.float32)
    R32, t32 = G[0, :, :3].astype(np.float64), G[0, :, 3].astype(np.float64)
    idx, w = _one_node_skin(sr.N)
    got = sr.deform_ref(sr.rest_of(kw), idx, w, G)
    m = kw["means"].astype(np.float64)
    assert np.abs(got["means"] - (m @ R32.T + t32)).max() < 1e-6   # (R32 is orthonormal to float32 precision only)
    if form == "quats":
        Rg, Rr = sr.quat_to_matrix(got["quats"]), sr.quat_to_matrix(kw["quats"])
        assert np.abs(Rg - R32 @ Rr).max() < 1e-6
    else:
        c = kw["covariances"].astype(np.float64)
        S = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)
        want = R32 @ S @ R32.T
        g = got["covariances"]
        G6 = np.stack([g[:, [0, 1, 2]], g[:, [1, 3, 4]], g[:, [2, 4, 5]]], axis=1)
        assert np.abs(G6 - want).max() < 1e-6 * np.abs(want).max() + 1e-9


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("form", ("quats", "covariances"))
def test_identity_transforms_return_the_rest_means_exactly(form, dtype):
    kw = sr.scene(form)
    q = sr.nodes("m70")
    d2, idx = sr.knn_cross_ref(kw["means"], q, 4)
    idx, w = sr.weights_ref(d2, idx, sr.default_sigma(q), dtype)
    assert not np.allclose(w.sum(axis=1), 1.0)   # the form does not need W = 1
    got = sr.deform_ref(sr.rest_of(kw), idx, w, sr.identity_transforms(70), dtype)
    assert got["means"].dtype == dtype and np.array_equal(got["means"], kw["means"].astype(dtype))
    if form == "quats":   # identity nodes: q_b = (1, 0, 0, 0) up to rounding of the sum's norm
        assert np.abs(got["quats"] - kw["quats"]).max() < 1e-6 * np.abs(kw["quats"]).max()


def test_sign_alignment_blends_q_and_minus_q_to_the_same_result():
    """Rotations by -(pi/2 - eps) and -(pi/2 + eps) about z are nearly the same matrix, but the conversion reaches them through different
    branches (the trace's: w > 0; R22's: z > 0) and returns nearly OPPOSITE quaternions.  Their blend must be the rotation between them,
    not a cancelled sum."""
    kw = sr.scene("quats", n=50)
    axis = np.array([0.0, 0.0, 1.0])
    def rot(a):
        return sr.quat_to_matrix(np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * axis]))
    A, B = rot(-(np.pi / 2 - 1e-3)), rot(-(np.pi / 2 + 1e-3))
    G = np.zeros((2, 3, 4), np.float32)
    G[0, :, :3], G[1, :, :3] = A, B
    Q = sr.node_quats(G[:, :, :3])
    assert Q[0] @ Q[1] < -0.99                  # opposite signs out of the conversion
    idx = np.tile(np.array([[0, 1]], np.int32), (50, 1))
    w = np.full((50, 2), 0.5, np.float32)
    got = sr.deform_ref(sr.rest_of(kw), idx, w, G)
    one = sr.deform_ref(sr.rest_of(kw), idx[:, :1], w[:, :1], G[:1])
    Rg, Ro = sr.quat_to_matrix(got["quats"]), sr.quat_to_matrix(one["quats"])
    assert np.abs(Rg - Ro).max() < 2e-3         # the half-way rotation, not a cancelled sum
    swapped = sr.deform_ref(sr.rest_of(kw), idx[:, ::-1], w, G)   # the other node first: the same rotation, the quaternion's sign may differ
    assert np.abs(sr.quat_to_matrix(swapped["quats"]) - Rg).max() < 1e-6


def test_entries_that_are_not_live_are_ignored():
    kw = sr.scene("quats", n=64)
    G = sr.transforms(sr.nodes("m3"))
    idx = np.tile(np.array([[-1, 3, 100, 1]], np.int32), (64, 1))
    w = np.tile(np.array([[1.0, 1.0, 1.0, 0.0]], np.float32), (64, 1))
    got = sr.deform_ref(sr.rest_of(kw), idx, w, G, np.float32)
    assert np.array_equal(got["means"], kw["means"]) and np.array_equal(got["quats"], kw["quats"])
    w[:, 3] = 0.25
    moved = sr.deform_ref(sr.rest_of(kw), idx, w, G, np.float32)
    only = sr.deform_ref(sr.rest_of(kw), idx[:, 3:], w[:, 3:], G, np.float32)
    assert np.array_equal(moved["means"], only["means"]) and np.array_equal(moved["quats"], only["quats"])
    assert not np.array_equal(moved["means"], kw["means"])


def test_knn_cross_ref_against_float64_and_its_edge_cases():
    p, q = sr.cloud(200), sr.nodes("m70")
    d2, idx = sr.knn_cross_ref(p, q, 4)
    full = ((q.astype(np.float64)[None] - p.astype(np.float64)[:, None]) ** 2).sum(axis=2)
    assert np.array_equal(idx, np.argsort(full, axis=1, kind="stable")[:, :4])          # (no near-ties in this draw)
    assert (np.diff(d2, axis=1) >= 0).all()
    # m < k: the last columns are missing
    d2, idx = sr.knn_cross_ref(p, sr.nodes("m3"), 8)
    assert (idx[:, 3:] == -1).all() and np.isinf(d2[:, 3:]).all() and (idx[:, :3] >= 0).all()
    # duplicates: the lower index first
    q = sr.nodes("dup")
    d2, idx = sr.knn_cross_ref(p, q, 2)
    assert np.array_equal(d2[:, 0], d2[:, 1]) and (idx[:, 0] < idx[:, 1]).all() and np.array_equal(q[idx[:, 0]], q[idx[:, 1]])
    # the cut: nothing beyond it, and some points with no neighbour at all
    d2, idx = sr.knn_cross_ref(p, sr.nodes("m70"), 4, 0.12)
    assert (d2[idx >= 0] <= np.float32(0.12) * np.float32(0.12)).all() and (idx[:, 0] < 0).any() and (idx[:, 0] >= 0).any()
    # non-finite points have no neighbours; non-finite nodes are nobody's
    pts, q = sr.non_finite_cloud(), sr.nodes("non_finite")
    d2, idx = sr.knn_cross_ref(pts, q, 3)
    bad_p = ~np.isfinite(pts).all(axis=1)
    assert (idx[bad_p] == -1).all() and (idx[200] == -1).all()
    assert not np.isin(idx, [3, 10, 20, 21, 40]).any()


def test_weights_ref_nearest_is_one_and_missing_is_zero():
    p, q = sr.cloud(200), sr.nodes("m70")
    d2, idx = sr.knn_cross_ref(p, q, 4, 0.25)
    keep = np.arange(200) % 2 == 0
    for dt in (np.float32, np.float64):
        i, w = sr.weights_ref(d2, idx, 0.01, dt, keep)   # a tiny sigma: the far weights underflow, the nearest stays 1
        has = i[:, 0] >= 0
        assert (w[has, 0] == 1).all() and (w[~has] == 0).all() and (i[~keep] == -1).all() and (w[~keep] == 0).all()
        assert (w[has].sum(axis=1) >= 1).all() and np.isfinite(w).all()
    assert sr.default_sigma(q) == pytest.approx(float(np.mean(np.sqrt(kr.knn_f64(q, 1)[0]))), rel=1e-6)
    assert sr.default_sigma(sr.nodes("m1")) == 1.0


def test_float32_restatement_is_close_to_float64():
    """What the GPU test's bound is made of: the float32 restatement's own error, at the level of float32 rounding."""
    for form in ("quats", "covariances"):
        kw = sr.scene(form)
        q = sr.nodes("m70")
        d2, idx = sr.knn_cross_ref(kw["means"], q, 4)
        idx, w = sr.weights_ref(d2, idx, sr.default_sigma(q), np.float32)
        G = sr.transforms(q)
        a, b = sr.deform_ref(sr.rest_of(kw), idx, w, G, np.float32), sr.deform_ref(sr.rest_of(kw), idx, w, G, np.float64)
        for k in a:
            assert a[k].dtype == np.float32 and 0.0 < sr.rel_err(a[k], b[k]) < 2e-6, (form, k, sr.rel_err(a[k], b[k]))
        assert np.abs(b["means"] - kw["means"]).max() > 0.01   # (the transforms do move the scene)


# ---- sim_a_splat_amd.deform -----------------------------------------------------------------------------------------------------------------
def test_transforms_from_positions_recovers_a_rigid_motion():
    rest = deform.grid_nodes(((-1.0, -0.5, 0.0), (1.0, 0.5, 0.25)), 0.25).astype(np.float64)
    R, t = _rigid(3)
    G = deform.transforms_from_positions(rest, rest @ R.T + t, neighbours=6)
    assert G.shape == (rest.shape[0], 3, 4) and G.dtype == np.float32
    # float64 inside: compare before the rounding to float32 by refitting in float64
    for i in (0, 7, rest.shape[0] - 1):
        Ri, ti = deform.kabsch(rest[[i, (i + 1) % len(rest), (i + 9) % len(rest), (i + 14) % len(rest)]],
                               (rest @ R.T + t)[[i, (i + 1) % len(rest), (i + 9) % len(rest), (i + 14) % len(rest)]])
        assert np.abs(Ri - R).max() < 1e-9 and np.abs(ti - t).max() < 1e-9
    assert np.abs(G[:, :, :3] - R).max() < 1e-6 and np.abs(G[:, :, 3] - t).max() < 1e-6
    assert deform.check_node_transforms(G) is not None
    # a bend: every node lands exactly on its moved position
    moved = rest.copy()
    moved[:, 2] += 0.1 * np.sin(3.0 * rest[:, 0])
    G = deform.transforms_from_positions(rest, moved).astype(np.float64)
    assert np.abs(np.einsum("mij,mj->mi", G[:, :, :3], rest) + G[:, :, 3] - moved).max() < 1e-6
    deform.check_node_transforms(G)
    with pytest.raises(ValueError, match="differ in shape"):
        deform.transforms_from_positions(rest, moved[:-1])


def test_transforms_from_positions_to_1e_9_in_float64():
    """The fit itself, before the float32 rounding of the result: the known motion to 1e-9."""
    rest = np.random.default_rng(5).uniform(-1, 1, (30, 3))
    R, t = _rigid(6, 2.5)
    Rf, tf = deform.kabsch(rest, rest @ R.T + t)
    assert np.abs(Rf - R).max() < 1e-9 and np.abs(tf - t).max() < 1e-9 and np.linalg.det(Rf) > 0.999999


def test_grid_and_farthest_nodes_shapes():
    g = deform.grid_nodes(((0.0, 0.0, 0.0), (0.7, 0.7, 0.0)), 0.1)
    assert g.shape == (64, 3) and g.dtype == np.float32 and (g[:, 2] == 0).all()
    assert np.allclose(g[0], 0.0) and np.allclose(g[-1], (0.7, 0.7, 0.0)) and np.allclose(g[1], (0.1, 0.0, 0.0))   # x fastest, faces included
    assert deform.grid_nodes(((0, 0, 0), (1, 2, 3)), 1.0).shape == (2 * 3 * 4, 3)
    with pytest.raises(ValueError):
        deform.grid_nodes(((0, 0, 0), (1, 1, 1)), 0.0)
    with pytest.raises(ValueError, match="65536"):
        deform.grid_nodes(((0, 0, 0), (1, 1, 1)), 0.01)
    p = sr.non_finite_cloud()
    f = deform.farthest_nodes(p, 16)
    assert f.shape == (16, 3) and f.dtype == np.float32 and np.isfinite(f).all() and np.array_equal(f[0], p[0])
    assert len({tuple(r) for r in f}) == 16
    d = np.sqrt(((f.astype(np.float64)[:, None] - f.astype(np.float64)[None]) ** 2).sum(axis=2)) + np.eye(16) * 1e9   # (one point lies 1e30 away)
    assert d.min() > 0.05                                     # spread, not a cluster
    assert deform.farthest_nodes(p[:3], 10).shape == (3, 3) and deform.farthest_nodes(p[:0], 4).shape == (0, 3)


def test_host_validation_of_node_transforms():
    G = sr.transforms(sr.nodes("m3"))
    assert deform.check_node_transforms(G.tolist()).dtype == np.float32
    sheared = G.copy()
    sheared[1, 0, 1] += 0.05
    with pytest.raises(ValueError, match=r"node_transforms\[1\].*rigid"):
        deform.check_node_transforms(sheared)
    scaled = G.copy()
    scaled[2, :, :3] *= 1.01
    with pytest.raises(ValueError, match=r"node_transforms\[2\]"):
        deform.check_node_transforms(scaled)
    mirrored = G.copy()
    mirrored[0, :, 0] *= -1.0
    with pytest.raises(ValueError, match="reflection"):
        deform.check_node_transforms(mirrored)
    nan = G.copy()
    nan[0, 2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        deform.check_node_transforms(nan)
    for bad in (G[0], G[:, :, :3], np.zeros((2, 4, 3))):
        with pytest.raises(ValueError, match=r"\[m,3,4\]"):
            deform.check_node_transforms(bad)
    assert deform.check_node_transforms(np.zeros((0, 3, 4))).shape == (0, 3, 4)
