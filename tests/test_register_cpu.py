"""CPU: the registration of sim_a_splat_amd/register.py around a NumPy matcher, and the yardsticks of the GPU test.

``umeyama`` and ``initial_guess`` against closed forms; ``mesh_io.sample_surface`` on the mesh, in proportion and repeatable; the
float32 restatement of the matching contract (tests/tools/match_ref.py: ``match32``, which the GPU equals bit for bit in
tests/test_gpu_m_match.py) held to its float64 form; ``register_similarity`` with those matchers on two drawn cases; the command line
with a stub matcher.  Limits are the issue's or are derived where they are asserted; every check prints what it measured."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import match_cases as mc  # noqa: E402
import match_ref as mr  # noqa: E402
import mesh_query_cases as qc  # noqa: E402
import mesh_query_ref as qref  # noqa: E402

from sim_a_splat_amd import io, mesh_io, poses, register  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
EPS64 = float(np.finfo(np.float64).eps)


def _pair_moments(p, q):
    """Moments of the correspondences p[i] <-> q[i]."""
    d2 = ((np.asarray(q, np.float64) - np.asarray(p, np.float64)) ** 2).sum(axis=1)
    return mr.moments64(p, q, d2, np.arange(len(p)))


# ---- umeyama ------------------------------------------------------------------------------------------------------------------------------
def test_umeyama_recovers_a_known_similarity():
    rng = np.random.default_rng(1)
    p = rng.normal(0, 0.3, (50, 3))
    T = register.umeyama(_pair_moments(p, mc.apply(mc.TRUTH, p)))
    print(f"  umeyama: |T - truth| max {np.abs(T - mc.TRUTH).max():.3e}")
    assert np.abs(T - mc.TRUTH).max() <= 1e-12 and (T[3] == [0, 0, 0, 1]).all()
    assert np.abs(T - mr.umeyama(_pair_moments(p, mc.apply(mc.TRUTH, p)))).max() <= 1e-12
    # without scaling: scale 1, and on a rigid truth the truth
    rigid = mc.similarity(1.0, (0.3, -0.5, 0.8), 12.0, (0.21, -0.13, 0.34))
    Tr = register.umeyama(_pair_moments(p, mc.apply(rigid, p)), with_scaling=False)
    assert np.abs(Tr - rigid).max() <= 1e-12
    Tn = register.umeyama(_pair_moments(p, mc.apply(mc.TRUTH, p)), with_scaling=False)
    assert abs(np.linalg.det(Tn[:3, :3]) - 1.0) <= 1e-12 and np.abs(Tn[:3, :3] @ Tn[:3, :3].T - np.eye(3)).max() <= 1e-12


def test_umeyama_mirrored_case_returns_a_proper_rotation():
    rng = np.random.default_rng(2)
    p = rng.normal(0, 0.3, (40, 3))
    q = mc.apply(mc.TRUTH, p * [1.0, 1.0, -1.0])     # a reflection fits exactly; no rotation does
    T = register.umeyama(_pair_moments(p, q))
    s = np.cbrt(np.linalg.det(T[:3, :3]))
    assert s > 0 and np.abs(T[:3, :3] @ T[:3, :3].T / s ** 2 - np.eye(3)).max() <= 1e-12
    poses.decompose_icp(T)


def test_umeyama_refuses_degenerate_input():
    p = np.array([[0.0, 0, 0], [1, 0, 0]])
    with pytest.raises(ValueError):
        register.umeyama(_pair_moments(p, p))
    with pytest.raises(ValueError):
        register.umeyama(np.zeros(18))
    same = np.tile([[0.5, 0.25, -1.0]], (4, 1))
    with pytest.raises(ValueError):
        register.umeyama(_pair_moments(same, np.random.default_rng(3).normal(size=(4, 3))))
    with pytest.raises(ValueError):
        register.umeyama(np.zeros(17))


# ---- initial_guess ------------------------------------------------------------------------------------------------------------------------
def test_initial_guess_hand_computed():
    src = np.array([[0.0, 0, 0], [2, 0, 0], [0, 4, 0], [0, 0, 6]])        # centre (0.5, 1, 1.5)
    tgt = np.array([[1.0, 1, 1], [3, 5, 7]])                              # centre (2, 3, 4)
    T = register.initial_guess(src, tgt)
    assert (T == [[1, 0, 0, 1.5], [0, 1, 0, 2], [0, 0, 1, 2.5], [0, 0, 0, 1]]).all()
    # a quarter turn about z, scale 2, an offset: the unrotated centre is subtracted, as in the reference
    T = register.initial_guess(src, tgt, rotation_xyz=(0, 0, np.pi / 2), scale=2.0, offset=(0.25, 0, -0.5))
    assert np.abs(T - [[0, -2, 0, 1.75], [2, 0, 0, 2], [0, 0, 2, 2.0], [0, 0, 0, 1]]).max() <= 1e-15
    # open3d's order: Rx Ry Rz
    R = register.rotation_from_xyz((np.pi / 2, np.pi / 2, 0))
    assert np.abs(R - [[0, 0, 1], [1, 0, 0], [0, 1, 0]]).max() <= 1e-15


# ---- sample_surface -----------------------------------------------------------------------------------------------------------------------
def test_sample_surface_lies_on_the_mesh_and_repeats():
    v, f = qc.base_mesh()
    a, b = mesh_io.sample_surface(v, f, 1500, seed=4), mesh_io.sample_surface(v, f, 1500, seed=4)
    assert a.dtype == np.float64 and a.shape == (1500, 3) and a.tobytes() == b.tobytes()
    assert mesh_io.sample_surface(v, f, 1500, seed=5).tobytes() != a.tobytes()
    # on the mesh: the float64 distance of tests/tools/mesh_query_ref.py.  Its query_mesh rounds points and vertices to float32 first (what
    # the GPU is handed), which alone moves a float64 point eps32 L off the surface; _distance64 is the same per-triangle evaluation,
    # through the reference's own _segment_d2 / _dot / _cross, on the float64 values
    L = float(np.abs(v).max())
    d = _distance64(a[::5], v, f)
    print(f"  sample_surface: largest distance to the mesh {d.max():.3e} (limit {16 * EPS64 * L:.3e})")
    assert d.max() <= 16 * EPS64 * L
    assert mesh_io.sample_surface(v, f, 0).shape == (0, 3)


def _distance64(points, vertices, faces):
    px = tuple(points[:, k] for k in range(3))
    best = np.full(len(points), np.inf)
    for i0, i1, i2 in faces:
        A, B, C = vertices[i0], vertices[i1], vertices[i2]
        a, b, c = (tuple(V[k] - px[k] for k in range(3)) for V in (A, B, C))
        e1, e2, e3 = tuple(B - A), tuple(C - A), tuple(C - B)
        d2 = np.minimum(np.minimum(qref._segment_d2(a, e1, np.float64), qref._segment_d2(b, e3, np.float64)), qref._segment_d2(a, e2, np.float64))
        n = qref._cross(e1, e2)
        nn = qref._dot(n, n)
        if nn > 0:
            s1, s2, s3 = qref._dot(n, qref._cross(a, e1)), qref._dot(n, qref._cross(b, e3)), qref._dot(n, qref._cross(e2, c))
            h = qref._dot(n, a)
            d2 = np.where((s1 >= 0) & (s2 >= 0) & (s3 >= 0), np.minimum(d2, h * h / nn), d2)
        best = np.fmin(best, d2)
    return np.sqrt(best)


def test_sample_surface_counts_follow_the_areas():
    v, f = qc.box_mesh()
    tri = v[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    share = area / area.sum()
    # n = 1240: every triangle's share (3, 5 or 7.5 of 62) is a whole number of strata, so the cumulative areas fall on stratum
    # borders and a triangle receives its n a points exactly -- up to the one point a border's rounding may move: +-1
    for n, limit in ((1240, 1.0), (1000, 2.0)):
        p = mesh_io.sample_surface(v, f, n, seed=3)
        counts = np.array([_on_triangle(p, tri[k]).sum() for k in range(len(f))])
        # (points on the shared diagonal of a face would count twice: none is)
        assert counts.sum() == n
        dev = np.abs(counts - n * share).max()
        print(f"  sample_surface counts n={n}: largest |count - n a| {dev:.3f} (limit {limit})")
        assert dev <= limit if limit == 1.0 else dev < limit
    # a zero-area triangle and one with a NaN vertex get none; the others' points do not move
    v2 = np.concatenate([v, [[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 0, 0]]])
    f2 = np.concatenate([f[:5], [[8, 9, 10]], f[5:], [[0, 1, 11]]])
    q = mesh_io.sample_surface(v2, f2, 1240, seed=3)
    assert np.isfinite(q).all() and q.tobytes() == mesh_io.sample_surface(v, f, 1240, seed=3).tobytes()
    with pytest.raises(ValueError):
        mesh_io.sample_surface(v2, [[8, 9, 10]], 10)


def _on_triangle(p, t):
    """bool [N]: p in the closed triangle t (box faces: exact in-plane test through barycentric coordinates)."""
    e1, e2 = t[1] - t[0], t[2] - t[0]
    n = np.cross(e1, e2)
    w = p - t[0]
    inplane = np.abs(w @ n) <= 1e-12
    d11, d12, d22 = e1 @ e1, e1 @ e2, e2 @ e2
    w1, w2 = w @ e1, w @ e2
    den = d11 * d22 - d12 * d12
    b = (d22 * w1 - d12 * w2) / den
    c = (d11 * w2 - d12 * w1) / den
    return inplane & (b >= -1e-12) & (c >= -1e-12) & (b + c <= 1 + 1e-12)


# ---- match32 held to match64 --------------------------------------------------------------------------------------------------------------
MATCH_CASES = {"none 257x300": (257, 300, None, np.inf), "similarity 700x700": (700, 700, mc.TRUTH, np.inf),
               "similarity 700x700 md 0.5": (700, 700, mc.TRUTH, 0.5)}


@pytest.mark.parametrize("name", list(MATCH_CASES))
def test_match32_against_match64(name):
    S, T, transform, md = MATCH_CASES[name]
    src, tgt = mc.drawn(S, T, seed=S + T)
    if transform is not None:
        transform = transform.astype(np.float32).astype(np.float64)     # (the rounding of the transform itself is the caller's)
    r32, r64 = mr.match32(src, tgt, transform, np.inf), mr.match64(src, tgt, transform, np.inf)
    L = mc.coordinate_scale(src, tgt, r64["moved"])
    tol = 4 * mc.EPS32 * L
    d32, d64 = np.sqrt(r32["dist2"].astype(np.float64)), np.sqrt(r64["dist2"])
    # the float64 runner-up: the nearest target other than the float64 match
    p, q = r64["moved"], tgt.astype(np.float64)
    d_all = np.sqrt(((q[None] - p[:, None]) ** 2).sum(-1))
    d_all[np.arange(S), r64["index"]] = np.inf
    runner = d_all.min(axis=1)
    differ = r32["index"] != r64["index"]
    print(f"  {name}: |d32 - d64| max {np.abs(d32 - d64).max():.3e} (tol {tol:.3e}), {int(differ.sum())} indices differ, "
          f"closest runner-up gap {np.min(runner - d64):.3e}")
    assert np.abs(d32 - d64).max() <= tol
    assert (runner[differ] - d64[differ] <= tol).all()
    # the threshold only removes matches
    if np.isfinite(md):
        h32 = mr.match32(src, tgt, transform, md)
        held = h32["index"] >= 0
        assert 0 < held.sum() < S and (h32["index"][held] == r32["index"][held]).all() and (h32["dist2"][held] <= np.float32(md) ** 2).all()
        assert (r32["dist2"][~held] > np.float32(md) ** 2).all() and h32["moments"][0] == held.sum()


def test_match_ref_ties_and_defined_inputs():
    tgt = np.array([[1.0, 0, 0], [-1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, 2, 0]], np.float32)
    src = np.array([[0.0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0]], np.float32)
    for match in (mr.match32, mr.match64):
        r = match(src, tgt)
        assert r["index"].tolist()[:3] == [0, -1, -1] and r["dist2"][0] == 1 and np.isinf(r["dist2"][1:3]).all()
        assert not np.isnan(r["dist2"]).any() and np.isfinite(r["moments"]).all()
    assert mr.match32(src, tgt)["index"][3] == -1          # 1e60 overflows float32: d2 is not < inf
    assert mr.match32(src, tgt[:0])["index"].tolist() == [-1] * 4 and mr.match32(src, tgt[:0])["moments"][0] == 0


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
def _errors(T, L):
    return float(np.abs(T[:3, :3] - mc.TRUTH[:3, :3]).max()), float(np.abs(T[:3, 3] - mc.TRUTH[:3, 3]).max()) / L


def test_register_similarity_clean_case():
    c = mc.clean_case()
    # the inputs are as the case's docstring says
    true = c["target"][:c["n_true"]].astype(np.float64)
    far = c["target"][c["n_true"]:].astype(np.float64)
    gap2 = ((far[:, None, :] - true[None, :, :]) ** 2).sum(-1).min()
    assert len(far) == 1000 and gap2 > 0.2 ** 2
    l32, l64, e32 = mc.loops("clean")
    for name, loop in (("float64", l64), ("float32", l32)):
        esr, et = _errors(loop["T"], c["L"])
        print(f"  clean case, {name} matcher: {loop['iterations']} iterations, |sR - sR_true| max {esr:.3e}, |t - t_true| / L {et:.3e}, "
              f"fitness {loop['fitness']:.4f}, rmse {loop['rmse']:.3e}")
        assert loop["iterations"] < 30 and esr <= 1e-5 and et <= 1e-5
    res = register.register_similarity(c["source"], c["target"], c["init"], matcher=mr.match32)
    esr, et = _errors(res.transformation, c["L"])
    assert esr <= 1e-5 and et <= 1e-5 and res.fitness == 1.0 and res.iterations < 30
    # the package's loop and the restated one are the same loop
    assert res.iterations == l32["iterations"] and np.abs(res.transformation - l32["T"]).max() <= 1e-12
    assert len(res.history) == res.iterations + 1 and res.history[-1] == (res.fitness, res.inlier_rmse)
    poses.decompose_icp(res.transformation)


def test_register_similarity_noisy_case():
    c = mc.noisy_case()
    l32, l64, e32 = mc.loops("noisy")
    res = register.register_similarity(c["source"], c["target"], c["init"], matcher=mr.match32)
    esr, et = _errors(l64["T"], c["L"])
    print(f"  noisy case: float64 loop {l64['iterations']} iterations, float32 loop {l32['iterations']}; e32 = |T32 - T64| max {e32:.3e}; "
          f"float64 loop against the truth: |sR| {esr:.3e}, |t| / L {et:.3e}; fitness {l64['fitness']:.4f}, rmse {l64['rmse']:.4e}")
    assert res.iterations == l32["iterations"] and np.abs(res.transformation - l32["T"]).max() <= 1e-12
    assert l64["iterations"] < 30 and l32["iterations"] < 30
    # against the truth only a sanity limit, ten standard errors: noise of sigma = 0.003 on n = 700 points of rms radius rho about
    # their centre turns and scales the fit by about sigma / (sqrt(n) rho), and moves t by that times the centre's distance from the
    # origin plus sigma / sqrt(n)
    src = c["source"].astype(np.float64)
    rho = float(np.sqrt(((src - src.mean(0)) ** 2).sum(1).mean()))
    se = 0.003 / (np.sqrt(len(src)) * rho)
    assert esr <= 10 * se and et * c["L"] <= 10 * (se * np.linalg.norm(src.mean(0)) + 0.003 / np.sqrt(len(src)))
    assert abs(l64["fitness"] - 1.0) < 1e-12 and 0.003 < l64["rmse"] < 0.003 * 2
    rigid = register.register_similarity(c["source"], c["target"], c["init"], matcher=mr.match32, with_scaling=False, max_iteration=3)
    assert abs(np.cbrt(np.linalg.det(rigid.transformation[:3, :3])) - 1.02 * 0.93) <= 1e-12 and rigid.iterations == 3


def test_register_similarity_needs_three_matches():
    src, tgt = mc.drawn(10, 10, seed=1, spread=0.01)
    far = np.eye(4)
    far[:3, 3] = 5.0
    with pytest.raises(ValueError):
        register.register_similarity(src, tgt, far, max_correspondence_distance=0.2, matcher=mr.match32)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
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


def test_command_line_round_trip(tmp_path, golden_dir, capsys):
    """python -m sim_a_splat_amd.register with the NumPy matcher where the GPU would answer."""
    urdf = _two_link_robot(tmp_path, golden_dir)
    robot = register.robot_surface_points(urdf, [0.5], str(tmp_path), "pkg", n_points=600, seed=1)
    assert robot.shape == (600, 3) and robot[:, 2].max() > 0.3         # the T block rides on the joint, 0.3 up
    truth = mc.similarity(0.93, (0.0, 0.0, 1.0), 4.0, (0.4, 0.3, -0.05))
    rng = np.random.default_rng(8)
    splat = np.concatenate([mc.apply(truth, register.robot_surface_points(urdf, [0.5], str(tmp_path), "pkg", n_points=900, seed=2))
                            + rng.normal(0, 0.001, (900, 3)), rng.uniform(-3, -2, (200, 3))]).astype(np.float32)
    np.save(tmp_path / "means.npy", splat)
    lo, hi = splat[:900, :2].min(0) - 0.02, splat[:900, :2].max(0) + 0.02
    poly = np.array([[lo[0], lo[1], 0], [hi[0], lo[1], 0], [hi[0], hi[1], 0], [lo[0], hi[1], 0]])
    np.save(tmp_path / "poly.npy", poly)
    out = tmp_path / "masks" / "r"
    calls = []

    def matcher(*a, **k):
        calls.append(k)
        return mr.match32(*a, **k)

    rc = register.main(["--splat", str(tmp_path / "means.npy"), "--urdf", str(urdf), "--joint-config", "0.5", "--robot-description-dir",
                        str(tmp_path), "--package-name", "pkg", "--polygon", str(tmp_path / "poly.npy"), "--axis-min", "-1", "--axis-max",
                        "1", "--points", "600", "--seed", "1", "--scale", "0.95", "--out", str(out)], matcher=matcher)
    assert rc == 0 and "fitness" in capsys.readouterr().out and calls and all(k["max_distance"] == 0.2 for k in calls)
    T = io.load_icp_transformation(out / "icp_transformation.npy")
    s, R, t = poses.decompose_icp(T)
    init = np.load(out / "trans_init.npy")
    crop = splat[:900]
    assert np.abs(init[:3, :3] - 0.95 * np.eye(3)).max() == 0 and np.abs(init[:3, 3] - (crop.astype(np.float64).mean(0) - robot.mean(0))).max() <= 1e-12
    print(f"  command line: scale {s:.5f} (truth 0.93), |T - truth| max {np.abs(T - truth).max():.3e}")
    # the file holds what register_robot returns for these inputs; against the truth only plausibility (the splat is another sampling
    # of a nearly cylindrical base, its points a centimetre apart: the loop's accuracy is the business of the two cases above)
    direct, _ = register.register_robot(splat, urdf, [0.5], str(tmp_path), "pkg", polygon=poly, axis_min=-1, axis_max=1, scale=0.95,
                                        n_points=600, seed=1, matcher=mr.match32)
    assert (T == direct.transformation).all()
    assert abs(s - 0.93) <= 0.01 and np.abs(T - truth).max() <= 0.02
    assert (np.load(out / "polygon_bounds.npy") == poly).all() and (io.load_joint_config(out / "joint_config.npy") == [0.5]).all()
    assert not (out / "link_masks_global_dict.npz").exists()


def test_match_constants_match_the_kernel():
    from sim_a_splat_amd import _capi
    from sim_a_splat_amd.rasterizer import MATCH_MOMENTS
    text = (ROOT / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()
    assert int(re.search(r"#define SAS_MATCH_CHUNK (\d+)", text).group(1)) == _capi.SAS_MATCH_CHUNK
    assert int(re.search(r"#define SAS_MATCH_MOMENTS (\d+)", text).group(1)) == MATCH_MOMENTS == register.N_MOMENTS
    assert "sas_match_points" in _capi.EXPORTS
