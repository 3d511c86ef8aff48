"""GPU: deformable splats (sas_knn_cross, sas_scene_skin, sas_scene_deform; Rasterizer.knn_nodes / set_skin / bind_skin / deform; DESIGN.md 3,
"Deformation") against tests/tools/skin_ref.py, the numpy restatement.  The cross-cloud kNN and the skin's round trip are compared for
EQUALITY; the deformed scene is held to the float64 restatement within four times the float32 restatement's own error (the measured
ratios are printed: profiles/deform.txt quotes them); what the contract makes exact -- Gaussians without a live entry, identity
transforms, clear_skin, no accumulation, the LDS and the global path, a frame of the deformed scene -- is compared bit for bit.
Frames are 64x48; scenes have 777 Gaussians in 2 groups (the n_pad tail), as quaternions and as covariances."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import Rasterizer, SasError

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import scene_cases as sc_kit  # noqa: E402
import skin_child  # noqa: E402
import skin_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
BG = (0.1, 0.2, 0.3)
FORMS = ("quats", "covariances")
_REF = {}


def _cam():
    return sc_kit.ring(W, H, f=55.0, yaw=25.0, elev=0.3)[:2]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _read(r):
    return {k: v.cpu().numpy() for k, v in r.read_scene().items()}


def _same_scene(a, b, rows=None):
    sel = slice(None) if rows is None else rows
    return set(a) == set(b) and all(_same_bits(a[k][sel], b[k][sel]) for k in a)


def _knn_ref(points_name, nodes_name, k, md=np.inf):
    key = (points_name, nodes_name, k, md)
    if key not in _REF:
        p = sr.non_finite_cloud() if points_name == "non_finite" else sr.cloud(int(points_name))
        _REF[key] = sr.knn_cross_ref(p, sr.nodes(nodes_name), k, md)
    return _REF[key]


def _points(r, points_name):
    p = sr.non_finite_cloud() if points_name == "non_finite" else sr.cloud(int(points_name))
    return torch.from_numpy(p).to(r.device)


def _knn_same(got, ref):
    d, i = ref
    gd, gi = got["dist2"].cpu().numpy(), got["index"].cpu().numpy()
    return gd.dtype == np.float32 and gi.dtype == np.int32 and gd.shape == d.shape and gi.shape == i.shape and \
        np.array_equal(_bits(gd), _bits(d)) and np.array_equal(gi, i)


# ---- knn_nodes ------------------------------------------------------------------------------------------------------------------------------
KNN_CASES = [("777", "m1", 1, np.inf), ("777", "m1", 4, np.inf), ("777", "m3", 4, np.inf), ("777", "m3", 8, np.inf), ("777", "m70", 1, np.inf),
             ("777", "m70", 3, np.inf), ("777", "m70", 4, np.inf), ("777", "m70", 8, np.inf), (str(sr.CHUNK + 1), "m%d" % (sr.CHUNK + 1), 8, np.inf),
             ("777", "m%d" % (sr.CHUNK + 1), 3, np.inf), ("777", "dup", 4, np.inf), ("777", "m70", 4, 0.2), ("777", "m70", 8, 0.35),
             ("non_finite", "non_finite", 3, np.inf), ("non_finite", "m70", 8, 0.5), ("1", "m70", 4, np.inf)]


@pytest.mark.parametrize("points,nodes,k,md", KNN_CASES)
def test_knn_nodes_is_the_restatement(rasterizer, points, nodes, k, md):
    r = rasterizer
    got = r.knn_nodes(_points(r, points), torch.from_numpy(sr.nodes(nodes)).to(r.device), k, md)
    ref = _knn_ref(points, nodes, k, md)
    assert got["dist2"].device == r.device and _knn_same(got, ref), (points, nodes, k, md)
    if nodes == "m3" and k > 3:
        assert (ref[1][:, 3:] == -1).all()                       # missing neighbours occur
    if md == 0.2:
        assert (ref[1][:, 0] < 0).any() and (ref[1][:, 0] >= 0).any() and (ref[1][:, -1] < 0).any()   # the cut leaves some points with none
    if nodes == "dup":
        assert (ref[1][:, 0] < ref[1][:, 1]).all() and np.array_equal(ref[0][:, 0], ref[0][:, 1])     # ties went to the lower index


def test_knn_nodes_inputs_streams_and_validation(rasterizer):
    r = rasterizer
    L = _capi.lib()
    q = sr.nodes("m70")
    # n = 0, host arrays and lists, without indices
    empty = r.knn_nodes(np.zeros((0, 3), np.float32), q, 5)
    assert tuple(empty["dist2"].shape) == (0, 5) and tuple(empty["index"].shape) == (0, 5) and empty["index"].dtype == torch.int32
    assert _knn_same(r.knn_nodes(sr.cloud(777), q.astype(np.float64).tolist(), 4), _knn_ref("777", "m70", 4))
    got = r.knn_nodes(sr.cloud(777), q, 4, indices=False)
    assert set(got) == {"dist2"} and _same_bits(got["dist2"], _knn_ref("777", "m70", 4)[0])
    # a side stream, and the default stream right behind it with nothing waited for
    side = torch.cuda.Stream(device=r.device)
    p, qd = _points(r, "777"), torch.from_numpy(q).to(r.device)
    torch.cuda.synchronize(r.device)
    with torch.cuda.stream(side):
        a = r.knn_nodes(p, qd, 8)
    b = r.knn_nodes(p, qd, 8)
    side.synchronize()
    torch.cuda.synchronize(r.device)
    assert _knn_same(a, _knn_ref("777", "m70", 8)) and _knn_same(b, _knn_ref("777", "m70", 8))
    # the C entry's validation
    d = torch.empty((777, 4), dtype=torch.float32, device=r.device)
    call = lambda n, m, k, md=float("inf"), pp=p.data_ptr(), qq=qd.data_ptr(), dd=d.data_ptr(): \
        L.sas_knn_cross(r._ctx, n, pp, m, qq, k, md, dd, None, None)
    for k in (0, -1, 9):
        assert call(777, 70, k) == -1 and b"k=" in L.sas_last_error(r._ctx)
    for m in (0, -1, 65537):
        assert call(777, m, 4) == -1 and b"m=" in L.sas_last_error(r._ctx)
    assert call(-1, 70, 4) == -1 and call(1 << 31, 70, 4) == -1
    assert call(777, 70, 4, -1.0) == -1 and call(777, 70, 4, float("nan")) == -1
    assert call(777, 70, 4, pp=None) == -1 and call(777, 70, 4, qq=None) == -1 and call(777, 70, 4, dd=None) == -1
    assert call(0, 70, 4, pp=None, qq=None, dd=None) == 0
    assert call(777, 70, 4) == 0
    torch.cuda.synchronize(r.device)
    assert _same_bits(d, _knn_ref("777", "m70", 4)[0])
    with pytest.raises(ValueError, match="nodes must be"):
        r.knn_nodes(sr.cloud(777), q[:, :2])
    with pytest.raises(SasError, match="status -1"):
        r.knn_nodes(sr.cloud(777), np.zeros((0, 3), np.float32))


# ---- set_skin / read_skin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 4, 5, 8))
def test_set_skin_read_skin_round_trip(rasterizer, k):
    r = rasterizer
    r.upload(**sr.scene("quats"))
    rng = np.random.default_rng(90 + k)
    idx = rng.integers(-2, 100, (sr.N, k)).astype(np.int32)
    w = rng.normal(0.0, 1.0, (sr.N, k)).astype(np.float32)
    w[3, 0], w[4, k - 1] = np.nan, np.inf
    assert not r.has_skin
    r.set_skin(torch.from_numpy(idx).to(r.device), torch.from_numpy(w).to(r.device))
    assert r.has_skin
    got = r.read_skin()
    assert got["indices"].dtype == torch.int32 and tuple(got["indices"].shape) == (sr.N, k) and got["weights"].device == r.device
    assert np.array_equal(got["indices"].cpu().numpy(), idx) and _same_bits(got["weights"], w)
    # a bind over the skin replaces the entries (host arrays, int64 indices)
    r.set_skin(idx[::-1].astype(np.int64), w[::-1].copy())
    got = r.read_skin()
    assert np.array_equal(got["indices"].cpu().numpy(), idx[::-1]) and _same_bits(got["weights"], w[::-1].copy())
    r.clear_skin()
    assert not r.has_skin
    with pytest.raises(SasError, match="no skin"):
        r.read_skin()


# ---- deform against the restatement ---------------------------------------------------------------------------------------------------------
def _deform_refs(form, name, k):
    """(indices, weights, transforms, float32 and float64 restatement) of a case, computed once."""
    key = ("deform", form, name, k)
    if key not in _REF:
        kw, q = sr.scene(form), sr.nodes(name)
        d2, idx = sr.knn_cross_ref(kw["means"], q, k)
        _REF[key] = (kw, q, d2, idx)
    return _REF[key]


@pytest.mark.parametrize("form,name,k", skin_child.CASES)
def test_deform_is_the_restatement_within_four_float32_errors(rasterizer, form, name, k):
    r = rasterizer
    kw, q, d2, idx_ref = _deform_refs(form, name, k)
    r.upload(**kw)
    before, order = _read(r), r.read_order().cpu().numpy()
    bound = r.bind_skin(q, k=k)
    idx, w = bound["indices"].cpu().numpy(), bound["weights"].cpu().numpy()
    assert np.array_equal(idx, idx_ref)
    G = sr.transforms(q)
    r.deform(torch.from_numpy(G).to(r.device))
    got = _read(r)
    r32, r64 = (sr.deform_ref(sr.rest_of(kw), idx, w, G, dt) for dt in (np.float32, np.float64))
    assert q.shape[0] <= sr.LDS_NODES or name == "m300"   # (the cases cover both sides of the LDS budget)
    for a in r64:
        e32, e = sr.rel_err(r32[a], r64[a]), sr.rel_err(got[a], r64[a])
        print(f"  deform {form} {name} k={k} {a}: device {e:.3e}, float32 restatement {e32:.3e}, ratio {e / e32:.2f}")
        assert e <= 4.0 * e32, (a, e, e32)
    assert np.abs(r64["means"] - kw["means"]).max() > 0.01
    # what a deformation never writes
    for a in ("opacities", "colors") + (("scales",) if form == "quats" else ()):
        assert _same_bits(got[a], before[a]), a
    assert np.array_equal(r.read_order().cpu().numpy(), order) and r.n == sr.N and r.has_skin


@pytest.mark.parametrize("budget", (0,))
def test_lds_and_global_paths_give_the_same_bits(rasterizer, tmp_path, budget):
    out = tmp_path / "skin_global.npz"
    env = dict(os.environ, SAS_SKIN_LDS=str(budget))
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "skin_child.py"), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "skin child ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
    bad = []
    with np.load(out) as z:
        for form, name, k in skin_child.CASES:
            mine = skin_child.deformed(rasterizer, form, name, k)
            bad += [(form, name, k, a) for a, v in mine.items() if not _same_bits(v, z[f"{form}_{name}_k{k}_{a}"])]
    assert not bad, bad


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_gaussians_without_a_live_entry_stay_at_rest(rasterizer, form):
    r = rasterizer
    kw, q = sr.scene(form), sr.nodes("m70")
    r.upload(**kw)
    rest = _read(r)
    assert _same_bits(rest["means"], kw["means"])
    bound = r.bind_skin(q, k=4, max_distance=0.3, group=1)
    idx, w = bound["indices"].cpu().numpy().copy(), bound["weights"].cpu().numpy().copy()
    gid = kw["group_id"]
    assert (idx[gid == 0] == -1).all() and (w[gid == 0] == 0).all()                        # outside the group
    far = (gid == 1) & (idx[:, 0] < 0)
    assert far.any() and ((gid == 1) & (idx[:, 0] >= 0)).sum() > 100                       # beyond max_distance: some, not all
    rows = np.nonzero((gid == 1) & (idx[:, 1] >= 0))[0]                                     # (two neighbours at least)
    assert rows.size >= 110
    idx[rows[0:20]] = 70                # index >= m
    idx[rows[20:40], :] = 1 << 30
    w[rows[40:60]] = 0.0                # weight 0
    w[rows[60:70]] = -1.0
    w[rows[70:80]] = np.nan
    idx[rows[80:100]] = -1              # index -1
    idx[rows[100:110], 0] = -5          # ... in the first entry alone: the others still count
    r.set_skin(idx, w)
    G = sr.transforms(q)
    r.deform(G)                          # (a host array: copied and checked)
    got = _read(r)
    live = ((idx >= 0) & (idx < 70) & (w > 0)).any(axis=1)
    assert 100 < live.sum() < sr.N - 300 and live[rows[100:110]].all() and not live[rows[:100]].any()
    assert _same_scene(got, rest, ~live)
    assert (np.abs(got["means"][live] - rest["means"][live]).max(axis=1) > 0).mean() > 0.99
    ref = sr.deform_ref(sr.rest_of(kw), idx, w, G, np.float32)
    assert np.abs(got["means"] - ref["means"]).max() < 1e-5


@pytest.mark.parametrize("form", FORMS)
def test_identity_clear_and_no_accumulation(rasterizer, form):
    r = rasterizer
    kw, q = sr.scene(form), sr.nodes("m70")
    V, K = _cam()
    r.upload(**kw)
    Rt = sc_kit.random_group_poses(sr.GROUPS, 7)
    r.set_group_poses(Rt)
    rest = _read(r)
    frame0 = sc_kit.to_numpy(r.render(V, K, W, H, BG))
    r.bind_skin(q, k=4)
    assert _same_scene(_read(r), rest)                                                      # binding moves nothing
    r.deform(sr.identity_transforms(70))
    got = _read(r)
    assert _same_bits(got["means"], rest["means"])                                          # identity: the rest means bit for bit
    if form == "covariances":
        assert np.abs(got["covariances"] - rest["covariances"]).max() < 1e-6 * np.abs(rest["covariances"]).max()
    A, B = sr.transforms(q, seed=81), sr.transforms(q, seed=82)
    r.deform(A)
    a = _read(r)
    r.deform(B)
    ab = _read(r)
    r.deform(sr.identity_transforms(70))
    r.deform(B)
    assert _same_scene(_read(r), ab) and not _same_bits(a["means"], ab["means"])            # rest -> current, never accumulated
    moved = sc_kit.to_numpy(r.render(V, K, W, H, BG))
    assert not np.array_equal(moved["rgb"], frame0["rgb"])
    r.clear_skin()
    assert not r.has_skin and _same_scene(_read(r), rest)
    sc_kit.same(sc_kit.to_numpy(r.render(V, K, W, H, BG)), frame0, keys=("rgb", "alpha", "depth"))
    r.clear_skin()                                                                          # without a skin: nothing
    assert _same_scene(_read(r), rest)


@pytest.mark.parametrize("form", FORMS)
def test_frames_show_the_deformed_scene(rasterizer, form):
    """A frame after deform is the frame of a second context that uploads the first one's read_scene() with the same groups and poses, with
    a non-identity pose on the deformable group."""
    r = rasterizer
    kw, q = sr.scene(form), sr.nodes("m70")
    V, K = _cam()
    r.upload(**kw)
    Rt = sc_kit.random_group_poses(sr.GROUPS, 11, max_angle=0.5, max_shift=0.2)
    r.set_group_poses(Rt)
    r.bind_skin(q, k=4, group=1)
    r.deform(sr.transforms(q))
    frame = sc_kit.to_numpy(r.render(V, K, W, H, BG))
    arrays = _read(r)
    assert not _same_bits(arrays["means"], kw["means"])
    r2 = Rasterizer(0)
    try:
        r2.upload(**arrays, sh_degree=-1, group_id=kw["group_id"], n_groups=sr.GROUPS)
        r2.set_group_poses(Rt)
        other = sc_kit.to_numpy(r2.render(V, K, W, H, BG))
    finally:
        r2.close()
    assert frame["alpha"].max() > 0.5
    sc_kit.same(frame, other, keys=("rgb", "alpha", "depth"))


# ---- guards ---------------------------------------------------------------------------------------------------------------------------------
def test_calls_a_skin_refuses_and_what_ends_it(rasterizer):
    r = rasterizer
    kw, q = sr.scene("quats"), sr.nodes("m70")
    V, K = _cam()
    r.upload(**kw)
    r.bind_skin(q, k=4)
    r.deform(sr.transforms(q))
    held = _read(r)
    zero = {"means": torch.zeros((sr.N, 3), dtype=torch.float32, device=r.device)}
    refused = {"adam_step": lambda: r.adam_step(zero, {"means": 1e-3}, 1), "densify": lambda: r.densify(r.new_density_stats()),
               "mcmc_refine": lambda: r.mcmc_refine(), "mcmc_noise": lambda: r.mcmc_noise(1e-3, 1), "reset_opacity": lambda: r.reset_opacity(0.01)}
    for name, call in refused.items():
        with pytest.raises(SasError, match=r"scene is skinned: clear_skin\(\) first"):
            call()
        assert _same_scene(_read(r), held) and r.n == sr.N and r.has_skin, name
    # render_backward runs under a skin and returns finite gradients
    g = r.render_backward(V, K, W, H, g_rgb=np.full((H, W, 3), 0.01, np.float32))
    assert all(torch.isfinite(v).all() for v in g.values()) and float(g["means"].abs().max()) > 0.0
    assert _same_scene(_read(r), held)
    # deform's own validation leaves the scene as it was
    G = sr.transforms(q)
    dev = torch.from_numpy(G).to(r.device)
    for bad in (dev.double(), dev[:, :, :3].contiguous(), dev.reshape(-1, 12), dev[:0], dev.transpose(1, 2)):
        with pytest.raises(ValueError, match="node_transforms"):
            r.deform(bad)
    sheared = G.copy()
    sheared[0, 0, 1] += 0.1
    for bad in (sheared, G[0], np.zeros((0, 3, 4), np.float32), np.full((2, 3, 4), np.nan, np.float32)):
        with pytest.raises(ValueError, match="node_transforms"):
            r.deform(bad)
    L = _capi.lib()
    for m in (0, 65537, -1):
        assert L.sas_scene_deform(r._ctx, m, dev.data_ptr(), None) == -1 and b"m=" in L.sas_last_error(r._ctx)
    assert L.sas_scene_deform(r._ctx, 70, None, None) == -1
    i32 = torch.zeros((sr.N, 9), dtype=torch.int32, device=r.device)
    f32 = torch.zeros((sr.N, 9), dtype=torch.float32, device=r.device)
    for k in (9, -1):
        assert L.sas_scene_skin(r._ctx, k, i32.data_ptr(), f32.data_ptr(), None) == -1 and b"k=" in L.sas_last_error(r._ctx)
    assert L.sas_scene_skin(r._ctx, 4, None, f32.data_ptr(), None) == -1
    for bad_i, bad_w in ((i32, f32), (i32[:, :0], f32[:, :0]), (i32[:5, :4], f32[:5, :4]), (f32[:, :4], f32[:, :4]), (i32[:, :4], f32[:, :3])):
        with pytest.raises(ValueError):
            r.set_skin(bad_i, bad_w)
    assert _same_scene(_read(r), held) and r.has_skin
    # after clear_skin the refused calls work
    r.clear_skin()
    assert _same_bits(_read(r)["means"], kw["means"])
    with pytest.raises(SasError, match="no skin is bound"):
        r.deform(dev)
    assert _same_bits(_read(r)["means"], kw["means"])
    for name in ("reset_opacity", "mcmc_noise", "adam_step", "mcmc_refine"):   # (mcmc_refine may change N: densify gets a fresh scene)
        refused[name]()
    r.upload(**kw)
    refused["densify"]()
    # upload drops the skin
    r.upload(**kw)
    r.bind_skin(q, k=4)
    assert r.has_skin
    r.upload(**kw)
    assert not r.has_skin
    with pytest.raises(SasError, match="no skin is bound"):
        r.deform(dev)
    r.adam_step(zero, {"means": 1e-3}, 1)   # (no skin: no refusal)


# ---- bind_skin ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,md", (("m70", 4, np.inf), ("m3", 8, np.inf), ("m70", 8, 0.3), ("m1", 4, np.inf)))
def test_bind_skin_is_the_restatement(rasterizer, name, k, md):
    r = rasterizer
    kw, q = sr.scene("quats"), sr.nodes(name)
    r.upload(**kw)
    res = r.bind_skin(q, k=k, max_distance=md)
    d2, idx = sr.knn_cross_ref(kw["means"], q, k, md)
    sigma = sr.default_sigma(q)
    assert res["sigma"] == sigma
    gi, gw = res["indices"].cpu().numpy(), res["weights"].cpu().numpy()
    i64, w64 = sr.weights_ref(d2, idx, sigma, np.float64)
    _, w32 = sr.weights_ref(d2, idx, sigma, np.float32)
    assert np.array_equal(gi, i64) and gw.dtype == np.float32
    e32, e = sr.rel_err(w32, w64), sr.rel_err(gw, w64)
    print(f"  bind_skin {name} k={k}: weights device {e:.3e}, float32 restatement {e32:.3e}")
    assert e <= 4.0 * e32 or (e32 == 0.0 and e == 0.0), (e, e32)
    has = gi[:, 0] >= 0
    assert (gw[has, 0] == 1.0).all() and (gw[gi < 0] == 0.0).all() and np.isfinite(gw).all()
    back = r.read_skin()
    assert np.array_equal(back["indices"].cpu().numpy(), gi) and _same_bits(back["weights"], gw)
    # a given sigma; one so small that every other weight underflows: the nearest stays 1 and no row sums to zero
    tiny = r.bind_skin(q, k=k, sigma=1e-4, max_distance=md)
    tw = tiny["weights"].cpu().numpy()
    assert tiny["sigma"] == 1e-4 and (tw[has, 0] == 1.0).all() and (tw[has].sum(axis=1) >= 1.0).all()
    with pytest.raises(ValueError, match="sigma"):
        r.bind_skin(q, k=k, sigma=0.0)
    with pytest.raises(ValueError, match="group"):
        r.bind_skin(q, k=k, group=2)


def test_bind_skin_group_follows_density_control(rasterizer):
    """The groups bind_skin selects by are those of the scene as it stands: after mcmc_refine every Gaussian has its parent's."""
    r = rasterizer
    kw = sr.scene("quats")
    r.upload(**kw)
    res = r.mcmc_refine(cap_max=900, grow_factor=1.1)
    gid = kw["group_id"][res["parents"].cpu().numpy()]
    idx = r.bind_skin(sr.nodes("m70"), k=4, group=1)["indices"].cpu().numpy()
    assert idx.shape[0] == r.n == res["n"] > sr.N
    assert (idx[gid == 0] == -1).all() and (idx[gid == 1][:, 0] >= 0).all()


def test_door_b_binds_only_its_handle(tmp_path):
    from sim_a_splat_amd import deform
    from sim_a_splat_amd.scene import SplatScene
    rng = np.random.default_rng(95)
    def group(n, centre):
        c = (rng.normal(0.0, 0.2, (n, 3)) + centre).astype(np.float32)
        cov = np.tile(np.eye(3, dtype=np.float32) * 4e-3, (n, 1, 1))
        return c, cov, rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0.5, 0.9, n).astype(np.float32)
    scene = SplatScene(0, background=BG)
    try:
        a = scene.add_gaussian_splats("static", *group(300, (-0.3, 0.0, 0.0)))
        b = scene.add_gaussian_splats("cloth", *group(200, (0.3, 0.0, 0.0)), position=(0.0, 0.1, 0.0))
        with pytest.raises(RuntimeError, match="bind_deformable first"):
            scene.deform(sr.identity_transforms(4))
        nodes = deform.grid_nodes(((0.0, -0.3, -0.3), (0.6, 0.3, 0.3)), 0.3)
        res = scene.bind_deformable(b, nodes, k=4)
        idx, w = res["indices"].cpu().numpy(), res["weights"].cpu().numpy()
        assert idx.shape == (500, 4) and (idx[:300] == -1).all() and (w[:300] == 0).all() and (idx[300:, 0] >= 0).all() and (w[300:, 0] == 1).all()
        cam = dict(wxyz=(0.0, 1.0, 0.0, 0.0), position=(0.0, 0.0, 3.0))
        f0 = scene.get_render(H, W, **cam).copy()
        rest = scene._raster.read_scene()["means"].cpu().numpy()
        moved = nodes.astype(np.float64)
        moved[:, 1] += 0.15 * np.sin(6.0 * moved[:, 0])
        scene.deform(deform.transforms_from_positions(nodes, moved))
        f1 = scene.get_render(H, W, **cam)
        now = scene._raster.read_scene()["means"].cpu().numpy()
        assert f1.shape == (H, W, 3) and f1.dtype == np.uint8 and not np.array_equal(f0, f1)
        assert _same_bits(now[:300], rest[:300]) and np.abs(now[300:] - rest[300:]).max() > 0.02
        with pytest.raises(ValueError, match="handle"):
            scene.bind_deformable(object(), nodes)
        # another handle registered: the scene is uploaded again and the skin bound again with it
        scene.add_gaussian_splats("more", *group(50, (0.0, 0.5, 0.0)))
        scene.deform(sr.identity_transforms(nodes.shape[0]))
        assert scene._raster.has_skin and scene._raster.n == 550
        assert a.index == 0 and b.index == 1
    finally:
        scene.close()


# ---- last: the bounds-checked build ---------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
