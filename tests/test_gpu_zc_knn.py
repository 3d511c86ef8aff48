"""GPU: the k nearest neighbours within a cloud (sas_knn_points; Rasterizer.knn_points; DESIGN.md 3, "Scene from points") against
tests/tools/knn_ref.py, the numpy restatement, and fit.init_scene on the device.  The search is exact and its contract names every bit:
dist2 and index are compared for EQUALITY, under the library's own grid, under forced grids (SAS_KNN_GRID = 1: brute force alone, 2, 7; each
in a child process, because the knob is read when a context is made) and for k = 1, 3, 8."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, fit
from sim_a_splat_amd.rasterizer import SasError

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import knn_ref as kr  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(name, k=3):
    """The restatement's (dist2, index) of a cloud, computed once."""
    if (name, k) not in _REF:
        _REF[(name, k)] = kr.knn_ref(kr.cloud(name), k)
    return _REF[(name, k)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref):
    d, i = ref
    gd, gi = got["dist2"].cpu().numpy(), got["index"].cpu().numpy()
    return gd.dtype == np.float32 and gi.dtype == np.int32 and gd.shape == d.shape and gi.shape == i.shape and \
        np.array_equal(_bits(gd), _bits(d)) and np.array_equal(gi, i)


def _knn(r, name, k=3, **kw):
    return r.knn_points(torch.from_numpy(kr.cloud(name)).to(r.device), k, **kw)


@pytest.mark.parametrize("name", kr.ALL_CLOUDS)
def test_knn_is_the_restatement(rasterizer, name):
    got = _knn(rasterizer, name)
    assert got["dist2"].device == rasterizer.device and tuple(got["dist2"].shape) == (kr.cloud(name).shape[0], 3)
    assert _same(got, _ref(name)), name


@pytest.mark.parametrize("name,k", [("tenfold", 1), ("uniform4099", 8), ("lattice", 8), ("uniform3", 8), ("sphere", 2)])
def test_other_k(rasterizer, name, k):
    assert _same(_knn(rasterizer, name, k), _ref(name, k)), (name, k)


def test_leftover_path_is_taken(rasterizer):
    """Two tight clusters and three points 1e4 away: the three find nothing within the ring limit and finish in the brute-force kernel; the
    clusters' points stop after a ring or two.  The sphere and the cube need no leftover pass at all; identical points have no extent to
    divide, so the whole cloud goes through the brute-force kernel."""
    r = rasterizer
    assert _same(_knn(r, "clusters"), _ref("clusters"))
    st = r.knn_stats()
    assert not st["brute"] and max(st["grid"]) > 1 and 3 <= st["leftover"] < 803, st
    for name in ("sphere", "uniform4099"):
        assert _same(_knn(r, name), _ref(name))
        st = r.knn_stats()
        assert not st["brute"] and max(st["grid"]) > 2 and st["leftover"] < kr.cloud(name).shape[0] // 20, (name, st)
    assert _same(_knn(r, "identical"), _ref("identical"))
    assert r.knn_stats()["brute"]


def test_inputs_streams_and_scratch_reuse(rasterizer):
    r = rasterizer
    # a large call, then small ones on the same scratch; twice in a row
    for name in ("sphere", "sphere", "uniform63", "uniform1", "non_finite", "uniform257"):
        assert _same(_knn(r, name), _ref(name)), name
    # without indices: the same distances
    got = _knn(r, "sphere", indices=False)
    assert set(got) == {"dist2"} and np.array_equal(_bits(got["dist2"].cpu().numpy()), _bits(_ref("sphere")[0]))
    # NumPy arrays and lists are copied; float64 is rounded to float32 first
    p = kr.cloud("uniform257")
    assert _same(r.knn_points(p), _ref("uniform257")) and _same(r.knn_points(p.astype(np.float64).tolist()), _ref("uniform257"))
    # a side stream, and the default stream right behind it with nothing waited for
    side = torch.cuda.Stream(device=r.device)
    d = torch.from_numpy(kr.cloud("tenfold")).to(r.device)
    torch.cuda.synchronize(r.device)
    with torch.cuda.stream(side):
        a = r.knn_points(d)
    b = r.knn_points(d)
    side.synchronize()
    torch.cuda.synchronize(r.device)
    assert _same(a, _ref("tenfold")) and _same(b, _ref("tenfold"))
    empty = r.knn_points(np.zeros((0, 3), np.float32), 5)
    assert tuple(empty["dist2"].shape) == (0, 5) and tuple(empty["index"].shape) == (0, 5) and empty["index"].dtype == torch.int32
    with pytest.raises(ValueError, match="points must be"):
        r.knn_points(p[:, :2])


def test_validation_errors_of_the_c_entry(rasterizer):
    r = rasterizer
    L = _capi.lib()
    p = torch.from_numpy(kr.cloud("uniform64")).to(r.device)
    d = torch.empty((64, 3), dtype=torch.float32, device=r.device)
    call = lambda n, pp, k, dd: L.sas_knn_points(r._ctx, n, pp, k, dd, None, None)
    for k in (0, -1, 9, 1 << 20):
        assert call(64, p.data_ptr(), k, d.data_ptr()) == -1
        assert b"k=" in L.sas_last_error(r._ctx)
    assert call(-1, p.data_ptr(), 3, d.data_ptr()) == -1
    assert call(1 << 31, p.data_ptr(), 3, d.data_ptr()) == -1
    assert call(64, None, 3, d.data_ptr()) == -1 and call(64, p.data_ptr(), 3, None) == -1
    assert call(0, None, 3, None) == 0                     # an empty cloud needs no arrays
    assert L.sas_knn_points(None, 64, p.data_ptr(), 3, d.data_ptr(), None, None) == -1
    for k in (0, 9):
        with pytest.raises(SasError, match="status -1"):
            r.knn_points(p, k)
    assert call(64, p.data_ptr(), 3, d.data_ptr()) == 0    # (and the context serves the next call)
    torch.cuda.synchronize(r.device)
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(_ref("uniform64")[0]))


@pytest.mark.parametrize("g", (1, 2, 7))
def test_forced_grids_give_the_same_bits(rasterizer, tmp_path, g):
    out = tmp_path / f"knn_g{g}.npz"
    env = dict(os.environ, SAS_KNN_GRID=str(g))
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "tools" / "knn_child.py"), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "knn child ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
    bad = []
    with np.load(out) as z:
        for name in kr.ALL_CLOUDS:
            default = _knn(rasterizer, name)
            if not (_same(default, (z[f"{name}_dist2"], z[f"{name}_index"])) and _same(default, _ref(name))):
                bad.append(name)
            left, nx, ny, nz, brute = (int(v) for v in z[f"{name}_stats"])
            n = kr.cloud(name).shape[0]
            if n == 0:
                continue
            if g == 1:
                assert brute and left == 0, (name, left, brute)
            else:
                assert max(nx, ny, nz) <= g and (brute or max(nx, ny, nz) > 1), (name, nx, ny, nz)
        if g == 7:   # the forced path is the grid search, not the brute-force kernel, where the cloud has an extent
            assert tuple(int(v) for v in z["sphere_stats"][1:]) == (7, 7, 7, 0) and tuple(int(v) for v in z["planar_stats"][1:]) == (7, 1, 7, 0)
    assert not bad, bad


def test_init_scene_on_the_device(rasterizer):
    """The uploaded scene, read back, is the CPU formulas (tests/tools/knn_ref.py: init_formulas) applied to the restatement's distances:
    the same bits for means, opacities, colours and quaternions; the scales within 1 ulp (the device's sqrt).  A frame of it renders."""
    r = rasterizer
    p = kr.cloud("sphere")
    c8 = np.random.default_rng(21).integers(0, 256, p.shape).astype(np.uint8)
    got = fit.init_scene(r, torch.from_numpy(p).to(r.device), torch.from_numpy(c8).to(r.device), sh_degree=2, init_opacity=0.3, init_scale=0.8)
    want = kr.init_formulas(p, _ref("sphere")[0], c8, 2, 0.3, 0.8)
    back = r.read_scene()
    assert r.n == p.shape[0] and r.sh_degree == 2
    for k, w in want.items():
        for src in (got[k], back[k]):
            g = src.cpu().numpy()
            assert g.shape == w.shape and g.dtype == np.float32, k
            if k == "scales":
                assert np.abs(_bits(g).astype(np.int64) - _bits(w).astype(np.int64)).max() <= 1
            else:
                assert np.array_equal(_bits(g), _bits(w)), k
    V, K, W, H = sc_kit.ring(96, 64, f=60.0, yaw=20.0, elev=0.1)
    frame = sc_kit.to_numpy(r.render(V, K, W, H, (0.0, 0.0, 0.0)))
    assert np.isfinite(frame["rgb"]).all() and frame["rgb"].shape == (H, W, 3)
    # host arrays, float colours and grey: the same scene but for the colours
    again = fit.init_scene(r, p, c8.astype(np.float32) / np.float32(255.0), sh_degree=2, init_opacity=0.3, init_scale=0.8)
    assert all(torch.equal(again[k], got[k]) for k in got)
    grey = fit.init_scene(r, p, sh_degree=0)
    assert not grey["colors"].any() and tuple(r.read_scene()["colors"].shape) == (p.shape[0], 1, 3)
    with pytest.raises(ValueError, match="non-finite"):
        fit.init_scene(r, kr.cloud("non_finite"))
    with pytest.raises(ValueError, match="at least 4"):
        fit.init_scene(r, p[:3])


# ---- last: the bounds-checked build -------------------------------------------------------------------------------------------------------
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
