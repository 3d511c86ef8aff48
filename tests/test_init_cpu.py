"""CPU: fit.init_scene with the numpy restatement of sas_knn_points in the kernel's place and a recording stand-in for the rasterizer; the
restatement (tests/tools/knn_ref.py) against a float64 brute force and on the tie rule; the export of the C entry.
tests/test_gpu_zc_knn.py holds the library to the restatement, bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, fit

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import knn_ref as kr  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


class Recorder:
    """What init_scene needs of a Rasterizer: ``upload``; it keeps what it was given."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def upload(self, means, opacities, colors, *, quats=None, scales=None, covariances=None, sh_degree=3, group_id=None, n_groups=0):
        self.calls.append(dict(means=means, opacities=opacities, colors=colors, quats=quats, scales=scales, covariances=covariances,
                               sh_degree=sh_degree, group_id=group_id, n_groups=n_groups))


def _knn(points, k):
    return kr.knn_ref(points, k, indices=False)


def _cloud(n=500, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.mark.parametrize("sh_degree,colored", [(3, True), (0, True), (2, False)])
def test_init_scene_uploads_the_formulas(sh_degree, colored):
    p, c8 = _cloud()
    r = Recorder()
    gid = (np.arange(p.shape[0]) % 3).astype(np.uint8)
    got = fit.init_scene(r, p, c8 if colored else None, sh_degree=sh_degree, init_opacity=0.25, init_scale=0.5, min_dist2=1e-6, group_id=gid,
                         n_groups=3, knn=_knn)
    want = kr.init_formulas(p, _knn(p, 3), c8 if colored else None, sh_degree, 0.25, 0.5, 1e-6)
    assert len(r.calls) == 1
    call = r.calls[0]
    assert call["sh_degree"] == sh_degree and call["n_groups"] == 3 and call["group_id"] is gid and call["covariances"] is None
    assert set(got) == set(want)
    for k, w in want.items():
        assert got[k] is call[k]                                   # what is returned is what was uploaded
        g = got[k].numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, k
        if k == "scales":   # torch's vectorised sqrt is not the correctly rounded one everywhere: within 1 ulp (positive floats: their bits are ordered)
            assert np.abs(_bits(g).astype(np.int64) - _bits(w).astype(np.int64)).max() <= 1
            assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], g[:, 2])
        else:
            assert np.array_equal(_bits(g), _bits(w)), k
    assert got["colors"].shape == (p.shape[0], (sh_degree + 1) ** 2, 3) and not got["colors"][:, 1:].any()
    if not colored:
        assert not got["colors"].any()                             # grey 0.5 is a zero DC term
    assert torch.equal(got["quats"], torch.tensor([1.0, 0, 0, 0]).expand(p.shape[0], 4))
    # the scale really is the RMS distance to the three nearest other points, in float64 within rounding
    d64, _ = kr.knn_f64(p, 3)
    assert np.allclose(got["scales"][:, 0].numpy(), 0.5 * np.sqrt(np.maximum(d64.mean(axis=1), 1e-6)), rtol=1e-5, atol=0)


def test_min_dist2_clamps_duplicates():
    p = np.repeat(_cloud(40)[0], 5, axis=0)     # every point five times: the three nearest others are at distance 0
    got = fit.init_scene(Recorder(), p, knn=_knn, min_dist2=1e-7, init_scale=2.0)
    want = _bits(np.full((200, 3), np.float32(2.0) * np.sqrt(np.float32(1e-7)))).astype(np.int64)
    assert np.abs(_bits(got["scales"].numpy()).astype(np.int64) - want).max() <= 1   # (sqrt: within 1 ulp)
    got = fit.init_scene(Recorder(), p, knn=_knn, min_dist2=0.0)
    assert not got["scales"].any()


def test_uint8_and_float_colours_give_the_same_dc():
    p, c8 = _cloud(64)
    a = fit.init_scene(Recorder(), p, c8, knn=_knn)["colors"]
    b = fit.init_scene(Recorder(), p, c8.astype(np.float32) / np.float32(255.0), knn=_knn)["colors"]
    c = fit.init_scene(Recorder(), torch.from_numpy(p), torch.from_numpy(c8), knn=_knn)["colors"]
    assert torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(_bits(a[:, 0].numpy()), _bits((c8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(fit.SH_C0)))


def test_refusals():
    p, c8 = _cloud(16)
    r = Recorder()
    with pytest.raises(ValueError, match="at least 4"):
        fit.init_scene(r, p[:3], knn=_knn)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        fit.init_scene(r, p[:, :2], knn=_knn)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[7, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            fit.init_scene(r, q, knn=_knn)
    with pytest.raises(ValueError, match="colors must be"):
        fit.init_scene(r, p, c8[:-1], knn=_knn)
    with pytest.raises(ValueError, match="colors must be"):
        fit.init_scene(r, p, c8[:, :2], knn=_knn)
    f = c8.astype(np.float32) / 255.0
    for bad in (1.5, -0.01, np.nan):
        g = f.copy()
        g[3, 2] = bad
        with pytest.raises(ValueError, match="outside 0..1"):
            fit.init_scene(r, p, g, knn=_knn)
    with pytest.raises(ValueError, match="sh_degree"):
        fit.init_scene(r, p, knn=_knn, sh_degree=-1)
    with pytest.raises(ValueError, match="knn returned"):
        fit.init_scene(r, p, knn=lambda pts, k: np.zeros((pts.shape[0], 2), np.float32))
    assert not r.calls                                              # nothing was uploaded by a refused call
    fit.init_scene(r, p[:4], knn=_knn)                              # four points are enough
    assert len(r.calls) == 1


@pytest.mark.parametrize("k", (1, 3, 8))
def test_restatement_against_float64_brute_force(k):
    """Drawn clouds have no near-ties at float32 resolution (checked), so the float32 keys order as the float64 distances do: the same
    indices, and distances within the float32 rounding of the restatement: a difference is off by u = 2^-24 (relative), its square by
    3 u with the product's own rounding, each of the two sums adds u: 5 u, taken as 5.1 u for the second-order terms."""
    for name in ("uniform257", "uniform4099", "sphere", "planar"):
        p = kr.cloud(name)
        d64, i64 = kr.knn_f64(p, k + 1)
        gap = (d64[:, 1:] - d64[:, :-1]) / d64[:, 1:]
        clear = gap.min(axis=1) > 1e-5                              # rows whose first k + 1 distances are well apart
        assert clear.mean() > 0.95, name
        d32, i32 = kr.knn_ref(p, k)
        assert d32.dtype == np.float32 and i32.dtype == np.int32
        assert np.array_equal(i32[clear], i64[clear, :k]), name
        assert np.all(np.abs(d32[clear].astype(np.float64) - d64[clear, :k]) <= 5.1 * 2.0 ** -24 * d64[clear, :k]), name
        assert np.all(d32[:, 1:] >= d32[:, :-1])


def test_restatement_tie_rule_on_a_lattice():
    """On the 9 x 9 x 9 integer lattice every distance is an exact small integer and most are tied: among equal distances the lower index
    wins, and the keys ascend."""
    p = kr.lattice()
    d, i = kr.knn_ref(p, 8)
    n = p.shape[0]
    exact = ((p[None].astype(np.int64) - p[:, None].astype(np.int64)) ** 2).sum(axis=2)
    np.fill_diagonal(exact, 10 ** 9)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), exact), axis=1)[:, :8]   # by (distance, index)
    assert np.array_equal(i, order.astype(np.int32))
    assert np.array_equal(d, np.take_along_axis(exact, order, axis=1).astype(np.float32))
    assert (d[:, 0] == 1).all() and (np.diff(d, axis=1) == 0).any()


def test_restatement_edge_cases():
    d, i = kr.knn_ref(np.zeros((0, 3), np.float32), 3)
    assert d.shape == (0, 3) and i.shape == (0, 3)
    d, i = kr.knn_ref(np.ones((1, 3), np.float32), 3)
    assert np.isinf(d).all() and (i == -1).all()
    d, i = kr.knn_ref(kr.uniform_cube(3), 3)
    assert np.isfinite(d[:, :2]).all() and np.isinf(d[:, 2]).all() and (i[:, 2] == -1).all() and (i[:, :2] >= 0).all()
    d, i = kr.knn_ref(kr.identical(), 3)                           # duplicates are neighbours at 0, the lowest other indices
    assert not d.any() and np.array_equal(i[0], [1, 2, 3]) and np.array_equal(i[1], [0, 2, 3]) and np.array_equal(i[5], [0, 1, 2])
    p = kr.non_finite()
    d, i = kr.knn_ref(p, 3)
    bad = ~np.isfinite(p).all(axis=1)
    assert np.isinf(d[bad]).all() and (i[bad] == -1).all()          # a non-finite point has no neighbours ...
    assert not np.isin(i, np.flatnonzero(bad)).any()                # ... and is nobody's
    assert np.isinf(d[400]).all() and np.isinf(d[401]).all()        # 1e30: every d2 overflows
    assert not np.isin(i, [400, 401]).any()
    ok = np.isfinite(p).all(axis=1) & (np.abs(p).max(axis=1) < 2)
    assert np.isfinite(d[ok]).all()
    # chunking does not reach the result
    a = kr.knn_ref(kr.uniform_cube(257), 3, chunk=1024)
    b = kr.knn_ref(kr.uniform_cube(257), 3, chunk=100)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_knn_entry_is_declared_and_exported():
    header = (ROOT / "include" / "sim_a_splat_amd.h").read_text()
    for name in ("sas_knn_points", "sas_knn_last_counts"):
        assert name in _capi.EXPORTS and f"int {name}(sas_ctx *ctx" in header
    internal = (ROOT / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()
    assert f"#define SAS_KNN_MAX_K {_capi.SAS_KNN_MAX_K}\n" in internal
    assert f"#define SAS_KNN_RING_LIMIT {_capi.SAS_KNN_RING_LIMIT} " in internal
    from sim_a_splat_amd import build
    assert build.CSRC / "sas_knn.hip" in build.SOURCES
