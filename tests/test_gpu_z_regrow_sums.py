"""GPU: frames that ADD into the caller's buffers, on lists that outgrow a fresh context's key buffer (lift_labels, lift_features,
render_backward in its three forms, density_accumulate behind it).  Such a frame is rendered twice (complete_oldest); DESIGN.md 3
promises that its first, truncated rendering adds nothing.  Every stored-frame overflow test would pass if it added its share.

The case, the inputs and the yardstick are tests/tools/regrow_cases.py's (tests/test_regrow_cpu.py holds them on the CPU): the
30 000-Gaussian scene under two 640x480 cameras, of which the C oracle counts 3.03 M list entries each against a buffer of 2^20 keys.

Held, per call, on a context of its own (fresh buffers):
  - the overflow happened: stats()["regrows"] rose on the first call, and not on the same call made again;
  - conservation against the oracle's alpha (regrow_cases' six identities), miss <= BOUND = 1e-3;
  - the first call against the second, which ran on grown buffers -- the path the small tests hold to their references: integer
    outputs torch.equal per Gaussian, float outputs grad_ref.rel_err <= BOUND;
  - the call adds: into the first call's buffers it leaves exactly twice the sums.
A truncated attempt that added would hold 2^20 / n_isect = 0.35 of a frame, a second addition all of it (test_regrow_cpu.py's mutants).

Every figure is printed (REGROW lines) before it is held; an MI355X run is in profiles/regrow_sums.txt: conservation 3e-9 for label
lifting, 1.6e-6 for feature lifting (what the floor takes at its 2^24 unit, below one unit per composited pair), 1e-8 for the
backward pass; first against second call at most 6e-7.  Nothing is near 1e-4."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd.rasterizer import Rasterizer

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import grad_ref  # noqa: E402
import regrow_cases as kit  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, G = kit.W, kit.H, kit.N_LABELS
N_SLOTS = 4   # the frame slots of a context (test_gpu_parity.py, test_stream_ordered_consumer_of_overflowing_async_frames)


def _context(groups=False):
    r = Rasterizer("cuda:0")
    sc_kit.upload(r, kit.scene(groups))
    return r


def _alphas(views, groups=False):
    """The oracle's alpha per view, after asserting that every one of these frames outgrows a fresh buffer."""
    for v in set(views):
        assert kit.frame(v, groups)["n_isect"] > kit.FLOOR, (v, kit.frame(v, groups)["n_isect"])
    return [kit.frame(v, groups)["alpha"] for v in views]


def _first(r, call):
    """``call()`` on the fresh context ``r``: its result and the regrow count it left, which must have risen."""
    before = r.stats()["regrows"]
    out = call()
    grown = r.stats()["regrows"]
    assert grown >= before + 1, (before, grown)
    return out, grown


class _Figures:
    """Print every figure in the style of the BACKWARD lines, then hold each to the bound."""

    def __init__(self, what):
        self.what, self.rows = what, []

    def add(self, key, figure):
        self.rows.append((key, float(figure)))
        print(f"REGROW {self.what:34s} {key:26s} hip {float(figure):.3e}  bound {kit.BOUND:.1e}  {'ok' if figure <= kit.BOUND else 'MISS'}")

    def conservation(self, key, lhs, rhs):
        for k, m in enumerate(kit.misses(lhs, rhs)):
            self.add(f"{key}[{k}] conservation" if np.ndim(lhs) else f"{key} conservation", m)

    def check(self):
        bad = [(k, e) for k, e in self.rows if not e <= kit.BOUND]
        assert not bad, (self.what, bad)


def _np(d):
    return {k: v.double().cpu().numpy() for k, v in d.items()}


def _dev(a):
    """A device copy of one of the kit's (read-only) arrays; None stays None."""
    return None if a is None else torch.from_numpy(np.array(a)).to("cuda:0")


# ---- lift_labels ---------------------------------------------------------------------------------------------------------------------------
def test_lift_labels_one_view():
    alphas = _alphas((0,))
    Vs, Ks = kit.cameras((0,))
    lab = kit.labels()[:1]
    dl = _dev(lab)
    r = _context()
    try:
        a, grown = _first(r, lambda: r.lift_labels(Vs, Ks, W, H, dl, G))
        st = r.stats()
        assert st["n_isect"] == kit.frame(0)["n_isect"] <= st["capacity"]
        fig = _Figures("lift_labels 1 view")
        lhs, rhs = kit.label_lhs(a["votes"].cpu().numpy(), a["seen"].cpu().numpy()), kit.label_rhs(alphas, lab)
        fig.conservation("votes", lhs[0], rhs[0])
        fig.conservation("seen", lhs[1], rhs[1])
        b = r.lift_labels(Vs, Ks, W, H, dl, G)                                     # zeroed buffers, grown context
        assert r.stats()["regrows"] == grown
        assert torch.equal(a["votes"], b["votes"]) and torch.equal(a["seen"], b["seen"])
        c = r.lift_labels(Vs, Ks, W, H, dl, G, votes=a["votes"], seen=a["seen"])   # the call adds: twice the first
        assert c["votes"].data_ptr() == a["votes"].data_ptr() and r.stats()["regrows"] == grown
        assert torch.equal(c["votes"], 2 * b["votes"]) and torch.equal(c["seen"], 2 * b["seen"]) and int(b["seen"].max()) > kit.LIFT_ONE
        fig.check()
    finally:
        r.close()


def test_lift_labels_five_views_in_one_call():
    """Every slot overflows on first use while the others are in flight; the fifth view lands on a grown slot."""
    alphas = _alphas(kit.VIEWS5)
    Vs, Ks = kit.cameras(kit.VIEWS5)
    lab = kit.labels()
    dl = _dev(lab)
    r = _context()
    try:
        a, grown = _first(r, lambda: r.lift_labels(Vs, Ks, W, H, dl, G))
        assert grown >= N_SLOTS, grown
        fig = _Figures("lift_labels 5 views")
        lhs, rhs = kit.label_lhs(a["votes"].cpu().numpy(), a["seen"].cpu().numpy()), kit.label_rhs(alphas, lab)   # 3 A_0 + 2 A_90
        fig.conservation("votes", lhs[0], rhs[0])
        fig.conservation("seen", lhs[1], rhs[1])
        singles = [r.lift_labels(Vs[k:k + 1], Ks[k:k + 1], W, H, dl[k:k + 1], G) for k in range(5)]
        assert r.stats()["regrows"] == grown
        assert torch.equal(a["votes"], sum(s["votes"] for s in singles)) and torch.equal(a["seen"], sum(s["seen"] for s in singles))
        assert not torch.equal(singles[0]["seen"], singles[1]["seen"]) and not torch.equal(singles[0]["votes"], singles[2]["votes"])
        fig.check()
    finally:
        r.close()


# ---- lift_features -------------------------------------------------------------------------------------------------------------------------
def _feature_figures(fig, got, alphas, img, mask):
    lhs = kit.feature_lhs(got["sums"].cpu().numpy(), got["weight"].cpu().numpy(), got["feature_scale"])
    rhs = kit.feature_rhs(alphas, img, mask)
    fig.conservation("sums", lhs[0], rhs[0])
    fig.conservation("weight", lhs[1], rhs[1])


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
def test_lift_features_one_view(masked):
    alphas = _alphas((0,))
    Vs, Ks = kit.cameras((0,))
    img, mask = kit.features()
    img, mask = img[:1], mask[:1] if masked else None
    di, dm = _dev(img), _dev(mask)
    r = _context()
    try:
        a, grown = _first(r, lambda: r.lift_features(Vs, Ks, W, H, di, mask=dm))
        scale = a["feature_scale"]
        fig = _Figures(f"lift_features 1 view mask={masked}")
        _feature_figures(fig, a, alphas, img, mask)
        b = r.lift_features(Vs, Ks, W, H, di, mask=dm, feature_scale=scale)
        assert r.stats()["regrows"] == grown and b["feature_scale"] == scale
        assert torch.equal(a["sums"], b["sums"]) and torch.equal(a["weight"], b["weight"])
        c = r.lift_features(Vs, Ks, W, H, di, mask=dm, feature_scale=scale, sums=a["sums"], weight=a["weight"])
        assert c["sums"].data_ptr() == a["sums"].data_ptr() and r.stats()["regrows"] == grown
        assert torch.equal(c["sums"], 2 * b["sums"]) and torch.equal(c["weight"], 2 * b["weight"]) and int(b["weight"].max()) > kit.LIFT_FEATURE_ONE
        fig.check()
    finally:
        r.close()


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
def test_lift_features_five_views_in_one_call(masked):
    alphas = _alphas(kit.VIEWS5)
    Vs, Ks = kit.cameras(kit.VIEWS5)
    img, mask = kit.features()
    mask = mask if masked else None
    di, dm = _dev(img), _dev(mask)
    m = lambda k: None if dm is None else dm[k:k + 1]
    r = _context()
    try:
        a, grown = _first(r, lambda: r.lift_features(Vs, Ks, W, H, di, mask=dm))
        assert grown >= N_SLOTS, grown
        scale = a["feature_scale"]
        fig = _Figures(f"lift_features 5 views mask={masked}")
        _feature_figures(fig, a, alphas, img, mask)
        singles = [r.lift_features(Vs[k:k + 1], Ks[k:k + 1], W, H, di[k:k + 1], mask=m(k), feature_scale=scale) for k in range(5)]
        assert r.stats()["regrows"] == grown
        assert torch.equal(a["sums"], sum(s["sums"] for s in singles)) and torch.equal(a["weight"], sum(s["weight"] for s in singles))
        assert not torch.equal(singles[0]["weight"], singles[1]["weight"]) and not torch.equal(singles[0]["sums"], singles[2]["sums"])
        fig.check()
    finally:
        r.close()


# ---- render_backward -----------------------------------------------------------------------------------------------------------------------
def _agree(fig, first, second, tag="first/second"):
    a, b = _np(first), _np(second)
    assert set(a) == set(b)
    for k in b:
        assert np.abs(b[k]).max() > 0, k
        fig.add(f"{k} {tag}", grad_ref.rel_err(a[k], b[k]))


def test_render_backward_screen():
    alphas = _alphas((0,))
    V, K, _, _ = kit.camera(0)
    g = kit.upstream()
    dg = [_dev(gi) for gi in g]
    r = _context()
    try:
        a, grown = _first(r, lambda: r.render_backward(V, K, W, H, *dg, screen_space=True))
        assert set(a) == set(grad_ref.SCREEN)
        fig = _Figures("render_backward screen")
        lhs, rhs = kit.grad_lhs(a["colors"].cpu().numpy(), a["depths"].cpu().numpy()), kit.grad_rhs(alphas[0], g[0], g[2])
        fig.conservation("d_colors", lhs[0], rhs[0])
        fig.conservation("d_depths", lhs[1], rhs[1])
        b = r.render_backward(V, K, W, H, *dg, screen_space=True)
        assert r.stats()["regrows"] == grown
        _agree(fig, a, b)
        fig.check()
    finally:
        r.close()


def test_render_backward_full():
    _alphas((0,))
    V, K, _, _ = kit.camera(0)
    g = kit.upstream()
    dg = [_dev(gi) for gi in g]
    r = _context()
    try:
        a, grown = _first(r, lambda: r.render_backward(V, K, W, H, *dg))
        assert set(a) == {"means", "opacities", "colors", "viewmat", "quats", "scales"}        # every output of the scene's form
        b = r.render_backward(V, K, W, H, *dg)
        assert r.stats()["regrows"] == grown
        fig = _Figures("render_backward full")
        _agree(fig, a, b)
        fig.check()
    finally:
        r.close()


def test_render_backward_pose_groups():
    _alphas((0,), groups=True)
    V, K, _, _ = kit.camera(0)
    g = kit.upstream()
    dg = [_dev(gi) for gi in g]
    groups = tuple(range(kit.N_GROUPS))
    r = _context(groups=True)
    try:
        a, grown = _first(r, lambda: r.render_backward(V, K, W, H, *dg, pose_groups=groups))
        assert set(a) == {"means", "opacities", "colors", "viewmat", "quats", "scales", "group_poses"}
        assert r.stats()["n_isect"] == kit.frame(0, True)["n_isect"]
        b = r.render_backward(V, K, W, H, *dg, pose_groups=groups)
        assert r.stats()["regrows"] == grown
        fig = _Figures("render_backward pose_groups")
        _agree(fig, a, b)
        fig.check()
    finally:
        r.close()


def test_render_backward_out_carries_the_overflowed_view_into_the_next():
    """``out=``: view 0 overflows the fresh buffers, view 1 adds to its result on the grown ones; then both again, nothing overflowing."""
    _alphas((0, 1))
    cams = [kit.camera(0), kit.camera(1)]
    g = kit.upstream()
    dg = [_dev(gi) for gi in g]
    r = _context()
    try:
        first, grown = _first(r, lambda: r.render_backward(cams[0][0], cams[0][1], W, H, *dg))
        alone = {k: v.clone() for k, v in first.items()}
        a = r.render_backward(cams[1][0], cams[1][1], W, H, *dg, out=first)
        assert r.stats()["regrows"] == grown and a["means"].data_ptr() == first["means"].data_ptr()
        b = None
        for V, K, _, _ in cams:
            b = r.render_backward(V, K, W, H, *dg, out=b)
        assert r.stats()["regrows"] == grown
        fig = _Figures("render_backward out= two views")
        _agree(fig, a, b)
        fig.check()
        assert all(grad_ref.rel_err(alone[k].double().cpu().numpy(), _np(b)[k]) > 100 * kit.BOUND for k in b)   # view 1 did add
    finally:
        r.close()


def test_density_accumulate_behind_the_overflowed_backward():
    """The sums the overflowed backward left in the context, read without ``d_means2d``: the Gaussians of ONE rendering."""
    _alphas((0,))
    V, K, _, _ = kit.camera(0)
    g = kit.upstream()
    dg = [_dev(gi) for gi in g]
    r = _context()
    try:
        first, second = r.new_density_stats(), r.new_density_stats()
        _, grown = _first(r, lambda: r.render_backward(V, K, W, H, *dg, want=("means",)))
        r.density_accumulate(W, H, first)
        radii = r.read_projection()["radii"]
        r.render_backward(V, K, W, H, *dg, want=("means",))
        r.density_accumulate(W, H, second)
        assert r.stats()["regrows"] == grown
        vis = radii[:, 0] > 0
        count = first["count"].cpu().numpy()
        assert np.array_equal(count, vis.astype(np.int32)) and int(count.sum()) == kit.frame(0)["n_visible"] and int(count.max()) == 1
        assert np.array_equal(first["max_radius"].cpu().numpy(), np.where(vis, radii.max(axis=1), 0).astype(np.float32))
        assert torch.equal(first["count"], second["count"]) and torch.equal(first["max_radius"], second["max_radius"])
        fig = _Figures("density_accumulate")
        _agree(fig, dict(grad_sum=first["grad_sum"]), dict(grad_sum=second["grad_sum"]))
        fig.check()
    finally:
        r.close()
