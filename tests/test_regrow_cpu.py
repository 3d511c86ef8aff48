"""CPU: the yardstick of tests/test_gpu_z_regrow_sums.py (tests/tools/regrow_cases.py) before it is trusted on the GPU.

1. The six conservation identities hold for the references that exist, each against that reference's own alpha: the float64
   gradients of grad_ref on grad_cases' "blob_32x32" and "dense_48x48" (to 1e-9), and the integer sums of lift_ref / lift_features_ref
   on the C oracle's weights at the size of tests/test_gpu_o_lift.py, within a tolerance derived here from the arithmetic contract.
2. The measure sees the faults the GPU tests are for.  The references are linear in the upstream gradients, the label indicator and
   the mask, so a faulty overflow path is formed from them: (a) the sums taken twice, (b) the sums plus those of the image's upper half
   alone (a truncated first attempt that added its share: the upstream gradients or the mask kept only there; for labels the weights
   themselves, so that ``seen``, which no label gates, takes its share too), (c) one view of two missing.  Every mutant misses the
   conservation bound by a factor of 100 and more; (b) and (c) also differ from the right sums row by row, which is what the
   comparison of the overflowing call with the same call on the grown context sees.

The tolerance of item 1 for the integer sums.  Per pixel p with n(p) composited entries, the contract takes w = alpha T and
T' = T - w in float32: w is the float32 the Gaussian is given, and T' is rounded once, by at most half an ulp of a number below 1:
2^-25.  So |sum_i vis_i(p) - (1 - T_final(p))| <= n(p) 2^-25, and 1 - T_final itself rounds by at most 2^-25 more.  The floor takes
less than one unit 1/ONE from each of the n(p) weights (the quantisation deficit: one-sided, below one unit per composited pair).  Hence

    | sum_i q_i(p) / ONE - A(p) |  <=  tol(p) = n(p) (1/ONE + 2^-25) + 2^-25

and for a channel, with fq = rint(f s) off f s by at most 0.5 plus the float32 product's rounding (32767 2^-24 < 0.01), nothing clamped
at the call's own scale:   | sum_i q_i(p) fq(p) / (ONE s) - A(p) f(p) |  <=  tol(p) |fq(p)| / s + A(p) 0.51 / s.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import grad_cases as gc  # noqa: E402
import grad_ref  # noqa: E402
import lift_features_ref as fr  # noqa: E402
import lift_ref as lr  # noqa: E402
import regrow_cases as kit  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

FACTOR = 100.0          # what every mutant misses BOUND by, at least
LW, LH = 40, 24         # the lift case: a size of tests/test_gpu_o_lift.py


def test_the_case_overflows_a_fresh_buffer_and_its_inputs_are_as_specified():
    """The oracle counts more than 2^20 list entries under every camera used (the group variant included); a truncated attempt would
    hold 2^20 / n_isect of the frame, hundreds of times the bound."""
    for view, groups in ((0, False), (1, False), (0, True)):
        f = kit.frame(view, groups)
        assert f["n_isect"] > kit.FLOOR and f["alpha"].shape == (kit.H, kit.W)
        assert kit.FLOOR / f["n_isect"] > 200 * kit.BOUND
        assert 0 < f["n_visible"] <= kit.N and f["alpha"].mean() > 0.5
    lab = kit.labels()
    assert lab.shape == (5, kit.H, kit.W) and lab.dtype == np.uint8 and set(np.unique(lab)) == set(range(kit.N_LABELS)) | {255}
    assert abs((lab == 255).mean() - 0.1) < 0.01
    img, mask = kit.features()
    assert img.shape == (5, kit.H, kit.W, 3) and img.dtype == np.float32 and abs((mask == 0).mean() - 0.3) < 0.01
    g = kit.upstream()
    assert [a.shape for a in g] == [(kit.H, kit.W, 3), (kit.H, kit.W), (kit.H, kit.W)] and all(0.5 < np.abs(a).mean() < 1.5 for a in g)
    for a in (lab, img, mask) + g:
        assert not a.flags.writeable
    # no right-hand side cancels: sum |x| A / |sum x A| stays below 1.5 for every channel
    A = kit.frame(0)["alpha"]
    for x in (img[0], g[0], g[2][..., None]):
        x = np.asarray(x, np.float64)
        assert (np.einsum("hw,hwc->c", A, np.abs(x)) / np.abs(np.einsum("hw,hwc->c", A, x))).max() < 1.5


# ---- 1. the identities hold for the references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob_32x32", "dense_48x48"])
def test_gradient_sums_are_conserved_by_the_float64_reference(name):
    ref = gc.reference(name)
    g_rgb, _, g_depth = gc.masked_upstream(name)
    A = ref["frame"]["alpha"]
    if name == "dense_48x48":
        assert (1.0 - A <= 2e-4).sum() > 100      # pixels that stopped: entries behind them receive nothing, and A says so
    rhs = kit.grad_rhs(A, g_rgb, g_depth)
    lhs = kit.grad_lhs(ref["screen"]["colors"], ref["screen"]["depths"])
    m = max(kit.miss(lhs[0], rhs[0]), kit.miss(lhs[1], rhs[1]))
    print(f"REGROW cpu {name:12s} d_colors, d_depths against sum g A: miss {m:.3e}")
    assert m <= 1e-9


@functools.lru_cache(maxsize=None)
def _lift_case():
    """The 64-Gaussian scene of tests/test_gpu_o_lift.py under two cameras: per view the oracle's weights [64,H,W], its alpha, n(p)."""
    sc = lr.blob_scene(64, 11, 0.12, n_groups=3)
    cams = [sc_kit.ring(LW, LH, f=0.45 * LW), sc_kit.ring(LW, LH, f=0.45 * LW, yaw=70.0, elev=0.4)]
    views = []
    for cam in cams:
        w = lr.weights_oracle(sc, cam)
        alpha = sc_kit.oracle_frame(sc, cam, (0.0, 0.0, 0.0))["alpha"][..., 0].astype(np.float64)
        views.append(dict(w=w, alpha=alpha, pairs=(w > 0).sum(axis=0)))
    return views


def _tol(pairs, one):
    """tol(p) of the module's docstring."""
    return pairs * (1.0 / one + 2.0 ** -25) + 2.0 ** -25


def test_label_sums_are_conserved_by_the_oracle_weights():
    v = _lift_case()[0]
    lab = kit.labels(2, LH, LW)
    votes, seen = lr.sums(v["w"], lab[0], kit.N_LABELS)
    lhs = kit.label_lhs(votes, seen)
    rhs = kit.label_rhs([v["alpha"]], lab[:1])
    tol = _tol(v["pairs"], kit.LIFT_ONE)
    assert v["pairs"].max() > 8 and abs(lhs[1] - rhs[1]) <= tol.sum()
    for g in range(kit.N_LABELS):
        assert abs(lhs[0][g] - rhs[0][g]) <= tol[lab[0] == g].sum(), g
    # the floor alone is one-sided and below one unit per composited pair
    deficit = v["w"].astype(np.float64).sum() * kit.LIFT_ONE - int(seen.sum())
    assert 0 <= deficit < v["pairs"].sum()
    print(f"REGROW cpu lift_labels   seen miss {kit.miss(lhs[1], rhs[1]):.3e}  votes miss {kit.miss(*[x[0] for x in (lhs, rhs)]):.3e}  "
          f"tolerance {tol.sum() / rhs[1]:.3e} of the sum")
    assert tol.sum() / rhs[1] < 0.01 * kit.BOUND       # what the identity is known to is a hundredth of the bound, at this list length


@pytest.mark.parametrize("masked", [False, True])
def test_feature_sums_are_conserved_by_the_oracle_weights(masked):
    v = _lift_case()[0]
    img, mask = kit.features(2, LH, LW)
    m = mask if masked else None
    scale = fr.auto_scale(img[0])
    sums, weight = fr.sums(v["w"], img[0], scale, None if m is None else m[0])
    lhs = kit.feature_lhs(sums, weight, scale)
    rhs = kit.feature_rhs([v["alpha"]], img[:1], None if m is None else m[:1])
    keep = np.ones((LH, LW)) if m is None else (m[0] != 0)
    tol = _tol(v["pairs"], kit.LIFT_FEATURE_ONE) * keep
    assert abs(lhs[1] - rhs[1]) <= tol.sum()
    fq = np.abs(fr.quantise_features(img[0], scale)).astype(np.float64)
    assert fq.max() == fr.FQ_MAX
    for c in range(kit.CHANNELS):
        t = (tol * fq[..., c] / scale + v["alpha"] * keep * 0.51 / scale).sum()
        assert abs(lhs[0][c] - rhs[0][c]) <= t, c
        assert t / abs(rhs[0][c]) < 0.2 * kit.BOUND        # (worst case, every rounding of fq to one side: 0.51 / s of |f| near 0.6)
    print(f"REGROW cpu lift_features mask={masked!s:5s} weight miss {kit.miss(lhs[1], rhs[1]):.3e}  sums miss {kit.miss(lhs[0], rhs[0]):.3e}")


# ---- 2. the measure sees the faults --------------------------------------------------------------------------------------------------------
def _report(what, figures):
    worst = min(figures)
    print(f"REGROW cpu mutant {what:34s} smallest miss {worst:.3e}  ({worst / kit.BOUND:.0f} x bound)")
    assert worst >= FACTOR * kit.BOUND, (what, figures)


def _rows_differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return int((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1).sum())


def test_label_mutants_miss_the_bound():
    views = _lift_case()
    lab = kit.labels(2, LH, LW)
    per_view = [lr.sums(v["w"], lab[k], kit.N_LABELS) for k, v in enumerate(views)]
    base = per_view[0][0] + per_view[1][0], per_view[0][1] + per_view[1][1]
    rhs = kit.label_rhs([v["alpha"] for v in views], lab)
    right = kit.label_lhs(*base)
    assert max(kit.miss(right[0], rhs[0]), kit.miss(right[1], rhs[1])) < 0.01 * kit.BOUND
    half = lr.sums(kit.upper_half(views[0]["w"], axis=1), lab[0], kit.N_LABELS)   # view 0's upper half alone
    mutants = dict(twice=(2 * base[0], 2 * base[1]), truncated_added=(base[0] + half[0], base[1] + half[1]), view_missing=per_view[0])
    for what, (votes, seen) in mutants.items():
        lhs = kit.label_lhs(votes, seen)
        _report("lift_labels " + what, list(kit.misses(lhs[0], rhs[0])) + [kit.miss(lhs[1], rhs[1])])
        if what != "twice":
            assert _rows_differ(votes, base[0]) > 32 and _rows_differ(seen, base[1]) > 32, what


@pytest.mark.parametrize("masked", [False, True])
def test_feature_mutants_miss_the_bound(masked):
    views = _lift_case()
    img, mask = kit.features(2, LH, LW)
    scale = fr.auto_scale(img)
    m = [mask[k] if masked else None for k in range(2)]
    per_view = [fr.sums(v["w"], img[k], scale, m[k]) for k, v in enumerate(views)]
    base = per_view[0][0] + per_view[1][0], per_view[0][1] + per_view[1][1]
    rhs = kit.feature_rhs([v["alpha"] for v in views], img, mask if masked else None)
    right = kit.feature_lhs(*base, scale)
    assert max(kit.miss(right[0], rhs[0]), kit.miss(right[1], rhs[1])) < 0.1 * kit.BOUND
    half_mask = kit.upper_half(np.ones((LH, LW), np.uint8) if m[0] is None else m[0])   # the mask kept only in the upper half
    half = fr.sums(views[0]["w"], img[0], scale, half_mask)
    mutants = dict(twice=(2 * base[0], 2 * base[1]), truncated_added=(base[0] + half[0], base[1] + half[1]), view_missing=per_view[0])
    for what, (sums, weight) in mutants.items():
        lhs = kit.feature_lhs(sums, weight, scale)
        _report(f"lift_features mask={masked} " + what, list(kit.misses(lhs[0], rhs[0])) + [kit.miss(lhs[1], rhs[1])])
        if what != "twice":
            assert _rows_differ(sums, base[0]) > 32 and _rows_differ(weight, base[1]) > 32, what


def test_gradient_mutants_miss_the_bound():
    """The scene of "blob_32x32" under the kit's upstream gradients (the distribution the GPU test draws, at 32x32)."""
    sc, cam, _ = gc.case("blob_32x32")
    g = kit.upstream(cam[3], cam[2])
    full = grad_ref.gradients(sc, cam, *g, mask_near=False)
    half = grad_ref.gradients(sc, cam, *[kit.upper_half(gi) for gi in g], mask_near=False)
    rhs = kit.grad_rhs(full["frame"]["alpha"], g[0], g[2])
    base = full["screen"]
    right = kit.grad_lhs(base["colors"], base["depths"])
    assert max(kit.miss(right[0], rhs[0]), kit.miss(right[1], rhs[1])) <= 1e-9
    mutants = dict(twice={k: 2 * v for k, v in base.items()}, truncated_added={k: v + half["screen"][k] for k, v in base.items()})
    for what, mut in mutants.items():
        lhs = kit.grad_lhs(mut["colors"], mut["depths"])
        _report("render_backward " + what, list(kit.misses(lhs[0], rhs[0])) + [kit.miss(lhs[1], rhs[1])])
        # ... and every one of the five arrays is far from the right one in the measure of the first-against-second comparison
        _report("render_backward " + what + " rel_err", [grad_ref.rel_err(mut[k], base[k]) for k in grad_ref.SCREEN])
        if what != "twice":
            assert all(_rows_differ(mut[k], base[k]) > 16 for k in grad_ref.SCREEN), what
