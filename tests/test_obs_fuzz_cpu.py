"""CPU: the observation fuzzer's draw and references (tests/tools/obs_fuzz.py), and that the seeds the GPU suite runs
(OBS_SEEDS, tests/test_gpu_q_obs_fuzz.py) cannot hide a failure: from the references alone, every arm's cases reach the edges they
are there for, and compare() reports every kind of single-value damage.  Nothing here touches a GPU."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import obs_fuzz as of  # noqa: E402


@functools.lru_cache(maxsize=None)
def _case(seed):
    """(case, reference): computed once, shared, never modified."""
    c = of.draw_case(seed)
    return c, of.reference(c)


def _cases(arm):
    return [_case(s) for s in of.OBS_SEEDS[arm]]


def _bytes(o):
    if isinstance(o, np.ndarray):
        return o.tobytes()
    if isinstance(o, dict):
        return b"".join(k.encode() + _bytes(v) for k, v in sorted(o.items()))
    if isinstance(o, (list, tuple)):
        return b"".join(_bytes(v) for v in o)
    if hasattr(o, "__dataclass_fields__"):
        return b"".join(_bytes(getattr(o, k)) for k in o.__dataclass_fields__)
    return repr(o).encode()


def test_the_draw_is_deterministic():
    for seed in (0, 7, 73, 181):
        assert _bytes(of.draw_case(seed)) == _bytes(of.draw_case(seed))
        assert _bytes(of.draw_case(seed, True)) == _bytes(of.draw_case(seed, True))
    assert _bytes(of.draw_case(0)) != _bytes(of.draw_case(1))
    c, ref = _case(4)
    assert _bytes(of.reference(of.draw_case(4))["want"]) == _bytes(ref["want"])


def test_seed_tuples_reach_every_kind_of_case():
    assert set(of.OBS_SEEDS) == set(of.ARMS)
    for arm, seeds in of.OBS_SEEDS.items():
        assert len(seeds) >= 10 and len(set(seeds)) == len(seeds)
        assert all(of.draw_case(s)["arm"] == arm for s in seeds), arm
    for arm in ("labels", "lift", "cloud"):
        cs = [c for c, _ in _cases(arm)]
        assert any(c["poisoned"] for c in cs) and any(c["strip"] for c in cs) and any(c["odd"] for c in cs), arm
        assert all(c["scene"].means.shape[0] in of.SIZES and c["n_groups"] in of.GROUPS and 1 <= len(c["cams"]) <= 3 for c in cs)
        assert all(max(c["W"], c["H"]) <= 3000 and (c["strip"] and min(c["W"], c["H"]) <= 16 or max(c["W"], c["H"]) <= 200) for c in cs)
    assert any(c["n_groups"] >= 9 for c, _ in _cases("labels"))
    assert all(c["scene"].means.shape[0] <= of.lift_ref.ORACLE_MAX for c, _ in _cases("lift"))


def test_labels_cases():
    cs = _cases("labels")
    several = sum(ref["notes"]["distinct_labels"] >= 2 for _, ref in cs)
    print(f"labels: {several} of {len(cs)} cases show at least 2 labels")
    assert several >= 0.6 * len(cs)
    # min_alpha = 0 over pixels nothing reaches: all weights zero, the tie goes to label 0 and the alpha rule does not hide it
    zero_ties = 0
    for c, ref in cs:
        if c["par"]["min_alpha"] == 0.0 and max(ref["notes"]["untouched"]) > 0:
            zero_ties += 1
            assert not any((v == 255).any() for k, v in ref["want"].items() if k.endswith("labels"))
    assert zero_ties >= 2
    assert any(c["par"]["min_alpha"] == 1.0 for c, _ in cs)
    assert any(c["par"]["pose_set"] is not None and len(set(c["par"]["pose_set"])) > 1 for c, _ in cs)


def test_lift_cases():
    cs = _cases("lift")
    assert all((ref["want"]["seen"] > 0).any() for _, ref in cs)
    assert sum(int((ref["want"]["votes"].sum(axis=0) > 0).sum()) >= 2 for _, ref in cs) >= 0.5 * len(cs)
    assert any(c["par"]["n_labels"] == 256 and ref["notes"]["has_255"] and ref["want"]["votes"][:, 255].any() for c, ref in cs)
    assert any((ref["want"]["seen"] == 0).any() for _, ref in cs)
    assert any(c["par"]["again"] is not None for c, _ in cs)
    assert {k for c, _ in cs for k, _ in c["par"]["images"]} == {"uniform", "blocks", "frame"}
    for _, ref in cs:
        assert (ref["want"]["votes"].sum(axis=1) <= ref["want"]["seen"]).all()


def test_cloud_cases():
    from sim_a_splat_amd.rasterizer import CLOUD_RESIDENT
    cs = _cases("cloud")
    count = lambda ref: [int(m) for m in ref["want"]["cloud.count"]]
    assert all(count(ref) == ref["notes"]["M"] for _, ref in cs)
    assert any(0 in count(ref) for _, ref in cs)
    assert any(any(0 < m < c["par"]["K"] for m in count(ref)) for c, ref in cs)
    assert sum(any(m > c["par"]["K"] for m in count(ref)) for c, ref in cs) >= 3
    assert any(max(count(ref)) > CLOUD_RESIDENT for _, ref in cs)
    assert any(ref["notes"]["M_no_grid"] is not None and sum(ref["notes"]["M"]) < sum(ref["notes"]["M_no_grid"]) for _, ref in cs)
    assert any(ref["args"]["bounds"] is not None and sum(ref["notes"]["M_no_grid"] or ref["notes"]["M"]) < sum(ref["notes"]["M_free"]) for _, ref in cs)
    assert any(c["par"]["per_view"] for c, _ in cs) and any(c["par"]["keep"] is not None for c, _ in cs)
    assert {c["par"]["frame_kind"] for c, _ in cs} == {"none", "rigid", "affine"}
    for c, ref in cs:                                     # the padding rows of the reference are what the contract says
        for e, m in enumerate(count(ref)):
            k = min(m, c["par"]["K"])
            assert (ref["want"]["cloud.index"][e, k:] == -1).all() and (ref["want"]["cloud.index"][e, :k] >= 0).all()


def _flip(want, key, how):
    got = {k: np.array(v, copy=True) for k, v in want.items()}
    how(got[key])
    return got


def test_compare_reports_single_value_damage():
    lab_c, lab = _case(of.OBS_SEEDS["labels"][0])
    lift = _case(of.OBS_SEEDS["lift"][2])[1]
    cloud = _case(4)[1]
    rgbd = _case(of.OBS_SEEDS["rgbd"][4])[1]
    for ref in (lab, lift, cloud, rgbd):
        assert of.compare({k: np.array(v, copy=True) for k, v in ref["want"].items()}, ref["want"]) == []

    def one(ref, key, how):
        diffs = of.compare(_flip(ref["want"], key, how), ref["want"])
        assert len(diffs) == 1 and diffs[0].startswith(key + ": 1 values differ"), diffs

    def flip_label(a):
        a[a.shape[0] // 2, a.shape[1] // 2] ^= 1

    def votes_off(a):
        a[-1, -1] += 1

    def seen_off(a):
        a[0] -= 1

    def last_bit(a):
        assert cloud["want"]["cloud.count"][0] > 0
        a.view(np.uint32)[0, 0, 2] ^= 1

    def mask_bit(a):
        a[-1, -1] ^= 1

    one(lab, "view0.labels", flip_label)
    one(lift, "votes", votes_off)
    one(lift, "seen", seen_off)
    one(cloud, "cloud.points", last_bit)
    one(rgbd, "view0.mask", mask_bit)
    got = _flip(cloud["want"], "cloud.index", lambda a: a.__setitem__((0, slice(0, 2)), a[0, 1::-1].copy()))
    assert cloud["want"]["cloud.count"][0] >= 2 and cloud["want"]["cloud.index"][0, 0] != cloud["want"]["cloud.index"][0, 1]
    diffs = of.compare(got, cloud["want"])
    assert len(diffs) == 1 and diffs[0].startswith("cloud.index: 2 values differ"), diffs
    # a NaN equals a NaN, -0 does not equal +0, a missing or mis-shaped output is reported
    w = {"x": np.array([np.nan, 0.0], np.float32)}
    assert of.compare({"x": np.array([np.nan, 0.0], np.float32)}, w) == []
    assert len(of.compare({"x": np.array([np.nan, -0.0], np.float32)}, w)) == 1
    assert len(of.compare({}, w)) == 1 and len(of.compare({"x": np.zeros(3, np.float32)}, w)) == 1


@pytest.mark.parametrize("seed", [of.OBS_SEEDS["labels"][1], of.OBS_SEEDS["labels"][7], of.OBS_SEEDS["cloud"][4]])
def test_reference_identities(seed):
    """What the label and lift references rest on, on three seeds (two poisoned, G = 7, 40 and 3): recolouring the scene leaves the
    oracle's alpha bit-identical, and every one-hot weight is finite and in [0, 1) (lift_ref.quantise's precondition)."""
    c, ref = _case(seed)
    assert c["poisoned"]
    assert ref["notes"]["alpha_same"] and ref["notes"]["weights_in_range"]
    inp = of.fz.scene_inputs(c)
    cm = c["cams"][0]
    w, a = of.group_weights(c, inp, cm.viewmat, cm.K, c["poses"][0])
    assert w.shape == (c["H"], c["W"], c["n_groups"]) and w.dtype == np.float32
    total = w.astype(np.float64).sum(-1)
    assert np.all(np.abs(total - a[..., 0]) <= 1e-5)                     # the groups partition the scene: their weights sum to alpha


def test_label_rule():
    w = np.array([[0.0, 0.0, 0.0], [0.2, 0.5, 0.5], [0.1, 0.0, 0.3]], np.float32)
    a = np.array([0.0, 0.9, 0.7], np.float32)
    assert of.label_rule(w, a, 0.0).tolist() == [0, 1, 2]                # all-zero weights: the tie goes to label 0
    assert of.label_rule(w, a, 0.8).tolist() == [255, 1, 255]
    assert of.label_rule(w, a, 1.0).tolist() == [255, 255, 255]
    assert float(a[2]) < 0.7                                             # float32(0.7) lies below the double 0.7 ...
    assert of.label_rule(w, a, 0.7).tolist() == [255, 1, 2]              # ... and the rule compares in float32: not below
    big = np.zeros((1, 300), np.float32)
    big[0, 299] = 1.0
    assert of.label_rule(big, np.ones(1, np.float32)).tolist() == [255]  # clamped


def test_named_lift_cases():
    """The cases kept from the long runs: each holds a Gaussian with a non-finite opacity that the reference SEES (it is listed
    and composited), in a frame with lanes beyond the image."""
    for seed, poison_all in of.LIFT_SEEDS_OPACITY_NOT_FINITE:
        c = of.draw_case(seed, poison_all)
        bad = np.nonzero(~np.isfinite(c["scene"].opacities))[0]
        assert c["arm"] == "lift" and len(bad) and (c["W"] % 16 or c["H"] % 16)
        assert (of.reference(c)["want"]["seen"][bad] > 0).any()
    for opacity in (np.inf, np.nan):
        sc, cam, labels, n_labels = of.reduced_lift_case(opacity)
        votes, seen = of.lift_ref.reference(sc, cam, labels[0], n_labels)
        # it is the nearer one and reaches every pixel of all four tiles with alpha 0.999; the other shows through it
        assert cam[2:] == (17, 17) and seen[1] == 17 * 17 * int(np.float32(0.999) * np.float32(of.lift_ref.LIFT_ONE)) and votes[1].sum() == seen[1]
        assert seen[0] > 0
