"""CPU: what tests/test_gpu_i_mesh_features.py asserts about the REFERENCE, settled without a GPU, and the host-side validators of
Rasterizer.upload_mesh_features.

The GPU tests hold the HIP frames to oracle.mesh_ref + the depth-limited oracle on stable pixels, under caps: the excluded share,
the shares of a label frame that show the mesh and the splats, the share on which the scene depth moves away from the splat-only
depth, and a depth tolerance that stays a small share of the depth.  Here every cap is evaluated with the oracle alone, so the GPU
tests assert conditions the reference is known to meet.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import mesh_cases as mc  # noqa: E402
import mesh_feature_cases as mf  # noqa: E402
import oracle_fuzz as fz  # noqa: E402
from sim_a_splat_amd.rasterizer import mesh_feature_channels, mesh_onehot_channels  # noqa: E402


# ---- host validators --------------------------------------------------------------------------------------------------------------
def test_mesh_feature_shapes():
    assert mesh_feature_channels((12, 5), 12, 5) == 5
    assert mesh_feature_channels([1, 256], 1, 256) == 256
    for shape in ((12,), (11, 5), (12, 5, 1), (5, 12)):
        with pytest.raises(ValueError):
            mesh_feature_channels(shape, 12, 5)


def test_mesh_feature_channel_mismatch():
    with pytest.raises(ValueError, match="feature store's 5 channels"):
        mesh_feature_channels((12, 4), 12, 5)
    with pytest.raises(ValueError, match="need a feature store"):
        mesh_feature_channels((12, 4), 12, 0)
    with pytest.raises(ValueError, match="need meshes"):
        mesh_feature_channels((0, 4), 0, 4)


def test_mesh_onehot_needs_a_channel_per_group():
    assert mesh_onehot_channels(np.array([0, 2, 2], np.uint8), 3, 3) == 3
    with pytest.raises(ValueError, match="has no channel"):
        mesh_onehot_channels(np.array([0, 3, 2], np.uint8), 3, 3)     # a scene without that many groups
    with pytest.raises(ValueError, match="need a feature store"):
        mesh_onehot_channels(np.array([0], np.uint8), 1, 0)
    with pytest.raises(ValueError, match="need meshes"):
        mesh_onehot_channels(np.zeros(0, np.uint8), 0, 3)
    with pytest.raises(ValueError):
        mesh_onehot_channels(np.array([0, 1], np.uint8), 3, 3)


def test_triples_cover_the_chunks():
    assert mf.triples(3) == [0] and mf.triples(9) == [0, 3, 6] and mf.triples(24) == [0, 11, 21]
    assert all(o + 3 <= C for C in mf.CHANNELS + (7,) for o in mf.triples(C))


def test_labels_of_matches_group_labels():
    import torch
    from sim_a_splat_amd.rasterizer import group_labels
    rng = np.random.default_rng(2)
    w = rng.uniform(0, 1, (9, 7, 5)).astype(np.float32)
    w[0, 0] = 0.25                                # a tie: the lowest row
    a = rng.uniform(0, 1, (9, 7, 1)).astype(np.float32)
    assert np.array_equal(mf.labels_of(w, a), group_labels(torch.from_numpy(w), torch.from_numpy(a)).numpy())


# ---- the caps of the fixed cases ----------------------------------------------------------------------------------------------------
def _surface_caps(name, e):
    s = mf.surface_reference(e)
    on = s["on"]
    rel = s["tol"][on] / s["D"][on]
    print(f"{name}: excluded {100 * e['excluded']:.2f} %, covered {100 * s['covered'].mean():.1f} %, stable uncovered {100 * s['off'].mean():.1f} %, "
          f"depth moves on {100 * s['moved_share']:.1f} %, tol / D_ref median {np.median(rel):.2e} max {rel.max():.2e}")
    assert np.isfinite(s["D"][on]).all() and (s["D"][on] > 0).all()
    assert (rel < mf.MAX_REL_TOL).all(), float(rel.max())
    return s


@pytest.mark.parametrize("name", list(mf.CASES))
def test_fixed_case_caps(name):
    case = mf.CASES[name]()
    e = mc.expected(case, 0)
    assert e["excluded"] <= mc.MAX_EXCLUDED
    s = _surface_caps(name, e)
    assert s["on"].mean() > 0.2                                       # the triangle shows on a good part of every case
    if name in mf.DEPTH_MOVES_CASES:
        assert s["moved_share"] >= mf.DEPTH_MOVES_MIN_SHARE           # an unchanged depth cannot pass the GPU test
    if name == "tblock":
        assert s["off"].mean() > 0.5                                  # ... and here most of the frame checks "uncovered pixels keep their bits"
    # the recolouring check compares three channels at a time against a frame whose background map is the triangles' rows
    f, fm, fbg = mf.draw_features(case, 9, seed=1)
    rgb = mf.oracle_recoloured_rgb(case, e, 0, f[:, 3:6], fm[:, 3:6], fbg[3:6])
    w = e["ref"]["winner"]
    opaque_mesh = (w >= 0) & (e["frame"]["alpha"][..., 0] == 0)
    assert np.array_equal(rgb[opaque_mesh], fm[:, 3:6][w[opaque_mesh]])   # nothing in front: the triangle's row itself, unshaded


def test_label_case_shares():
    case = mf.case_labels()
    e = mc.expected(case, 0)
    want = mf.expected_labels(case, e)
    st, G = e["stable"], case["sc"]["G"]
    assert G == 6 and list(case["mesh"]["groups"]) == [5, 5]
    assert np.array_equal(case["sc"]["Rt"].reshape(G, 12)[5], np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(12))
    mesh_share = float((st & (want["labels"] == G - 1)).mean())
    splat_share = float((st & (want["labels"] < G - 1)).mean())
    print(f"labels: excluded {100 * e['excluded']:.2f} %, mesh row {100 * mesh_share:.1f} %, splat rows {100 * splat_share:.1f} %")
    assert e["excluded"] <= mc.MAX_EXCLUDED
    assert mesh_share >= mf.LABEL_MIN_SHARE and splat_share >= mf.LABEL_MIN_SHARE
    assert len(np.unique(want["labels"][st & (want["labels"] < G - 1)])) >= 2        # more than one splat row shows
    # sum_g weights = alpha of the scene, up to rounding (1 on a covered pixel)
    assert float(np.abs(want["weights"].sum(-1) - want["alpha"])[st].max()) <= 1e-6


# ---- the drawn cases -------------------------------------------------------------------------------------------------------------------
def _drawn_meets_caps(seed):
    case = mf.drawn_case(seed)
    e = mc.expected(case, 0)
    s = mf.surface_reference(e)
    on = s["on"]
    rel = s["tol"][on] / s["D"][on] if on.any() else np.zeros(0)
    ok = e["excluded"] <= fz.MESH_MAX_EXCLUDED and bool(np.isfinite(s["D"][on]).all()) and bool((rel < mf.MAX_REL_TOL).all())
    return ok, f"{case['describe']} | excluded {100 * e['excluded']:.2f} % covered {100 * s['covered'].mean():.0f} % tol / D_ref max {rel.max(initial=0.0):.2e}"


def test_drawn_seed_list():
    """DRAWN_SEEDS is the first twenty seeds, from 0 upward, whose reference meets the caps; the two skipped ones do not."""
    assert len(mf.DRAWN_SEEDS) == 20 and mf.DRAWN_SEEDS == tuple(s for s in range(max(mf.DRAWN_SEEDS) + 1) if s not in mf.DRAWN_SEEDS_SKIPPED)
    for seed in range(max(mf.DRAWN_SEEDS) + 1):
        ok, line = _drawn_meets_caps(seed)
        print(("ok      " if ok else "SKIPPED ") + line)
        assert ok == (seed in mf.DRAWN_SEEDS), line
