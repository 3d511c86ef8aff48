"""CPU: label lifting's host side -- masks_from_votes on hand-made vote tables, the reference the GPU tests hold lift_labels to
(tests/tools/lift_ref.py) on a one-Gaussian scene, and the C ABI's new symbol."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import lift_ref as lr  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

ONE = 2 ** 32


def _masks(votes, seen, names=("a", "b", "c"), **kw):
    from sim_a_splat_amd.segment import masks_from_votes
    return masks_from_votes(np.asarray(votes, np.int64), np.asarray(seen, np.int64), names, **kw)


def test_masks_ties_go_to_the_lowest_label():
    m = _masks([[5, 5, 0], [0, 7, 7], [3, 3, 3], [0, 0, 9]], [10, 14, 9, 9], min_share=0.0)
    assert m["a"].tolist() == [True, False, True, False]
    assert m["b"].tolist() == [False, True, False, False]
    assert m["c"].tolist() == [False, False, False, True]


def test_masks_both_thresholds():
    votes = [[6 * ONE, 4 * ONE, 0], [5 * ONE, 0, 0], [4 * ONE, 0, 0], [ONE, 0, 0]]
    seen = [10 * ONE, 10 * ONE, 10 * ONE, ONE]
    m = _masks(votes, seen)                                    # min_share 0.5: 0.6 in, exactly 0.5 in (>=), 0.4 out
    assert m["a"].tolist() == [True, True, False, True]
    m = _masks(votes, seen, min_share=0.55)
    assert m["a"].tolist() == [True, False, False, True]
    m = _masks(votes, seen, min_share=0.0, min_seen=ONE)       # seen > min_seen: the Gaussian seen exactly ONE is out
    assert m["a"].tolist() == [True, True, True, False]
    m = _masks(votes, seen, min_share=0.0, min_seen=ONE - 1)
    assert m["a"].tolist() == [True, True, True, True]
    assert not m["b"].any() and not m["c"].any()


def test_masks_unseen_and_unvoted_gaussians_belong_to_nobody():
    # seen == 0; seen through unlabelled pixels only (votes all 0): neither may land in label 0 by argmax's default
    m = _masks([[0, 0, 0], [0, 0, 0], [0, 2, 0]], [0, 50, 2], min_share=0.0)
    assert not m["a"].any() and not m["c"].any()
    assert m["b"].tolist() == [False, False, True]


def test_masks_are_disjoint_and_round_trip_through_the_mask_file(tmp_path):
    from sim_a_splat_amd import io
    rng = np.random.default_rng(3)
    votes = rng.integers(0, 50, size=(500, 4)) * ONE
    votes[rng.uniform(size=500) < 0.2] = 0
    seen = votes.sum(axis=1) + rng.integers(0, 30, size=500) * ONE
    names = ["link0", "link1", "mug", "cloth"]
    m = _masks(votes, seen, names, min_share=0.3)
    assert list(m) == names and all(v.dtype == bool and v.shape == (500,) for v in m.values())
    stack = np.stack([m[k] for k in names])
    assert stack.sum(axis=0).max() == 1 and stack.any(axis=1).all()
    io.save_link_masks(tmp_path / "link_masks_global_dict.npz", m)
    back = io.load_link_masks(tmp_path / "link_masks_global_dict.npz")
    assert set(back) == set(names) and all(np.array_equal(back[k], m[k]) for k in names)
    # tensors are taken as arrays are
    import torch
    m2 = _masks(torch.from_numpy(votes), torch.from_numpy(seen), names, min_share=0.3)
    assert all(np.array_equal(m2[k], m[k]) for k in names)
    with pytest.raises(ValueError):
        _masks(votes, seen[:-1], names)
    with pytest.raises(ValueError):
        _masks(votes, seen, names[:3])


def test_reference_on_one_gaussian():
    """lift_ref: seen is the sum of floor(rgb * 2^32) of the oracle's frame of the one Gaussian drawn white, and a label image split
    in two halves splits it accordingly."""
    import oracle
    oracle.build()
    sc = dict(means=np.array([[0.1, -0.05, 0.0]], np.float32), op=np.array([0.8], np.float32), colors=np.array([[1.0, 1.0, 1.0]], np.float32),
              sh=-1, quats=np.array([[1.0, 0.2, 0.1, 0.0]], np.float32), scales=np.array([[0.5, 0.3, 0.4]], np.float32), cov6=None,
              gid=None, G=0, Rt=None)
    cam = sc_kit.ring(16, 16, f=14.0, yaw=0.0, elev=0.0)
    fr = sc_kit.oracle_frame(sc, cam, (0.0, 0.0, 0.0))
    q = np.floor(fr["rgb"].astype(np.float64) * ONE).astype(np.int64)
    assert (q[..., 0] == q[..., 1]).all() and (q[..., 0] == q[..., 2]).all() and (q[..., 0] > 0).sum() > 100
    labels = np.zeros((16, 16), np.uint8)
    labels[:, 8:] = 1
    labels[7, :] = 255                                          # unlabelled: seen only
    votes, seen = lr.reference(sc, cam, labels, 2)
    assert votes.shape == (1, 2) and seen.shape == (1,) and votes.dtype == np.int64 and seen.dtype == np.int64
    assert seen[0] == q[..., 0].sum()
    rest = np.arange(16) != 7
    assert votes[0, 0] == q[rest, :8, 0].sum() > 0 and votes[0, 1] == q[rest, 8:, 0].sum() > 0
    assert votes[0].sum() == seen[0] - q[7, :, 0].sum() and q[7, :, 0].sum() > 0
    # a label the call does not count (>= n_labels) is unlabelled too
    v1, s1 = lr.reference(sc, cam, labels, 1)
    assert s1[0] == seen[0] and v1[0, 0] == votes[0, 0]


def test_header_declares_and_library_exports_sas_lift_labels():
    from sim_a_splat_amd import _capi, build
    header = (ROOT / "include" / "sim_a_splat_amd.h").read_text()
    assert re.search(r"\bint\s+sas_lift_labels\s*\(\s*sas_ctx\s*\*", header)
    assert re.search(r"#define\s+SAS_LIFT_ONE\s+4294967296\.0f", header)
    assert "sas_lift_labels" in _capi.EXPORTS and _capi.SAS_LIFT_ONE == ONE
    L = ctypes.CDLL(str(build.build()))
    assert hasattr(L, "sas_lift_labels")
    assert len(_capi.lib().sas_lift_labels.argtypes) == 12
    from sim_a_splat_amd import rasterizer
    assert rasterizer.LIFT_ONE == ONE and callable(rasterizer.Rasterizer.lift_labels)
