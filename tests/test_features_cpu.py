"""CPU: the host-side pieces of the feature channels -- the group label reduction and argument validation."""
import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi
from sim_a_splat_amd.rasterizer import MAX_FEATURES, feature_background_array, feature_channels, group_labels


def test_labels_take_the_argmax_with_ties_to_the_lowest_group():
    w = torch.tensor([[[0.1, 0.7, 0.2], [0.4, 0.4, 0.2]],
                      [[0.0, 0.0, 0.0], [0.3, 0.3, 0.3]]], dtype=torch.float32)
    a = torch.tensor([[[1.0], [0.8]], [[0.0], [0.9]]], dtype=torch.float32)
    lab = group_labels(w, a, min_alpha=0.5)
    assert lab.dtype == torch.uint8 and lab.shape == (2, 2)
    assert lab.tolist() == [[1, 0], [255, 0]]


def test_labels_match_numpy_argmax_on_drawn_weights():
    rng = np.random.default_rng(0)
    w = rng.integers(0, 4, size=(40, 30, 9)).astype(np.float32) / 4    # many ties
    a = rng.uniform(0, 1, size=(40, 30, 1)).astype(np.float32)
    lab = group_labels(torch.from_numpy(w), torch.from_numpy(a), min_alpha=0.3).numpy()
    ref = np.argmax(w, axis=-1).astype(np.uint8)       # numpy: the first maximum
    ref[a[..., 0] < 0.3] = 255
    assert np.array_equal(lab, ref)


def test_labels_threshold_is_strict():
    w = torch.ones((1, 2, 2))
    a = torch.tensor([[[0.5], [0.4999]]])
    assert group_labels(w, a, 0.5).tolist() == [[0, 255]]


def test_feature_shape_validation():
    assert feature_channels((5, 3), 5) == 3
    assert feature_channels((0, 1), 0) == 1
    assert feature_channels((4, MAX_FEATURES), 4) == MAX_FEATURES
    for shape, n in [((5,), 5), ((5, 3), 4), ((5, 0), 5), ((5, MAX_FEATURES + 1), 5), ((5, 2, 2), 5)]:
        with pytest.raises(ValueError):
            feature_channels(shape, n)


def test_feature_background_validation():
    assert feature_background_array(None, 3) is None
    a = feature_background_array([1, 2, 3], 3)
    assert a.dtype == np.float32 and a.flags.c_contiguous and a.tolist() == [1, 2, 3]
    assert feature_background_array(torch.arange(4.0), 4).tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        feature_background_array([1, 2], 3)


def test_binding_and_header_declare_the_feature_calls():
    from pathlib import Path
    hdr = (Path(__file__).resolve().parent.parent / "include" / "sim_a_splat_amd.h").read_text()
    for name in ("sas_scene_features", "sas_render_features"):
        assert name in _capi.EXPORTS
        assert f"int {name}(" in hdr
