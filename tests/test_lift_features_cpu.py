"""CPU: feature lifting's host side -- the reference the GPU tests hold lift_features to (tests/tools/lift_features_ref.py) on a
hand-computed two-Gaussian case, features_from_sums, relevancy, masks_from_relevancy, the slab bookkeeping of lift_feature_views
on a stub rasterizer, set_language_queries' string handling, and the C ABI's new symbol."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import lift_features_ref as fr  # noqa: E402

ONE = 2 ** 24


def test_reference_on_two_gaussians_by_hand():
    # two Gaussians, a 1x3 image of 2 channels; weights chosen exact in float32
    w = np.array([[[0.5, 0.25, 0.0]], [[0.0, 0.75, 2.0 ** -25]]], np.float32)       # [2,1,3]
    img = np.array([[[1.0, -2.0], [0.5, 4.0], [np.nan, -np.inf]]], np.float32)        # [1,3,2]
    scale = 1000.0
    s, wt = fr.sums(w, img, scale)
    q = [[ONE // 2, ONE // 4, 0], [0, 3 * ONE // 4, 0]]                              # 2^-25 * 2^24 = 0.5 -> floor 0
    fq = [[1000, -2000], [500, 4000], [0, -32767]]
    assert wt.tolist() == [q[0][0] + q[0][1], q[1][1]] and wt.dtype == np.int64 and s.dtype == np.int64
    assert s.tolist() == [[q[0][0] * fq[0][0] + q[0][1] * fq[1][0], q[0][0] * fq[0][1] + q[0][1] * fq[1][1]],
                          [q[1][1] * fq[1][0], q[1][1] * fq[1][1]]]
    # a mask removes the middle pixel from both outputs
    s, wt = fr.sums(w, img, scale, mask=np.array([[1, 0, 7]], np.uint8))
    assert wt.tolist() == [q[0][0], 0] and s.tolist() == [[q[0][0] * 1000, q[0][0] * -2000], [0, 0]]


def test_reference_quantiser_edges():
    f = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.5, 1.5, 2.5, -0.5, -1.5, -0.0, 32766.5, 32767.4, 40000.0], np.float32)
    assert fr.quantise_features(f, 1.0).tolist() == [0, 32767, -32767, 32767, -32767, 0, 2, 2, 0, -2, 0, 32766, 32767, 32767]
    # the product is float32's: float32(0.1) * 25 rounds to 2.5 exactly, a tie (-> 2); in float64 it is 2.50000004 (-> 3)
    assert fr.quantise_features(np.array([0.5, 0.1], np.float32), np.array([5.0, 25.0])).tolist() == [2, 2]
    assert np.rint(float(np.float32(0.1)) * 25.0) == 3.0
    assert fr.auto_scale(np.array([0.0, np.nan, -4.0, np.inf], np.float32)) == float(np.float32(32767 / 4.0))
    assert fr.auto_scale(np.zeros(3, np.float32)) == 1.0


def test_features_from_sums_mean_unseen_and_overflow_guard():
    from sim_a_splat_amd.semantics import features_from_sums
    scale = 100.0
    weight = torch.tensor([3 * ONE, 0, ONE // 2, 5], dtype=torch.int64)
    sums = torch.tensor([[3 * ONE * 250, -3 * ONE * 100], [0, 0], [(ONE // 2) * -32767, 0], [5 * 7, 5 * 9]], dtype=torch.int64)
    f, seen = features_from_sums(sums, weight, scale)
    assert f.dtype == torch.float32 and seen.dtype == torch.bool and seen.tolist() == [True, False, True, True]
    assert torch.equal(f, torch.tensor([[2.5, -1.0], [0.0, 0.0], [-327.67, 0.0], [0.07, 0.09]], dtype=torch.float32))
    f, seen = features_from_sums(sums, weight, scale, min_weight=5)          # weight > min_weight
    assert seen.tolist() == [True, False, True, False] and f[3].tolist() == [0.0, 0.0]
    f2, _ = features_from_sums(sums.numpy(), weight.numpy(), scale)           # arrays are taken as tensors are
    assert f2[0].tolist() == [2.5, -1.0]
    weight[0] = 2 ** 48 - 1
    features_from_sums(sums, weight, scale)
    weight[0] = 2 ** 48
    with pytest.raises(OverflowError):
        features_from_sums(sums, weight, scale)
    with pytest.raises(ValueError):
        features_from_sums(sums, weight[:-1], scale)
    with pytest.raises(ValueError):
        features_from_sums(sums.to(torch.int32), weight, scale)


def _relevancy64(e, p, n, t):
    """The LERF rule restated in float64 numpy, softmax written out."""
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    e, p, n = unit(np.asarray(e, np.float64)), unit(np.asarray(p, np.float64)), unit(np.asarray(n, np.float64))
    out = np.zeros((len(e), len(p)))
    for j in range(len(p)):
        a = t * (e @ p[j])
        probs = []
        for k in range(len(n)):
            b = t * (e @ n[k])
            m = np.maximum(a, b)
            probs.append(np.exp(a - m) / (np.exp(a - m) + np.exp(b - m)))
        out[:, j] = np.min(probs, axis=0)
    return out


def test_relevancy_matches_float64_restatement():
    from sim_a_splat_amd.semantics import relevancy
    rng = np.random.default_rng(0)
    e, p, n = rng.normal(size=(200, 32)).astype(np.float32), rng.normal(size=(3, 32)).astype(np.float32), rng.normal(size=(4, 32)).astype(np.float32)
    got = relevancy(torch.from_numpy(e), p, n)
    assert got.shape == (200, 3) and got.dtype == torch.float32
    assert np.abs(got.numpy().astype(np.float64) - _relevancy64(e, p, n, 10.0)).max() <= 1e-6
    got = relevancy(e, p, n[:1], temperature=3.0)
    assert np.abs(got.numpy().astype(np.float64) - _relevancy64(e, p, n[:1], 3.0)).max() <= 1e-6
    # an embedding equal to the positive and opposite to the negative: sigmoid(2 t); equal to the negative too: 0.5
    r = relevancy(np.array([[1.0, 0.0], [0.0, 3.0]], np.float32), np.array([[2.0, 0.0]], np.float32), np.array([[-1.0, 0.0]], np.float32))
    assert abs(float(r[0, 0]) - 1.0 / (1.0 + np.exp(-20.0))) <= 1e-6 and float(r[1, 0]) == 0.5
    assert relevancy(np.zeros((2, 2), np.float32), [[1.0, 0.0]], [[0.0, 1.0]]).tolist() == [[0.5], [0.5]]   # a zero row stays zero
    with pytest.raises(ValueError):
        relevancy(e, p, np.zeros((0, 32), np.float32))                                                    # Q >= 1
    with pytest.raises(ValueError):
        relevancy(e, p[:, :5], n)


def test_masks_from_relevancy_ties_threshold_and_seen():
    from sim_a_splat_amd.semantics import masks_from_relevancy
    rel = np.array([[0.7, 0.7, 0.1], [0.2, 0.5, 0.5], [0.49, 0.3, 0.2], [0.1, 0.2, 0.9], [0.5, 0.0, 0.0]])
    m = masks_from_relevancy(rel, ["a", "b", "c"])
    assert m["a"].tolist() == [True, False, False, False, True]      # the tie to the lowest j; exactly the threshold is in (>=)
    assert m["b"].tolist() == [False, True, False, False, False]
    assert m["c"].tolist() == [False, False, False, True, False]     # row 2's maximum 0.49 < 0.5: nobody's
    m = masks_from_relevancy(torch.from_numpy(rel), ["a", "b", "c"], threshold=0.6, seen=np.array([1, 1, 1, 0, 1], bool))
    assert m["a"].tolist() == [True, False, False, False, False] and not m["b"].any() and not m["c"].any()
    stack = np.stack(list(masks_from_relevancy(rel, ["a", "b", "c"], threshold=0.0).values()))
    assert (stack.sum(axis=0) == 1).all() and stack.dtype == bool
    with pytest.raises(ValueError):
        masks_from_relevancy(rel, ["a", "b"])
    with pytest.raises(ValueError):
        masks_from_relevancy(rel, ["a", "a", "b"])
    with pytest.raises(ValueError):
        masks_from_relevancy(rel, ["a", "b", "c"], seen=np.ones(4, bool))


class _StubRasterizer:
    """lift_features as a recorder: adds (views, channel offset marker) into the buffers it is handed, as the real one accumulates."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def lift_features(self, V, K, W, H, images, *, feature_scale, mask, sums, weight):
        images = np.asarray(images)
        D = images.shape[-1]
        assert D <= 256 and images.shape[:3] == (len(V), H, W)
        self.calls.append((len(V), D, feature_scale, None if mask is None else np.asarray(mask).shape, sums is None, weight))
        out = {"feature_scale": feature_scale}
        s = torch.zeros((self.n, D), dtype=torch.int64) if sums is None else sums
        s += torch.from_numpy(images.reshape(-1, D).sum(axis=0).astype(np.int64))[None, :]
        out["sums"] = s
        if weight is not False:
            w = torch.zeros(self.n, dtype=torch.int64) if weight is None else weight
            w += len(V)
            out["weight"] = w
        return out


def test_lift_feature_views_slabs_and_batches():
    from sim_a_splat_amd.semantics import lift_feature_views
    C, H, W, D = 5, 2, 3, 600
    rng = np.random.default_rng(1)
    img = rng.integers(-5, 6, size=(C, H, W, D)).astype(np.float32)
    V, K = np.tile(np.eye(4, dtype=np.float32), (C, 1, 1)), np.tile(np.eye(3, dtype=np.float32), (C, 1, 1))
    r = _StubRasterizer(4)
    out = lift_feature_views(r, V, K, W, H, img, 2.0, mask=np.ones((C, H, W), np.uint8), views_per_call=2)
    # three batches of views (2, 2, 1) x three slabs (256, 256, 88); weight only with the first slab
    assert [(c[0], c[1]) for c in r.calls] == [(2, 256), (2, 256), (2, 88), (2, 256), (2, 256), (2, 88), (1, 256), (1, 256), (1, 88)]
    assert all(c[2] == 2.0 and c[3] == (c[0], H, W) for c in r.calls)
    assert [c[5] is False for c in r.calls] == [False, True, True] * 3
    assert [c[4] for c in r.calls] == [True] * 3 + [False] * 6          # buffers allocated once, then accumulated into
    assert out["sums"].shape == (4, D) and out["weight"].tolist() == [C] * 4 and out["feature_scale"] == 2.0
    assert np.array_equal(out["sums"][0].numpy(), img.reshape(-1, D).sum(axis=0).astype(np.int64))
    # a sequence of images, one slab
    r = _StubRasterizer(2)
    out = lift_feature_views(r, V[:3], K[:3], W, H, [img[0, ..., :7], torch.from_numpy(img[1, ..., :7]), img[2, ..., :7]], 1.0)
    assert [(c[0], c[1], c[3]) for c in r.calls] == [(3, 7, None)] and out["sums"].shape == (2, 7)
    with pytest.raises(ValueError):
        lift_feature_views(r, V, K, W, H, img[:4], 1.0)
    with pytest.raises(ValueError):
        lift_feature_views(r, V, K, W, H, img, None)                     # one scale for all calls
    with pytest.raises(ValueError):
        lift_feature_views(r, V, K, W, H, img, 1.0, views_per_call=0)


def _splat(n=6):
    from sim_a_splat_amd.gaussian_splat import GaussianSplat, PinholeCamera, SplatModel
    rng = np.random.default_rng(4)
    model = SplatModel(rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.normal(size=(n, 4)), rng.normal(size=(n, 3)),
                       rng.normal(size=(n, 15, 3)), rng.normal(size=(n, 1)))
    return GaussianSplat.from_model(model, PinholeCamera(torch.eye(4)[:3], 10.0, 10.0, 8.0, 8.0, 16, 16)), model


def test_set_language_queries_takes_embeddings_and_refuses_bare_strings():
    gs, model = _splat()
    assert model.clip_embeds is None and model.positives is None
    with pytest.raises(ValueError, match="no text encoder ships here"):
        gs.set_language_queries(["mug"], np.ones((1, 4), np.float32))
    with pytest.raises(ValueError, match="no text encoder ships here"):
        gs.set_language_queries(np.ones((1, 4), np.float32), "object")
    gs.set_language_queries(np.ones((2, 4), np.float32), np.ones(4, np.float32))
    assert model.positives.shape == (2, 4) and model.negatives.shape == (1, 4) and model.positives.dtype == torch.float32
    table = {"mug": [1.0, 0, 0, 0], "cloth": [0, 1.0, 0, 0], "object": [0, 0, 1.0, 0], "stuff": [0, 0, 0, 1.0]}
    seen = []

    def encoder(words):
        seen.append(list(words))
        return np.array([table[w] for w in words], np.float32)
    gs.set_language_queries(["mug", "cloth"], ("object", "stuff"), encoder=encoder)
    assert seen == [["mug", "cloth"], ["object", "stuff"]] and model.positives.tolist() == [table["mug"], table["cloth"]]
    with pytest.raises(ValueError):
        gs.set_language_queries(np.ones((1, 4), np.float32), np.ones((1, 5), np.float32))
    # per-Gaussian relevancy needs embeddings: the same TypeError as compute_semantics without them
    with pytest.raises(TypeError, match="compute_semantics is not supported"):
        gs.get_semantic_point_cloud(model.positives, model.negatives)
    with pytest.raises(ValueError):
        model.set_clip_embeds(np.zeros((5, 4), np.float32))
    e = np.tile(np.array(table["mug"], np.float32), (6, 1))
    model.set_clip_embeds(e)
    rel = gs.get_semantic_point_cloud(model.positives, model.negatives)
    assert rel.shape == (6, 2) and bool((rel[:, 0] > 0.99).all()) and bool((rel[:, 1] == 0.5).all())
    rel2 = gs.get_semantic_point_cloud(model.positives, model.negatives, pcd_attr={"clip_embeds": e[:2]})
    assert rel2.shape == (2, 2)


def test_header_declares_and_library_exports_sas_lift_features():
    from sim_a_splat_amd import _capi, build, rasterizer
    header = (ROOT / "include" / "sim_a_splat_amd.h").read_text()
    assert re.search(r"\bint\s+sas_lift_features\s*\(\s*sas_ctx\s*\*", header)
    assert re.search(r"#define\s+SAS_LIFT_FEATURE_ONE\s+16777216\.0f", header)
    assert "sas_lift_features" in _capi.EXPORTS and _capi.SAS_LIFT_FEATURE_ONE == ONE
    L = ctypes.CDLL(str(build.build()))
    assert hasattr(L, "sas_lift_features")
    assert len(_capi.lib().sas_lift_features.argtypes) == 14
    assert rasterizer.LIFT_FEATURE_ONE == ONE and callable(rasterizer.Rasterizer.lift_features)
