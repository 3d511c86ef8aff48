"""The case kit of the overflow tests for frames that ADD into the caller's buffers (tests/test_regrow_cpu.py,
tests/test_gpu_z_regrow_sums.py): lift_labels, lift_features and render_backward on a frame whose lists outgrow a fresh context's key
buffer, so that the frame is rendered twice ("Label lifting": "its first, truncated rendering adds nothing").

The case.  A fresh context's key buffer holds max(8 N, 2^20) keys, so the smallest frame that can overflow has more than 2^20 list
entries: the scene and the two cameras the stored-frame overflow tests already use (tests/test_gpu_parity.py,
test_gpu_f_features.py): make_scene(30000, seed=444, log_scale_mean=log 0.12) under ring_camera(640, 480, 500, yaw 0 / 90).

The yardstick.  No float64 reference runs at this size; what does is conservation against the C oracle's frame.  With
A(p) = 1 - T_final(p) the oracle's alpha (the forward frame equals it bit for bit), the weights a pixel hands out sum to A(p) in exact
arithmetic, so (C channels, ONE the fixed-point unit of DESIGN.md: 2^32 for label lifting, 2^24 for feature lifting, and
``feature_scale`` for the channels: sums hold q * fq = vis 2^24 * f feature_scale)

    sum_i seen[i]      / 2^32           = sum_p A(p)                   sum_i votes[i,l] / 2^32 = sum_{p: label l} A(p)
    sum_i weight[i]    / 2^24           = sum_{p: mask} A(p)           sum_i sums[i,c] / (2^24 feature_scale) = sum_{p: mask} A(p) f(p,c)
    sum_i d_colors[i,c]                 = sum_p g_rgb[p,c] A(p)        sum_i d_depths[i] = sum_p g_depth[p] A(p)

both sides in float64 on the host.  The measure is |lhs - rhs| / |rhs| (``miss``), and BOUND = 1e-3 holds it and the comparison of
the overflowing call with the same call on the grown context: a hundred times the float32 ceiling of this project's figures (1e-5,
tests/test_grad_cpu.py), a few hundred times under the smallest fault in question (a truncated attempt that added holds 2^20 / n_isect
of the frame, a second addition all of it).

The inputs are drawn so that no right-hand side cancels: feature channels and upstream gradients are ``mean + 0.5 N(0,1)`` with
|mean| >= 0.6, so sum |g| A / |sum g A| stays near 1 and a relative measure of the SUM says what it would say of its terms (zero-mean
inputs would leave a right-hand side of order sqrt(pixels), against which float32 rounding of 3e5 terms is no longer small, and a
doubled sum of which misses by no more than it does).  The generators take the image size, so the CPU tests draw the same
distributions at 32x32.  Everything is drawn once per process (functools.lru_cache) and never written to.
"""
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scene_cases as sc_kit  # noqa: E402

N, SEED, SCALE = 30000, 444, 0.12
W, H, F = 640, 480, 500.0
YAWS = (0.0, 90.0)
FLOOR = 1 << 20                     # keys of a fresh context's buffer while 8 N stays below it
N_LABELS, CHANNELS, N_GROUPS = 5, 3, 3
VIEWS5 = (0, 1, 0, 1, 0)            # the five-view calls: yaw alternating 0 and 90
BOUND = 1e-3
LIFT_ONE, LIFT_FEATURE_ONE = 2 ** 32, 2 ** 24                 # DESIGN.md 3, "Label lifting" / "Feature lifting"
FEATURE_MEANS = (1.0, -0.8, 0.6)
UPSTREAM_MEANS = dict(rgb=(1.0, -0.8, 0.6), alpha=0.9, depth=-0.7)
assert 8 * N < FLOOR


# ---- the scene, the cameras, the oracle's frames ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(groups=False):
    """The 30 000-Gaussian scene as a scene_cases dict; ``groups``: the same Gaussians in N_GROUPS posed groups (i mod 3)."""
    sc = sc_kit.synthetic(N, SEED, SCALE)
    if groups:
        sc = dict(sc, gid=(np.arange(N) % N_GROUPS).astype(np.uint8), G=N_GROUPS, Rt=sc_kit.random_group_poses(N_GROUPS, SEED + 1))
    return sc


@functools.lru_cache(maxsize=None)
def camera(view):
    return sc_kit.ring(W, H, f=F, yaw=YAWS[view], elev=0.0)


@functools.lru_cache(maxsize=None)
def frame(view, groups=False):
    """The C oracle's frame of camera ``view``: alpha [H,W] as float64, n_isect, n_visible (once per process)."""
    fr = sc_kit.oracle_frame(scene(groups), camera(view), (0.0, 0.0, 0.0))
    alpha = fr["alpha"][..., 0].astype(np.float64)
    alpha.setflags(write=False)
    return dict(alpha=alpha, n_isect=int(fr["n_isect"]), n_visible=int(fr["n_visible"]))


def cameras(views):
    """(viewmats [V,4,4], Ks [V,3,3]) of the cameras ``views`` (indices into YAWS)."""
    cams = [camera(v) for v in views]
    return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])


# ---- seeded inputs, by image size ---------------------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def labels(views=5, height=H, width=W, seed=1):
    """Label images [V,H,W] uint8: N_LABELS labels, about 10 % unlabelled (255)."""
    rng = np.random.default_rng(7000 + seed)
    lab = rng.integers(0, N_LABELS, size=(views, height, width)).astype(np.uint8)
    lab[rng.uniform(size=lab.shape) < 0.1] = 255
    return _frozen(lab)


@functools.lru_cache(maxsize=None)
def features(views=5, height=H, width=W, seed=2):
    """(images [V,H,W,3] float32 = FEATURE_MEANS + 0.5 N(0,1), mask [V,H,W] uint8 with about 30 % zeros)."""
    rng = np.random.default_rng(7000 + seed)
    img = (np.asarray(FEATURE_MEANS) + 0.5 * rng.normal(size=(views, height, width, CHANNELS))).astype(np.float32)
    mask = (rng.uniform(size=(views, height, width)) >= 0.3).astype(np.uint8)
    return _frozen(img), _frozen(mask)


@functools.lru_cache(maxsize=None)
def upstream(height=H, width=W, seed=3):
    """(g_rgb [H,W,3], g_alpha [H,W], g_depth [H,W]) float32 = UPSTREAM_MEANS + 0.5 N(0,1): magnitude O(1), no sum cancels."""
    rng = np.random.default_rng(7000 + seed)
    m = UPSTREAM_MEANS
    g_rgb = (np.asarray(m["rgb"]) + 0.5 * rng.normal(size=(height, width, 3))).astype(np.float32)
    g_alpha = (m["alpha"] + 0.5 * rng.normal(size=(height, width))).astype(np.float32)
    g_depth = (m["depth"] + 0.5 * rng.normal(size=(height, width))).astype(np.float32)
    return _frozen(g_rgb), _frozen(g_alpha), _frozen(g_depth)


def upper_half(a, axis=0):
    """``a`` with everything below the image's middle row zeroed (``axis``: the image's row axis): what a truncated attempt that
    reached only the first tile rows would have worked on."""
    out = np.array(a)
    idx = [slice(None)] * out.ndim
    idx[axis] = slice(out.shape[axis] // 2, None)
    out[tuple(idx)] = 0
    return out


# ---- the right-hand sides, in float64 ------------------------------------------------------------------------------------------------------
def label_rhs(alphas, lab, n_labels=N_LABELS):
    """(per label [G], over all pixels) of sum_p A(p) over the views: ``alphas`` a list of [H,W], ``lab [V,H,W]``."""
    votes, seen = np.zeros(n_labels), 0.0
    for a, l in zip(alphas, lab):
        a = np.asarray(a, np.float64)
        seen += a.sum()
        for g in range(n_labels):
            votes[g] += a[np.asarray(l) == g].sum()
    return votes, seen


def feature_rhs(alphas, images, mask=None):
    """(per channel [C] of sum_{p: mask} A(p) f(p,c), sum_{p: mask} A(p)) over the views."""
    sums, weight = np.zeros(np.asarray(images).shape[-1]), 0.0
    for k, a in enumerate(alphas):
        a = np.asarray(a, np.float64) * (1.0 if mask is None else (np.asarray(mask[k]) != 0))
        weight += a.sum()
        sums += np.einsum("hw,hwc->c", a, np.asarray(images[k], np.float64))
    return sums, weight


def grad_rhs(alpha, g_rgb, g_depth):
    """(sum_p g_rgb[p,c] A(p) [3], sum_p g_depth[p] A(p))."""
    a = np.asarray(alpha, np.float64)
    return np.einsum("hw,hwc->c", a, np.asarray(g_rgb, np.float64)), float((a * np.asarray(g_depth, np.float64)).sum())


# ---- the left-hand sides, in float64, in the right-hand sides' unit ------------------------------------------------------------------------
def label_lhs(votes, seen):
    """(sum_i votes[i,l] / 2^32 [G], sum_i seen[i] / 2^32) from int64 arrays; the column sums are taken in Python integers."""
    v, s = np.asarray(votes), np.asarray(seen)
    assert v.dtype == np.int64 and s.dtype == np.int64
    return np.array([int(c) / LIFT_ONE for c in v.sum(axis=0, dtype=object)], np.float64), int(s.sum(dtype=object)) / LIFT_ONE


def feature_lhs(sums, weight, feature_scale):
    s, w = np.asarray(sums), np.asarray(weight)
    assert s.dtype == np.int64 and w.dtype == np.int64
    unit = LIFT_FEATURE_ONE * float(feature_scale)
    return np.array([int(c) / unit for c in s.sum(axis=0, dtype=object)], np.float64), int(w.sum(dtype=object)) / LIFT_FEATURE_ONE


def grad_lhs(d_colors, d_depths):
    return np.asarray(d_colors, np.float64).reshape(-1, 3).sum(axis=0), float(np.asarray(d_depths, np.float64).sum())


def misses(lhs, rhs):
    """|lhs - rhs| / |rhs| per component: the conservation measure."""
    lhs, rhs = np.atleast_1d(np.asarray(lhs, np.float64)), np.atleast_1d(np.asarray(rhs, np.float64))
    assert lhs.shape == rhs.shape and (rhs != 0).all()
    return np.abs(lhs - rhs) / np.abs(rhs)


def miss(lhs, rhs):
    """... and its maximum over the components."""
    return float(misses(lhs, rhs).max())
