"""The reference of label lifting (sas_lift_labels; DESIGN.md 3, "Label lifting"), from code that predates it.

The weight image of Gaussian i -- vis_i(p), the float32 weight the frame's compositing gives it at pixel p -- is the red channel of the C
oracle's frame of the scene recoloured one-hot: final RGB (sh_degree < 0), colour row i = (1, 0, 0), every other row 0, background 0.  A
Gaussian enters a pixel's sum at most once, with fma(1, vis, 0 + ...zeros) = vis, and the epilogue adds (1 - alpha) * 0: the channel IS
vis_i(p), bit for bit.  Three Gaussians ride on one oracle frame (red, green, blue).  Scenes beyond a couple of hundred Gaussians take
the weights from Rasterizer.render_features instead (explicit one-hot features, 256 Gaussians per pass, zero feature background): the
same identity on a path that is itself held to the oracle (tests/test_gpu_f_features.py).  Nothing here calls lift_labels.

    votes_ref[i, g] = sum_p floor(vis_i(p) * 2^32) [labels(p) == g]        seen_ref[i] = sum_p floor(vis_i(p) * 2^32)
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scene_cases as sc_kit  # noqa: E402

LIFT_ONE = 2 ** 32
ORACLE_MAX = 200   # Gaussians up to which the oracle's one-hot frames are the weights (a third as many frames)


def weights_oracle(sc, cam, Rt=None):
    """vis [N,H,W] float32 from the C oracle: one frame per three Gaussians."""
    V, K, W, H = cam
    n = len(sc["means"])
    out = np.zeros((n, H, W), np.float32)
    flat = dict(sc, sh=-1)
    for a in range(0, n, 3):
        col = np.zeros((n, 3), np.float32)
        for k in range(min(3, n - a)):
            col[a + k, k] = 1.0
        fr = sc_kit.oracle_frame(dict(flat, colors=col), cam, (0.0, 0.0, 0.0), Rt=Rt)
        for k in range(min(3, n - a)):
            out[a + k] = fr["rgb"][..., k]
    return out


def weights_features(r, sc, cam, Rt=None):
    """vis [N,H,W] float32 from Rasterizer.render_features with explicit one-hot features, 256 Gaussians per pass.  Leaves the scene
    uploaded on ``r`` (with the last pass's features in the store)."""
    V, K, W, H = cam
    n = len(sc["means"])
    sc_kit.upload(r, sc)
    if Rt is not None:
        r.set_group_poses(Rt)
    out = np.zeros((n, H, W), np.float32)
    for a in range(0, n, 256):
        b = min(n, a + 256)
        f = np.zeros((n, b - a), np.float32)
        f[np.arange(a, b), np.arange(b - a)] = 1.0
        r.upload_features(f)
        got = r.render_features(V, K, W, H, want=("features",))["features"].cpu().numpy()
        out[a:b] = np.moveaxis(got, 2, 0)
    return out


def quantise(w):
    """floor(vis * 2^32) as int64; the product is exact in float32 (and in float64)."""
    w = np.asarray(w)
    assert w.dtype == np.float32 and (w >= 0).all() and (w < 1).all()
    return np.floor(w.astype(np.float64) * float(LIFT_ONE)).astype(np.int64)


def sums(weights, labels, n_labels):
    """(votes [N,G], seen [N]) int64 of ONE view: ``weights [N,H,W]``, ``labels [H,W]`` uint8."""
    q = quantise(weights).reshape(len(weights), -1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    votes = np.zeros((len(q), n_labels), np.int64)
    for g in range(n_labels):
        hit = lab == g
        if hit.any():
            votes[:, g] = q[:, hit].sum(axis=1)
    return votes, q.sum(axis=1)


def reference(sc, cam, labels, n_labels, Rt=None, rasterizer=None):
    """(votes, seen) of one view; the oracle's weights up to ORACLE_MAX Gaussians, else the feature path's on ``rasterizer``."""
    if len(sc["means"]) <= ORACLE_MAX:
        w = weights_oracle(sc, cam, Rt)
    else:
        assert rasterizer is not None, "scenes beyond ORACLE_MAX Gaussians need a Rasterizer for the feature path"
        w = weights_features(rasterizer, sc, cam, Rt)
    return sums(w, labels, n_labels)


# ---- the scenes of the lift tests ---------------------------------------------------------------------------------------------------------
def blob_scene(n, seed, scale, n_groups=0, spread=1.0, z_spread=1.0, op=(0.2, 0.95)):
    """n isotropic-ish Gaussians in a box of half width ``spread`` (x, y) and ``z_spread`` (z), final RGB colours."""
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.uniform(-z_spread, z_spread, n)], 1)
    gid = (np.arange(n) % n_groups).astype(np.uint8) if n_groups else None
    return dict(means=means.astype(np.float32), op=rng.uniform(op[0], op[1], n).astype(np.float32),
                colors=rng.uniform(0, 1, (n, 3)).astype(np.float32), sh=-1, quats=rng.normal(size=(n, 4)).astype(np.float32),
                scales=(scale * rng.uniform(0.6, 1.4, (n, 3))).astype(np.float32), cov6=None, gid=gid, G=n_groups,
                Rt=sc_kit.random_group_poses(n_groups, seed + 1) if n_groups else None)


def two_clusters(seed=5, n_each=100, scale=0.01):
    """Two clusters of small Gaussians at x = -0.6 (group 0) and x = +0.6 (group 1): the separation case."""
    rng = np.random.default_rng(seed)
    n = 2 * n_each
    c = np.where(np.arange(n) < n_each, -0.6, 0.6)
    means = np.stack([c + rng.normal(0, 0.08, n), rng.normal(0, 0.15, n), rng.normal(0, 0.1, n)], 1).astype(np.float32)
    gid = (np.arange(n) >= n_each).astype(np.uint8)
    Rt = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(1, 12), (2, 1)).astype(np.float32)
    return dict(means=means, op=rng.uniform(0.5, 0.95, n).astype(np.float32), colors=rng.uniform(0, 1, (n, 3)).astype(np.float32), sh=-1,
                quats=np.tile(np.array([1.0, 0, 0, 0], np.float32), (n, 1)), scales=np.full((n, 3), scale, np.float32), cov6=None,
                gid=gid, G=2, Rt=Rt)
