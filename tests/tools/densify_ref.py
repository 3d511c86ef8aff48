"""The yardstick of density control ("Density control"): sas_density_accumulate and sas_scene_densify restated in numpy.

A scene is a dict of the arrays in the caller's order: ``means [n,3]``, ``opacities [n]``, ``colors [n,K,3]``, ``quats [n,4]``, ``scales [n,3]``
(float32) and ``gid [n]`` (uint8) or None.  A config is a dict under the keys of ``Rasterizer.densify``.  ``densify`` returns the new scene
(survivors, clones, pairs of children), ``parents``, the counts, and the class of every old Gaussian; ``dtype`` is the arithmetic of the
children's means: float64 for the reference, float32 (every operation rounded, log / cos / sqrt the float64 functions rounded) to measure
what float32 alone costs.  Everything else is a copy or one float32 division and is the same in both.

``decide`` ASSERTS that no decision of the case sits near a threshold (a factor two on either side): inside that condition the decisions of
any float32 evaluation are the same, so the GPU's must be exact."""
import numpy as np

CONFIG = dict(grow_grad2d=2e-4, grow_scale3d=0.01, prune_opacity=0.005, prune_scale3d=0.1, scene_extent=1.0, split_factor=1.6, max_gaussians=0,
              seed=0, grow=True, prune_opacity_on=True, prune_scale_on=True)
TWO_PI_F32 = float(np.float32(6.2831855))
_M = np.uint64(0xffffffff)


def mix32(x):
    """The generator's integer hash on uint32 values (kept in uint64 arrays, reduced modulo 2^32)."""
    x = np.asarray(x, np.uint64) & _M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & _M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & _M
    x ^= x >> np.uint64(16)
    return x


def uniforms(seed, parents):
    """(u1, u2) float64 ``[P,2,3]``: u1 in (0, 1], u2 in [0, 1), multiples of 2^-24, for (parent, child, axis)."""
    parents = np.asarray(parents, np.uint64).reshape(-1, 1, 1)
    base = mix32(mix32(np.uint64(int(seed) & 0xffffffff) ^ np.uint64(0x9e3779b9)) + parents)
    c = (2 * (3 * np.arange(2).reshape(1, 2, 1) + np.arange(3).reshape(1, 1, 3))).astype(np.uint64)
    h1 = mix32(base ^ (((c + np.uint64(1)) * np.uint64(0x9e3779b9)) & _M))
    h2 = mix32(base ^ (((c + np.uint64(2)) * np.uint64(0x9e3779b9)) & _M))
    return ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24, (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normals(seed, parents, dtype=np.float64):
    """Standard normals ``[P,2,3]`` by Box-Muller: sqrt(-2 log u1) cos(2 pi u2), 2 pi the float32 constant."""
    dt = np.dtype(dtype).type
    u1, u2 = uniforms(seed, parents)
    r = lambda a: np.asarray(a, np.float64).astype(dt)   # round to the arithmetic's format
    lg = r(np.log(r(u1).astype(np.float64)))
    rad = r(np.sqrt(r(dt(-2.0) * lg).astype(np.float64)))
    ang = r(dt(TWO_PI_F32) * r(u2))
    return r(rad * r(np.cos(ang.astype(np.float64))))


def accumulate(stats, d_means2d, radii, W, H):
    """One view added to ``stats`` (a dict of grad_sum, count, max_radius; changed in place), in float32 operation by operation:
    ``d_means2d [n,2]`` float32, ``radii [n,2]`` int32 as read_projection reports them."""
    d = np.asarray(d_means2d, np.float32)
    radii = np.asarray(radii)
    vis = radii[:, 0] > 0
    gx, gy = np.float32(0.5 * W) * d[:, 0], np.float32(0.5 * H) * d[:, 1]
    norm = np.sqrt(gx * gx + gy * gy, dtype=np.float32)
    stats["grad_sum"] = np.where(vis, stats["grad_sum"] + norm, stats["grad_sum"]).astype(np.float32)
    stats["count"] = (stats["count"] + vis).astype(np.int32)
    stats["max_radius"] = np.where(vis, np.maximum(stats["max_radius"], radii.max(axis=1).astype(np.float32)), stats["max_radius"]).astype(np.float32)
    return stats


def _apart(v, thr, what):
    """No value within a factor two of the threshold."""
    v = np.asarray(v, np.float64)
    bad = (v > 0.5 * thr) & (v < 2.0 * thr)
    assert not bad.any(), (what, thr, v[bad][:4])


def decide(scene, stats, cfg):
    """(pruned, clone candidates, split candidates) of the old set, boolean ``[n]``."""
    cf = dict(CONFIG, **cfg)
    f32 = np.float32
    op, smax = np.asarray(scene["opacities"], f32), np.asarray(scene["scales"], f32).max(axis=1)
    cnt = np.asarray(stats["count"], np.int32)
    avg = np.asarray(stats["grad_sum"], f32) / np.maximum(cnt, 1).astype(f32)
    grow_scale, prune_scale = f32(cf["grow_scale3d"]) * f32(cf["scene_extent"]), f32(cf["prune_scale3d"]) * f32(cf["scene_extent"])
    n = op.shape[0]
    no = np.zeros(n, bool)
    if cf["grow"]:
        _apart(avg[cnt > 0], float(f32(cf["grow_grad2d"])), "avg")
        _apart(smax, float(grow_scale), "grow_scale")
    if cf["prune_scale_on"]:
        _apart(smax, float(prune_scale), "prune_scale")
    if cf["prune_opacity_on"]:
        _apart(op, float(f32(cf["prune_opacity"])), "prune_opacity")
    high = (cnt > 0) & (avg > f32(cf["grow_grad2d"])) if cf["grow"] else no
    small = smax <= grow_scale
    prune_o = op < f32(cf["prune_opacity"]) if cf["prune_opacity_on"] else no
    prune_s = smax > prune_scale if cf["prune_scale_on"] else no
    pruned = prune_o | (prune_s & ~(high & ~small))
    return pruned, high & small & ~pruned, high & ~small & ~pruned


def plan(kept, clone_cand, split_cand, max_gaussians):
    """(survivors, clones, splits, n_new): the growth budget under the cap, clones first."""
    budget = clone_cand + split_cand
    if max_gaussians > 0:
        budget = min(budget, max(max_gaussians - kept, 0))
    clones = min(clone_cand, budget)
    splits = min(split_cand, budget - clones)
    return kept - splits, clones, splits, kept - splits + clones + 2 * splits


def quat_to_rotmat(q):
    """R(q / |q|) for wxyz rows, in q's dtype."""
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def children_means(scene, parents, seed, dtype=np.float64):
    """``[P,2,3]``: mean + R(q / |q|) (scale * xi) of both children of each parent."""
    dt = np.dtype(dtype).type
    p = np.asarray(parents, np.int64)
    m, s, q = (np.asarray(scene[k])[p].astype(dt) for k in ("means", "scales", "quats"))
    d = s[:, None, :] * normals(seed, p, dt)
    out = m[:, None, :] + np.einsum("pij,pcj->pci", quat_to_rotmat(q), d)
    assert out.dtype == np.dtype(dt)
    return out


def densify(scene, stats, cfg, dtype=np.float64):
    cf = dict(CONFIG, **cfg)
    pruned, clone_c, split_c = decide(scene, stats, cf)
    n = pruned.shape[0]
    n_surv, n_clone, n_split, n_new = plan(int((~pruned).sum()), int(clone_c.sum()), int(split_c.sum()), int(cf["max_gaussians"]))
    cloned = clone_c & (np.cumsum(clone_c) - clone_c < n_clone)
    split = split_c & (np.cumsum(split_c) - split_c < n_split)
    surv_i, clone_i, split_i = np.flatnonzero(~pruned & ~split), np.flatnonzero(cloned), np.flatnonzero(split)
    assert len(surv_i) == n_surv and len(clone_i) == n_clone and len(split_i) == n_split
    parents = np.concatenate([surv_i, clone_i, np.repeat(split_i, 2)]).astype(np.int32)
    new = {k: np.asarray(scene[k])[parents].copy() for k in ("means", "opacities", "colors", "quats", "scales")}
    new["gid"] = None if scene.get("gid") is None else np.asarray(scene["gid"])[parents].copy()
    first = n_surv + n_clone
    kids = children_means(scene, split_i, cf["seed"], dtype).reshape(-1, 3)
    means = new["means"].astype(np.dtype(dtype))
    means[first:] = kids
    new["means"] = means
    sc = np.asarray(scene["scales"])   # (float32 scenes: one float32 division, the kernel's)
    new["scales"][first:] = sc[np.repeat(split_i, 2)] / sc.dtype.type(np.float32(cf["split_factor"]))
    return dict(scene=new, parents=parents, n=n_new, n_survivors=n_surv, cloned=n_clone, split=n_split, pruned=int(pruned.sum()),
                classes=dict(pruned=pruned, cloned=cloned, split=split))


def carry_state(S, res, fit_ref):
    """fit_ref's state ``S`` of the old scene carried to the new one of ``res``: the survivors keep moments and raw values, clones and
    children start from zero moments and the raw values of their new activated values.  ``x`` becomes the new scene in S's dtype."""
    dt, p, ns = S["dt"], res["parents"], res["n_survivors"]
    new = res["scene"]
    T = dict(x={k: np.asarray(new[k]).astype(dt) for k in S["x"]}, m={}, v={}, raw={}, dt=dt, n=res["n"])
    T["x"]["colors"] = T["x"]["colors"].reshape(res["n"], -1, 3)
    for k in S["x"]:   # the survivors' activated values are the state's own, not their float32 roundings
        T["x"][k][:ns] = S["x"][k][p[:ns]]
    for k in S["m"]:
        for name in ("m", "v"):
            a = S[name][k][p].copy()
            a[ns:] = 0
            T[name][k] = a
        if k in S["raw"]:
            raw = S["raw"][k][p].copy()
            raw[ns:] = fit_ref.inverse_activation(k, T["x"][k][ns:], dt)
            T["raw"][k] = raw
    return T
