"""The yardstick of MCMC density control ("MCMC density control"): sas_scene_mcmc_noise and sas_scene_mcmc_refine restated in
numpy.

A scene is a dict of the arrays in the caller's order: ``means [n,3]``, ``opacities [n]``, ``colors [n,K,3]``, ``quats [n,4]``, ``scales [n,3]``
(or ``covariances [n,6]``) and ``gid [n]`` (uint8) or None.  A config is a dict under the keys of ``Rasterizer.mcmc_refine``.

The SAMPLING is integer arithmetic and exact: weights ``uint32(o 2^24)``, their uint64 prefix, 64-bit uniforms of the generator, targets
``(u total) >> 64`` as Python integers, ``searchsorted(side="right")``, ``bincount``.  ``decide`` ASSERTS that no opacity of the case sits
within a factor two of ``min_opacity``: inside that condition the alive set of any float32 evaluation is the same.

The RELOCATION is parametrised by ``dtype``: float64 is the contract (a binary64 sum in a fixed order, ``o'`` and ``o / denom`` rounded
once to float32 where the scene is float32); float32 evaluates everything in float32 (pow and sqrt the float64 functions rounded) to
measure what float32 alone would cost.  The NOISE likewise: float64 for the reference, float32 operation by operation."""
import numpy as np

from densify_ref import TWO_PI_F32, mix32

CONFIG = dict(min_opacity=0.005, cap_max=1_000_000, grow_factor=1.05, seed=0)
GOLDEN = 0x9e3779b9
MAX_N = 51
_M = np.uint64(0xffffffff)
FLT_EPSILON = float(np.finfo(np.float32).eps)


def _binomials():
    """C(n, k) for n, k < 51 as Python integers (every one below 2^53)."""
    rows = [[1]]
    for n in range(1, MAX_N):
        prev = rows[-1]
        rows.append([1] + [prev[k - 1] + (prev[k] if k < n else 0) for k in range(1, n + 1)])
    return rows


BINOM = _binomials()


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _normal_from(base, c, dtype):
    """Box-Muller on the hashes of (base, c + 1) and (base, c + 2), as densify_ref.normals."""
    dt = np.dtype(dtype).type
    h1 = mix32(base ^ (((c + np.uint64(1)) * np.uint64(GOLDEN)) & _M))
    h2 = mix32(base ^ (((c + np.uint64(2)) * np.uint64(GOLDEN)) & _M))
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = lambda a: np.asarray(a, np.float64).astype(dt)
    lg = r(np.log(r(u1).astype(np.float64)))
    rad = r(np.sqrt(r(dt(-2.0) * lg).astype(np.float64)))
    ang = r(dt(TWO_PI_F32) * r(u2))
    return r(rad * r(np.cos(ang.astype(np.float64))))


def noise_normals(seed, step, index, dtype=np.float64):
    """Standard normals ``[n,3]`` keyed by (seed, step, index, axis)."""
    index = np.asarray(index, np.uint64).reshape(-1, 1)
    base = mix32(mix32(mix32(np.uint64(int(seed) & 0xffffffff) ^ np.uint64(GOLDEN)) + np.uint64(int(step) & 0xffffffff)) + index)
    c = (2 * np.arange(3).reshape(1, 3)).astype(np.uint64)
    return _normal_from(base, c, dtype)


def draw_uniforms(seed, draws):
    """The 64-bit uniforms of draws 0 .. draws-1 as Python integers."""
    d = np.arange(int(draws), dtype=np.uint64)
    base = mix32(mix32(np.uint64(int(seed) & 0xffffffff) ^ np.uint64(GOLDEN)) + d)
    hi, lo = mix32(base ^ np.uint64(GOLDEN)), mix32(base ^ np.uint64((2 * GOLDEN) & 0xffffffff))
    return [(int(a) << 32) | int(b) for a, b in zip(hi, lo)]


# ---- noise --------------------------------------------------------------------------------------------------------------------------
def covariances(scene, dtype):
    """C = M M^T, M = R(q / |q|) diag(s), ``[n,3,3]`` in ``dtype`` -- or the stored covariances of a cov6 scene."""
    dt = np.dtype(dtype).type
    if scene.get("covariances") is not None:
        c = np.asarray(scene["covariances"]).astype(dt)
        return np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], axis=1).reshape(-1, 3, 3)
    q, s = np.asarray(scene["quats"]).astype(dt), np.asarray(scene["scales"]).astype(dt)
    one = dt(1)
    inorm = one / np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))
    M = quat_to_rotmat_unit(q * inorm[:, None]) * s[:, None, :]
    C = np.empty((q.shape[0], 3, 3), dt)
    for r in range(3):
        for c in range(3):
            C[:, r, c] = (M[:, r, 0] * M[:, c, 0] + M[:, r, 1] * M[:, c, 1]) + M[:, r, 2] * M[:, c, 2]
    return C


def quat_to_rotmat_unit(q):
    """R of unit wxyz rows, in q's dtype (the kernel normalises by one multiplication with 1 / |q|)."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def noise(scene, scale, step, seed, dtype=np.float64):
    """The means after sas_scene_mcmc_noise, ``[n,3]`` in ``dtype``; a Gaussian whose gate is not positive keeps its mean."""
    dt = np.dtype(dtype).type
    m, o = np.asarray(scene["means"]).astype(dt), np.asarray(scene["opacities"]).astype(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((dt(-100.0) * ((dt(1) - o) - dt(np.float32(0.995)))).astype(np.float64)).astype(dt)
        g = dt(1) / (dt(1) + e)
    xi = noise_normals(seed, step, np.arange(m.shape[0]), dt)
    n = (xi * g[:, None]) * dt(np.float32(scale))
    C = covariances(scene, dt)
    d = np.stack([(C[:, k, 0] * n[:, 0] + C[:, k, 1] * n[:, 1]) + C[:, k, 2] * n[:, 2] for k in range(3)], axis=1)
    out = np.where((g > 0)[:, None], m + d, m)
    assert out.dtype == np.dtype(dt)
    return out


# ---- refine -------------------------------------------------------------------------------------------------------------------------
def grow_count(n, cap_max, grow_factor):
    """n_grow = max(0, min(cap_max, floor(grow_factor n)) - n), the product in binary64."""
    return max(0, min(int(cap_max), int(np.floor(float(grow_factor) * float(n)))) - int(n))


def decide(opacities, min_opacity):
    """(alive [n] bool, weights [n] uint64); asserts the factor two."""
    o = np.asarray(opacities, np.float32)
    thr = np.float32(min_opacity)
    v = o.astype(np.float64)
    bad = (v > 0.5 * float(thr)) & (v < 2.0 * float(thr))
    assert not bad.any(), (float(thr), v[bad][:4])
    with np.errstate(invalid="ignore"):
        alive = o > thr
    w = np.where(alive, (np.minimum(np.where(alive, o, np.float32(0)), np.float32(1)) * np.float32(16777216.0)).astype(np.uint64), np.uint64(0)).astype(np.uint64)
    return alive, w


def sample(weights, draws, seed):
    """(source [draws] int64, copies [n] int64): draw d selects the i with P_(i-1) <= (u_d total) >> 64 < P_i."""
    P = np.cumsum(np.asarray(weights, np.uint64), dtype=np.uint64)
    total = int(P[-1])
    t = np.array([(u * total) >> 64 for u in draw_uniforms(seed, draws)], dtype=np.uint64)
    src = np.searchsorted(P, t, side="right").astype(np.int64)
    return src, np.bincount(src, minlength=len(P)).astype(np.int64)


def relocate(o, copies, min_opacity, scales, dtype=np.float64):
    """gsplat's compute_relocation for the sources: (o' [m] float32, scale' [m,3] float32, o' and o / denom unrounded in ``dtype``).
    float64: the contract.  float32: every operation in float32."""
    dt = np.dtype(dtype).type
    o32 = np.asarray(o, np.float32)
    n = np.minimum(np.asarray(copies, np.int64) + 1, MAX_N)
    od = o32.astype(dt)
    with np.errstate(all="ignore"):
        on = (dt(1) - np.power((dt(1) - od).astype(np.float64), (dt(1) / n.astype(dt)).astype(np.float64)).astype(dt)).astype(dt)
    denom = np.zeros_like(od)
    for nn in np.unique(n):
        sel = n == nn
        x, acc = on[sel], np.zeros(int(sel.sum()), dt)
        for i in range(1, int(nn) + 1):
            p = x.copy()
            for k in range(i):
                term = (dt(BINOM[i - 1][k]) * (-p if k & 1 else p)) / dt(np.sqrt(np.float64(k + 1)))
                acc = (acc + term).astype(dt)
                p = (p * x).astype(dt)
        denom[sel] = acc
    with np.errstate(all="ignore"):
        ratio = od / denom
    o_new = np.minimum(np.maximum(on.astype(np.float32), np.float32(min_opacity)), np.float32(1.0 - FLT_EPSILON)).astype(np.float32)
    s_new = (ratio.astype(np.float32)[:, None] * np.asarray(scales, np.float32)).astype(np.float32)
    return o_new, s_new, on, ratio


def refine(scene, cfg, dtype=np.float64, decide_on=None):
    """The new scene, ``parents``, the counts, and which new rows are fresh.  ``decide_on``: opacities the DECISIONS (alive, weights, draws)
    are taken from in place of the scene's own -- the float32 values a device holds, where ``scene`` is a float64 restatement of them."""
    cf = dict(CONFIG, **cfg)
    o_dec = np.asarray(scene["opacities"] if decide_on is None else decide_on).astype(np.float32)
    alive, w = decide(o_dec, cf["min_opacity"])
    n = alive.shape[0]
    n_alive = int(alive.sum())
    assert n_alive > 0
    n_dead, n_grow = n - n_alive, grow_count(n, cf["cap_max"], cf["grow_factor"])
    D = n_dead + n_grow
    keys = ("means", "opacities", "colors", "quats", "scales")
    if D == 0:
        new = {k: np.asarray(scene[k]).copy() for k in keys}
        new["gid"] = None if scene.get("gid") is None else np.asarray(scene["gid"]).copy()
        return dict(scene=new, parents=np.arange(n, dtype=np.int32), n=n, relocated=0, added=0, n_alive=n, fresh=np.zeros(n, bool),
                    copies=np.zeros(n, np.int64), source=np.zeros(0, np.int64), rel=None)
    src, copies = sample(w, D, cf["seed"])
    alive_i = np.flatnonzero(alive)
    parents = np.concatenate([alive_i, src]).astype(np.int32)
    new = {k: np.asarray(scene[k])[parents].copy() for k in keys}
    new["gid"] = None if scene.get("gid") is None else np.asarray(scene["gid"])[parents].copy()
    fresh = copies[parents] > 0
    sources = np.flatnonzero(copies > 0)
    o_new, s_new, on, ratio = relocate(np.asarray(scene["opacities"])[sources], copies[sources], cf["min_opacity"], np.asarray(scene["scales"])[sources], dtype)
    where = np.searchsorted(sources, parents[fresh])
    new["opacities"] = new["opacities"].astype(np.asarray(scene["opacities"]).dtype)
    new["opacities"][fresh] = o_new[where]
    new["scales"][fresh] = s_new[where]
    return dict(scene=new, parents=parents, n=n_alive + D, relocated=n_dead, added=n_grow, n_alive=n_alive, fresh=fresh, copies=copies, source=src,
                rel=dict(sources=sources, opacity=on, ratio=ratio, o_new=o_new, s_new=s_new))


def carry_state(S, res, fit_ref):
    """fit_ref's state ``S`` of the old scene carried to the new one of ``res``: rows that are not fresh keep activated values, moments and
    raw values; sources and children start from zero moments and the raw values of their new activated values."""
    dt, p, fresh = S["dt"], res["parents"], res["fresh"]
    new = res["scene"]
    T = dict(x={k: np.asarray(new[k]).astype(dt) for k in S["x"]}, m={}, v={}, raw={}, dt=dt, n=res["n"])
    T["x"]["colors"] = T["x"]["colors"].reshape(res["n"], -1, 3)
    for k in S["x"]:   # what is inherited is the state's own value, not its float32 rounding
        keep = ~fresh if k in ("opacities", "scales") else np.ones(len(p), bool)
        T["x"][k][keep] = S["x"][k][p[keep]]
    for k in S["m"]:
        for name in ("m", "v"):
            a = S[name][k][p].copy()
            a[fresh] = 0
            T[name][k] = a
        if k in S["raw"]:
            raw = S["raw"][k][p].copy()
            raw[fresh] = fit_ref.inverse_activation(k, T["x"][k][fresh], dt)
            T["raw"][k] = raw
    return T
