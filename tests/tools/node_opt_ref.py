"""The numpy restatement of the node optimiser's two kernels (sas_nodes_rigidity, sas_nodes_twist_step; DESIGN.md 3, "Deformation": the node
optimiser), the cases the CPU and GPU tests share, and the two bounds they hold the device to.

``rigidity_gather`` is k_nodes_rigidity's form in float64 numpy: every node sums its own edges in slot order and then its incoming edges in the
reverse table's order, every residual recomputed from the two transforms.  ``rigidity_bound`` is the ROUNDING bound of such a sum, derived and not
measured: with every residual expanded into its eight products (three of ``R_i g``, ``t_i``, three of ``R_j g``, ``t_j``), an entry of the
gradient is a sum of ``terms = 8 (edges at the node)`` products and the value a sum of ``terms = 64 * 3 * edges`` products; whatever order the
sum is taken in and however the products are formed (a few roundings each), the result is within ``(terms + 4) 2^-53 sum |term|`` of the exact one.

``step_yardstick`` is the reference's OWN rounding error: ``deform._twist_step`` in float64 against the same operations in ``np.longdouble``,
per output array, floored at one unit in the last place (binary64) of the array's largest magnitude.  The device is held to four times it.

    python tests/tools/node_opt_ref.py        # prints the yardstick table
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository: the cases run deform's host code
import knn_ref  # noqa: E402

U = 2.0 ** -53


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------
def knn_table(nodes, neighbours: int = 6) -> np.ndarray:
    """``[M,k]`` int32, ``k = min(neighbours, M - 1)``: Rasterizer.knn_points' table of the nodes, by knn_ref's restatement of its contract
    (float32 d2, ties to the lower index, the node itself left out by index)."""
    g = np.ascontiguousarray(np.asarray(nodes, np.float32).reshape(-1, 3))
    k = int(min(neighbours, g.shape[0] - 1))
    if k <= 0:
        return np.zeros((g.shape[0], 0), np.int32)
    return np.ascontiguousarray(knn_ref.knn_ref(g, k)[1].astype(np.int32))


def reverse_table(nb):
    """``(rev_start [M+1], rev_edge [M*k])`` int32: for node j the edge numbers ``i * k + slot`` with ``nb[i, slot] == j``, ascending; entries
    outside ``[0, M)`` name nobody; -1 behind the last edge.  Per node, with np.nonzero: not deform.reverse_table's sort."""
    nb = np.asarray(nb)
    M = nb.shape[0]
    flat = nb.reshape(-1)
    lists = [np.nonzero(flat == j)[0] for j in range(M)]
    rev_start = np.zeros(M + 1, np.int32)
    rev_start[1:] = np.cumsum([len(x) for x in lists])
    rev_edge = np.full(flat.size, -1, np.int32)
    if lists and rev_start[-1]:
        rev_edge[:rev_start[-1]] = np.concatenate(lists)
    return rev_start, rev_edge


# ---- the rigidity kernel ------------------------------------------------------------------------------------------------------------------------
def _apply(T, g):
    """``T(g)`` as the kernel forms it: ((R0 gx + R1 gy) + R2 gz) + t per row."""
    return ((T[:, 0] * g[0] + T[:, 1] * g[1]) + T[:, 2] * g[2]) + T[:, 3]


def rigidity_gather(nodes, T, nb, rev=None):
    """``(value, d_T [M,3,4])`` float64 in k_nodes_rigidity's gather form and order."""
    g = np.asarray(nodes, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3, 4)
    nb = np.asarray(nb).reshape(g.shape[0], -1)
    M, kn = nb.shape
    d = np.zeros((M, 3, 4))
    if kn == 0:
        return 0.0, d
    rev_start, rev_edge = reverse_table(nb) if rev is None else rev
    scale2 = 2.0 * (1.0 / (M * kn))
    own = np.zeros(M)
    for i in range(M):
        for s in range(kn):
            j = int(nb[i, s])
            if j < 0 or j >= M:
                continue
            r = _apply(T[i], g[j]) - _apply(T[j], g[j])
            own[i] = own[i] + ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
            dr = scale2 * r
            d[i, :, :3] = d[i, :, :3] + dr[:, None] * g[j][None, :]
            d[i, :, 3] = d[i, :, 3] + dr
        for p in range(int(rev_start[i]), int(rev_start[i + 1])):
            k = int(rev_edge[p]) // kn
            dr = scale2 * (_apply(T[k], g[i]) - _apply(T[i], g[i]))
            d[i, :, :3] = d[i, :, :3] - dr[:, None] * g[i][None, :]
            d[i, :, 3] = d[i, :, 3] - dr
    return float(own.sum() * (1.0 / (M * kn))), d


def rigidity_bound(nodes, T, nb):
    """``(value bound, gradient bound [M,3,4])``: ``(terms + 4) 2^-53 sum |term|`` per entry, see the module's text."""
    g = np.abs(np.asarray(nodes, np.float32).astype(np.float64).reshape(-1, 3))
    A = np.abs(np.asarray(T, np.float64).reshape(-1, 3, 4))
    nb = np.asarray(nb).reshape(g.shape[0], -1).astype(np.int64)
    M, kn = nb.shape
    if kn == 0:
        return 0.0, np.zeros((M, 3, 4))
    live = (nb >= 0) & (nb < M)
    j = np.where(live, nb, 0)
    gj = g[j]                                                                                     # [M,k,3]
    mag = lambda R, t: np.einsum("...ab,...b->...a", R, gj) + t                                    # sum of the four |products| of a row
    S = (mag(A[:, None, :, :3], A[:, None, :, 3]) + mag(A[j][..., :3], A[j][..., 3])) * live[..., None]   # [M,k,3]: the eight of a residual
    scale = 1.0 / (M * kn)
    value = (64.0 * 3.0 * live.sum() + 4.0) * U * scale * float((S * S).sum())
    lever = np.concatenate([gj, np.ones_like(gj[..., :1])], axis=2)                              # [M,k,4]: |g_j|, 1
    per_edge = 2.0 * scale * S[..., :, None] * lever[..., None, :]                                # [M,k,3,4]
    total = per_edge.sum(axis=1)
    np.add.at(total, j.reshape(-1), (per_edge * live[..., None, None]).reshape(-1, 3, 4))
    degree = live.sum(axis=1) + np.bincount(j[live].reshape(-1), minlength=M)
    return value, (8.0 * degree[:, None, None] + 4.0) * U * total


def rigid_transforms(rng, m: int, angle: float = 0.5, shift: float = 0.3) -> np.ndarray:
    """``[m,3,4]`` float64 rigid transforms, rotations by up to ``angle`` rad about drawn axes, translations up to ``shift``."""
    from sim_a_splat_amd import deform
    xi = np.concatenate([rng.normal(size=(m, 3)), rng.uniform(-shift, shift, (m, 3))], axis=1)
    xi[:, :3] *= (rng.uniform(0.0, angle, m) / np.linalg.norm(xi[:, :3], axis=1))[:, None]
    return np.ascontiguousarray(deform.se3_exp_batch(xi)[:, :3, :])


def _drawn(m, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (m, 3)).astype(np.float32)


def _hub(m=300):
    """Drawn nodes and a table SET BY HAND: node 0 is the one neighbour of every other node (and node 1 is node 0's), in-degree m - 1.  No
    point set has such a table (in three dimensions at most twelve points can have one centre as their nearest), but the kernel takes any
    table, and a lane that walks m - 1 incoming edges is the case."""
    nb = np.zeros((m, 1), np.int32)
    nb[0, 0] = 1
    return _drawn(m, 77), nb


RIGIDITY_CASES = {   # name -> (nodes, neighbours or the table itself)
    "m1": lambda: (np.array([[0.25, -0.5, 0.125]], np.float32), 6),
    "m2": lambda: (np.array([[0.0, 0.0, 0.0], [0.5, 0.25, -0.125]], np.float32), 6),
    "grid3x3": lambda: (grid3x3(), 6),
    "drawn257": lambda: (_drawn(257, 11), 6),
    "drawn2049": lambda: (_drawn(2049, 12), 6),
    "hub300": _hub,
}


def grid3x3() -> np.ndarray:
    """The recovery case's nodes (skin_grad_ref.recovery_case): a 3x3 grid of spacing 0.5 x 0.4 -- exact ties."""
    from sim_a_splat_amd import deform
    return deform.grid_nodes(((-0.5, -0.4, 0.0), (0.5, 0.4, 0.0)), 0.5)


@functools.lru_cache(maxsize=None)
def rigidity_case(name: str) -> dict:
    """``nodes``, the knn table ``nb`` with its reverse ``rev``, drawn rigid ``T`` and the host's ``value`` / ``grad`` (deform.rigidity(table=))
    with the derived bounds."""
    from sim_a_splat_amd import deform
    nodes, neighbours = RIGIDITY_CASES[name]()
    nb = knn_table(nodes, neighbours) if np.isscalar(neighbours) else neighbours
    T = rigid_transforms(np.random.default_rng(1000 + sorted(RIGIDITY_CASES).index(name)), nodes.shape[0])
    value, grad = deform.rigidity(nodes, T, table=nb)
    vb, gb = rigidity_bound(nodes, T, nb)
    return dict(nodes=nodes, nb=nb, rev=reverse_table(nb), T=T, value=value, grad=grad, value_bound=vb, grad_bound=gb)


# ---- the step kernel ----------------------------------------------------------------------------------------------------------------------------
def _se3_exp_long(xi):
    """deform.se3_exp_batch's operations on ``np.longdouble``."""
    L = np.longdouble
    w, v = xi[:, :3], xi[:, 3:]
    th = np.sqrt((w * w).sum(axis=1))
    small = th < L(1e-8)
    ths = np.where(small, L(1), th)
    A = np.where(small, L(1) - th * th / L(6), np.sin(ths) / ths)
    B = np.where(small, L(0.5) - th * th / L(24), (L(1) - np.cos(ths)) / (ths * ths))
    C = np.where(small, L(1) / L(6) - th * th / L(120), (ths - np.sin(ths)) / ths ** 3)
    Wx = np.zeros((xi.shape[0], 3, 3), L)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    W2 = np.einsum("mab,mbc->mac", Wx, Wx)
    I = np.eye(3, dtype=L)
    ER = I + A[:, None, None] * Wx + B[:, None, None] * W2
    Et = np.einsum("mab,mb->ma", I + B[:, None, None] * Wx + C[:, None, None] * W2, v)
    return ER, Et


def twist_step_long(T, dT, g, m1, m2, it, per, step):
    """deform._twist_step's operations on ``np.longdouble`` (the constants are the doubles the float64 code holds, widened)."""
    L = np.longdouble
    T, dT, g, m1, m2 = (np.asarray(a, np.float64).astype(L) for a in (T, dT, g, m1, m2))
    piv = np.einsum("mab,mb->ma", T[:, :, :3], g) + T[:, :, 3]
    tw = np.zeros((T.shape[0], 6), L)
    tw[:, :3] = np.cross(T.transpose(0, 2, 1), dT.transpose(0, 2, 1)).sum(axis=1)
    tw[:, 3:] = dT[:, :, 3]
    tw[:, :3] += np.cross(tw[:, 3:], piv)
    m1 = L(0.9) * m1 + L(0.1) * tw
    m2 = L(0.999) * m2 + L(0.001) * tw * tw
    hat = (m1 / L(1 - 0.9 ** (it + 1))) / (np.sqrt(m2 / L(1 - 0.999 ** (it + 1))) + L(1e-12))
    decay = L(0.05 ** (it / max(1, per - 1)))
    ER, Et = _se3_exp_long(-np.concatenate([L(step[0]) * decay * hat[:, :3], L(step[1]) * decay * hat[:, 3:]], axis=1))
    Rn = np.einsum("mab,mbc->mac", ER, T[:, :, :3])
    tn = np.einsum("mab,mb->ma", ER, T[:, :, 3] - piv) + Et + piv
    return np.concatenate([Rn, tn[:, :, None]], axis=2), m1, m2


def twist_step_kernel(T, d32, d64, weight, g, m1, m2, lr, c1, c2, beta1=0.9, beta2=0.999, gain1=0.1, gain2=0.001, eps=1e-12):
    """k_nodes_twist_step in float64 numpy, its operations in its order: ``(T, m1, m2, T32)`` after the step.  ``d32`` or ``d64`` may be None."""
    T, g, m1, m2 = (np.asarray(a, np.float64) for a in (T, g, m1, m2))
    R, t = T[:, :, :3], T[:, :, 3]
    p = ((R[:, :, 0] * g[:, None, 0] + R[:, :, 1] * g[:, None, 1]) + R[:, :, 2] * g[:, None, 2]) + t
    G = np.asarray(d32, np.float32).astype(np.float64) if d64 is None else weight * np.asarray(d64, np.float64) if d32 is None else \
        np.asarray(d32, np.float32).astype(np.float64) + weight * np.asarray(d64, np.float64)
    tw = np.zeros((T.shape[0], 6))
    for c in range(4):
        a0, a1, a2, b0, b1, b2 = T[:, 0, c], T[:, 1, c], T[:, 2, c], G[:, 0, c], G[:, 1, c], G[:, 2, c]
        x = np.stack([a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0], axis=1)
        tw[:, :3] = x if c == 0 else tw[:, :3] + x
    tw[:, 3:] = G[:, :, 3]
    v = tw[:, 3:]
    tw[:, :3] = tw[:, :3] + np.stack([v[:, 1] * p[:, 2] - v[:, 2] * p[:, 1], v[:, 2] * p[:, 0] - v[:, 0] * p[:, 2], v[:, 0] * p[:, 1] - v[:, 1] * p[:, 0]], axis=1)
    m1 = beta1 * m1 + gain1 * tw
    m2 = beta2 * m2 + (gain2 * tw) * tw
    hat = (m1 / c1) / (np.sqrt(m2 / c2) + eps)
    xi = -(np.array([lr[0]] * 3 + [lr[1]] * 3) * hat)
    w = xi[:, :3]
    th = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    C = np.where(small, 1.0 / 6.0 - th * th / 120.0, (ths - np.sin(ths)) / ((ths * ths) * ths))
    Wx = np.zeros((T.shape[0], 3, 3))
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    mul = lambda X, Y: (X[:, :, 0, None] * Y[:, None, 0, :] + X[:, :, 1, None] * Y[:, None, 1, :]) + X[:, :, 2, None] * Y[:, None, 2, :]
    W2 = mul(Wx, Wx)
    I = np.eye(3)
    ER = (I + A[:, None, None] * Wx) + B[:, None, None] * W2
    V = (I + B[:, None, None] * Wx) + C[:, None, None] * W2
    dot = lambda X, y: (X[:, :, 0] * y[:, None, 0] + X[:, :, 1] * y[:, None, 1]) + X[:, :, 2] * y[:, None, 2]
    Et = dot(V, xi[:, 3:])
    out = np.concatenate([mul(ER, R), ((dot(ER, t - p) + Et) + p)[:, :, None]], axis=2)
    return out, m1, m2, out.astype(np.float32)


def _ulp_of_largest(a) -> float:
    return float(np.spacing(np.abs(np.asarray(a, np.float64)).max()))


STEP_CASES = {   # name -> (M, it, per, drawn moments?, gradient magnitudes (log10 range), a node with a zero gradient?)
    "first_m1": (1, 0, 30, False, (-3, -1), False),
    "first_m257": (257, 0, 30, False, (-3, -1), False),
    "mid_m257": (257, 17, 30, True, (-3, -1), False),
    "zero_node_m257": (257, 0, 30, False, (-3, -1), True),
    "wide_m2049": (2049, 5, 30, True, (-8, 3), True),
}


@functools.lru_cache(maxsize=None)
def step_case(name: str) -> dict:
    """One step from a given state: ``nodes`` float32, ``T`` rigid float64, ``d32`` float32 and ``d64`` float64 gradients with ``weight``,
    the moments, ``it`` / ``per`` / ``step``; ``ref``: (T, m1, m2) of deform._twist_step on ``double(d32) + weight * d64``."""
    from sim_a_splat_amd import deform
    M, it, per, moments, (lo, hi), zero = STEP_CASES[name]
    rng = np.random.default_rng(2000 + sorted(STEP_CASES).index(name))
    nodes = rng.uniform(-1.0, 1.0, (M, 3)).astype(np.float32)
    T = rigid_transforms(rng, M)
    mag = 10.0 ** rng.uniform(lo, hi, (M, 1, 1))
    d32 = (rng.normal(size=(M, 3, 4)) * mag).astype(np.float32)
    d64 = rng.normal(size=(M, 3, 4)) * mag
    m1, m2 = np.zeros((M, 6)), np.zeros((M, 6))
    if moments:
        m1 = rng.normal(size=(M, 6)) * mag[:, 0]
        m2 = (rng.uniform(0.5, 2.0, (M, 6)) * mag[:, 0]) ** 2
    if zero:
        d32[M // 2], d64[M // 2], m1[M // 2], m2[M // 2] = 0.0, 0.0, 0.0, 0.0
    c = dict(nodes=nodes, T=T, d32=d32, d64=d64, weight=0.01, m1=m1, m2=m2, it=it, per=per, step=(0.01, 0.01))
    c["dT"] = d32.astype(np.float64) + c["weight"] * d64
    c["ref"] = deform._twist_step(T, c["dT"], nodes.astype(np.float64), m1, m2, it, per, c["step"])
    return c


def step_yardstick(c: dict) -> dict:
    """``{"T", "m1", "m2"}`` -> the largest error of deform._twist_step in float64 against ``twist_step_long``, floored at one unit in the
    last place (binary64) of the array's largest magnitude."""
    wide = twist_step_long(c["T"], c["dT"], c["nodes"].astype(np.float64), c["m1"], c["m2"], c["it"], c["per"], c["step"])
    out = {}
    for key, got, ref in zip(("T", "m1", "m2"), c["ref"], wide):
        err = float(np.abs(got.astype(np.longdouble) - ref).max())
        out[key] = max(err, _ulp_of_largest(got))
    return out


def step_ratios(c: dict, got_T, got_m1, got_m2) -> dict:
    """The device's (or anybody's) distance to ``c["ref"]`` per array, in yardsticks."""
    y = step_yardstick(c)
    return {key: float(np.abs(np.asarray(got, np.float64) - ref).max()) / y[key] for key, got, ref in zip(("T", "m1", "m2"), (got_T, got_m1, got_m2), c["ref"])}


if __name__ == "__main__":
    print("step_yardstick: deform._twist_step in float64 against np.longdouble (%d-bit significand), per array; floor = 1 ulp of the largest magnitude"
          % np.finfo(np.longdouble).nmant)
    for name in STEP_CASES:
        c = step_case(name)
        y = step_yardstick(c)
        print(f"  {name:16s} " + "  ".join(f"{k}: {y[k]:.2e} (floor {_ulp_of_largest(ref):.2e})" for k, ref in zip(("T", "m1", "m2"), c["ref"])))
    print("rigidity_bound: (terms + 4) 2^-53 sum |term|")
    for name in RIGIDITY_CASES:
        c = rigidity_case(name)
        v, d = rigidity_gather(c["nodes"], c["T"], c["nb"], c["rev"])
        print(f"  {name:10s} value {c['value']:.6e} bound {c['value_bound']:.2e} gather off by {abs(v - c['value']):.2e};  gradient: largest "
              f"|gather - host| / bound {np.max(np.abs(d - c['grad']) / np.maximum(c['grad_bound'], 1e-300)):.3f}")
