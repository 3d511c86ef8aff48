"""The numpy restatement of the per-node rigid fit on the device (sas_nodes_fit_rigid, k_nodes_fit_rigid; DESIGN.md 3, "Deformation": the node
driver), the cases the CPU and GPU tests share, their margins, and the bounds the device is held to.

``fit_ref(nodes, moved, table, dtype)`` is the kernel operation by operation, vectorised over the (step, node) lanes, for ``np.float64`` and
``np.longdouble``: members (the node, then its table entries in slot order; an entry outside [0, m) or with a non-finite moved position is left
out), centroids, the cross-covariance ``S`` summed in member order, Horn's 4x4 matrix, ``SWEEPS`` cyclic Jacobi sweeps (a pivot that is exactly zero
turns nothing: its tangent is set to 0, which is what the kernel does too), the projection of ``e0`` onto the span of the top eigenvectors, the
rotation of the unit quaternion and ``t = moved_i - R rest_i``.  Only ``+ - * /`` and ``sqrt``: in float64 it can agree with the device in every bit.

The YARDSTICK of a case is ``|fit_ref(float64) - fit_ref(longdouble)|`` per entry, the float64 restatement's own error, floored at one unit in the
last place of ``max(1, |entry|)``; the device is held to FOUR times it (the project's factor, as in node_opt_ref).

Every case's MARGINS are asserted here, so that no case sits on a threshold where float64 and longdouble may decide differently: an eigenvalue's
distance to the top one is either below 1e-3 of the threshold ``FIT_GAP * max |eigenvalue|`` or above 1e3 of it, and the squared norm of the
projection is either an exact zero (the half-turn case, by construction) or above 1e3 times ``HALF_TURN``.

    python tests/tools/node_fit_ref.py        # prints the table of yardsticks and margins
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import node_opt_ref as no  # noqa: E402

FIT_GAP = 1e-9        # SAS_NODES_FIT_GAP: eigenvalues within this times the largest |eigenvalue| of the top one span the quaternion's space
HALF_TURN = 1e-12     # SAS_NODES_FIT_HALF_TURN: a projection of e0 with a squared norm below this is an exact half turn
SWEEPS = 14           # SAS_NODES_FIT_SWEEPS: sweeps_needed over the kit's matrices (12) and drawn_matrices() (11) -- rank-one matrices both, whose
                      # double top eigenvalue converges linearly, halving per sweep -- plus two
MAX_K = 8
FLOOR = 4.0 * 2.0 ** -53   # "at the rounding floor": the largest off-diagonal entry is within four roundings of the largest |eigenvalue|
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ---- the kernel, restated -------------------------------------------------------------------------------------------------------------------------
def _members(nodes, moved, table):
    """``(idx [L,1+kn], live [L,1+kn], own_ok [L], a [M,3], b [S,M,3])``: every lane's members in the kernel's order."""
    a = np.ascontiguousarray(np.asarray(nodes, np.float32).reshape(-1, 3))
    b = np.asarray(moved, np.float32)
    b = np.ascontiguousarray(b.reshape((-1,) + a.shape))
    M, S = a.shape[0], b.shape[0]
    nb = np.zeros((M, 0), np.int64) if table is None else np.asarray(table).reshape(M, -1).astype(np.int64)
    fin = np.isfinite(b).all(axis=2)                                           # [S,M]
    inside = (nb >= 0) & (nb < M)
    j = np.where(inside, nb, 0)
    idx = np.concatenate([np.arange(M)[:, None], j], axis=1)                   # [M,1+kn]
    live = np.concatenate([np.ones((M, 1), bool), inside], axis=1)[None] & np.take_along_axis(fin[:, None, :].repeat(M, 1), idx[None].repeat(S, 0), axis=2)
    return idx, live, fin, a, b


def horn_matrix(S):
    """Horn's symmetric 4x4 matrix ``[L,4,4]`` of ``S [L,3,3]`` (``S[u][v] = sum a_u b_v``), the kernel's expressions."""
    N = np.zeros(S.shape[:-2] + (4, 4), S.dtype)
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[..., u, v] for u in range(3) for v in range(3))
    N[..., 0, 0] = (xx + yy) + zz
    N[..., 0, 1] = yz - zy
    N[..., 0, 2] = zx - xz
    N[..., 0, 3] = xy - yx
    N[..., 1, 1] = (xx - yy) - zz
    N[..., 1, 2] = xy + yx
    N[..., 1, 3] = zx + xz
    N[..., 2, 2] = (yy - xx) - zz
    N[..., 2, 3] = yz + zy
    N[..., 3, 3] = (zz - xx) - yy
    for p, q in PAIRS:
        N[..., q, p] = N[..., p, q]
    return N


def jacobi(N, sweeps: int = SWEEPS, trace=None):
    """``(eigenvalues [L,4], V [L,4,4])`` (columns) of the symmetric ``N [L,4,4]`` after ``sweeps`` cyclic Jacobi sweeps, the kernel's operations.
    ``trace``: a list that receives the largest |off-diagonal entry| per lane after every sweep."""
    dt = N.dtype.type
    A = N.copy()
    V = np.zeros_like(A)
    for k in range(4):
        V[..., k, k] = dt(1)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq, app, aqq = A[..., p, q].copy(), A[..., p, p].copy(), A[..., q, q].copy()
                theta = (aqq - app) / (dt(2) * apq)
                sgn = np.where(theta >= dt(0), dt(1), dt(-1))
                t = sgn / (np.abs(theta) + np.sqrt(theta * theta + dt(1)))
                t = np.where(apq == dt(0), dt(0), t)            # (an exactly zero pivot turns nothing; an overflowed theta gives 0 by itself)
                c = dt(1) / np.sqrt(t * t + dt(1))
                s = t * c
                A[..., p, p] = app - t * apq
                A[..., q, q] = aqq + t * apq
                A[..., p, q] = A[..., q, p] = dt(0)
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[..., r, p].copy(), A[..., r, q].copy()
                        A[..., r, p] = A[..., p, r] = c * arp - s * arq
                        A[..., r, q] = A[..., q, r] = s * arp + c * arq
                for r in range(4):
                    vrp, vrq = V[..., r, p].copy(), V[..., r, q].copy()
                    V[..., r, p] = c * vrp - s * vrq
                    V[..., r, q] = s * vrp + c * vrq
            if trace is not None:
                trace.append(np.max(np.abs(np.stack([A[..., p, q] for p, q in PAIRS], axis=-1)), axis=-1))
    return np.stack([A[..., k, k] for k in range(4)], axis=-1), V


def quaternion(lam, V):
    """``(q [L,4] wxyz, parts)``: the kernel's rule on the eigenvalues ``lam [L,4]`` and eigenvectors ``V [L,4,4]``."""
    dt = lam.dtype.type
    top = np.maximum(np.maximum(lam[..., 0], lam[..., 1]), np.maximum(lam[..., 2], lam[..., 3]))
    al = np.abs(lam)
    scale = np.maximum(np.maximum(al[..., 0], al[..., 1]), np.maximum(al[..., 2], al[..., 3]))
    inc = (top[..., None] - lam) <= dt(FIT_GAP) * scale[..., None]            # [L,4]
    q = np.zeros_like(lam)
    for k in range(4):
        w = np.where(inc[..., k], V[..., 0, k], dt(0))
        q = q + w[..., None] * V[..., :, k]
    n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    first = np.zeros_like(lam)            # the top eigenvector as it is: the first column that holds the largest eigenvalue
    taken = np.zeros(lam.shape[:-1], bool)
    for k in range(4):
        pick = (lam[..., k] == top) & ~taken
        first = np.where(pick[..., None], V[..., :, k], first)
        taken |= pick
    half = n2 < dt(HALF_TURN)
    proj2 = n2
    q = np.where(half[..., None], first, q)
    n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    q = q / np.sqrt(n2)[..., None]
    return q, dict(lam=lam, top=top, scale=scale, included=inc, half=half, proj2=proj2)


def rotation(q):
    dt = q.dtype.type
    w, x, y, z = (q[..., k] for k in range(4))
    R = np.zeros(q.shape[:-1] + (3, 3), q.dtype)
    two = dt(2)
    R[..., 0, 0] = dt(1) - two * (y * y + z * z)
    R[..., 0, 1] = two * (x * y - w * z)
    R[..., 0, 2] = two * (x * z + w * y)
    R[..., 1, 0] = two * (x * y + w * z)
    R[..., 1, 1] = dt(1) - two * (x * x + z * z)
    R[..., 1, 2] = two * (y * z - w * x)
    R[..., 2, 0] = two * (x * z - w * y)
    R[..., 2, 1] = two * (y * z + w * x)
    R[..., 2, 2] = dt(1) - two * (x * x + y * y)
    return R


def fit_ref(nodes, moved, table, dtype=np.float64, sweeps: int = SWEEPS, parts: bool = False):
    """The rows ``[R | t]`` of every (step, node) as the kernel forms them, in ``dtype``: ``[M,3,4]`` for ``moved [M,3]``, ``[S,M,3,4]`` for
    ``[S,M,3]``.  ``parts``: also a dict with ``S``, the eigenvalues, the included set and the half-turn flags (for the margins)."""
    dt = np.dtype(dtype).type
    idx, live, fin, a32, b32 = _members(nodes, moved, table)
    single = np.asarray(moved).ndim == 2
    a, b = a32.astype(dtype), np.where(np.isfinite(b32), b32, np.float32(0)).astype(dtype)
    Sn, M = b.shape[0], a.shape[0]
    am = a[idx][None].repeat(Sn, 0)                                         # [S,M,1+kn,3]
    bm = np.stack([b[s][idx] for s in range(Sn)])
    cnt = np.zeros((Sn, M), dtype)
    ca, cb = np.zeros((Sn, M, 3), dtype), np.zeros((Sn, M, 3), dtype)
    for k in range(idx.shape[1]):
        on = live[:, :, k]
        cnt = cnt + np.where(on, dt(1), dt(0))
        ca = ca + np.where(on[..., None], am[:, :, k], dt(0))
        cb = cb + np.where(on[..., None], bm[:, :, k], dt(0))
    cnt = np.maximum(cnt, dt(1))                                            # (a lane whose own position is poisoned: overwritten below)
    ca, cb = ca / cnt[..., None], cb / cnt[..., None]
    S = np.zeros((Sn, M, 3, 3), dtype)
    for k in range(idx.shape[1]):
        on = live[:, :, k]
        da, db = am[:, :, k] - ca, bm[:, :, k] - cb
        S = S + np.where(on[..., None, None], da[..., :, None] * db[..., None, :], dt(0))
    lam, V = jacobi(horn_matrix(S), sweeps)
    q, info = quaternion(lam, V)
    R = rotation(q)
    g, p = a[None].repeat(Sn, 0), b
    t = p - ((R[..., 0] * g[..., None, 0] + R[..., 1] * g[..., None, 1]) + R[..., 2] * g[..., None, 2])
    out = np.concatenate([R, t[..., None]], axis=-1)
    ident = np.concatenate([np.eye(3, dtype=dtype), np.zeros((3, 1), dtype)], axis=1)
    out = np.where(fin[..., None, None], out, ident)
    info.update(S=S, own=fin, q=q)
    out = out[0] if single else out
    return (out, info) if parts else out


def sweeps_needed(N, most: int = SWEEPS) -> int:
    """The smallest number of sweeps after which the largest off-diagonal entry of every matrix of ``N [L,4,4]`` is at the rounding floor,
    ``FLOOR`` times the matrix' largest |eigenvalue| -- and stays there for every later sweep up to ``most``."""
    trace = []
    lam, _ = jacobi(np.asarray(N, np.float64), most, trace)
    scale = np.abs(lam).max(axis=-1)
    worst = [float(np.max(np.where(scale > 0, off / np.where(scale > 0, scale, 1.0), np.where(off > 0, np.inf, 0.0)))) for off in trace]
    need = most + 1
    for n in range(most, 0, -1):
        if worst[n - 1] <= FLOOR:
            need = n
        else:
            break
    return need


DRAWN = 100000
WITNESSES = (48072,)   # the matrices of drawn_matrices() that need the most sweeps (11), as this file run as a script finds and prints them


def drawn_matrices(count: int = DRAWN, seed: int = 5) -> np.ndarray:
    """Horn matrices ``[count,4,4]`` of drawn cross-covariances: a fifth each full rank, of rank two, of rank one, with a repeated singular value
    and scaled by 1e-20 .. 1e20 -- the degenerate ones included."""
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(count, 3, 3))
    U, s, Vt = np.linalg.svd(S)
    kind = np.arange(count) % 5
    s[kind == 1, 2] = 0.0
    s[kind == 2, 1:] = 0.0
    s[kind == 3, 1] = s[kind == 3, 0]
    S = np.einsum("nab,nb,nbc->nac", U, s, Vt)
    S[kind == 4] *= 10.0 ** rng.uniform(-20, 20, (int((kind == 4).sum()), 1, 1))
    return horn_matrix(S)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


LINE_DIR = np.array([0.375, -0.25, 0.75])   # generic (no axis), and every multiple used below is exact in binary32


def _line(count, angle_deg, seed):
    """``count`` nodes on a line along LINE_DIR (exactly collinear in binary32), turned by ``angle_deg`` about a drawn axis that is NOT
    perpendicular to the line (so the turn of the line itself is smaller), and shifted."""
    rng = np.random.default_rng(seed)
    s = np.arange(count) - (count - 1) / 2.0 if count % 2 else np.arange(count) - count / 2.0
    rest = (np.array([0.5, 0.25, -1.0]) + s[:, None] * LINE_DIR).astype(np.float32)
    R = _rot(rng.normal(size=3), np.radians(angle_deg))
    moved = (rest.astype(np.float64) @ R.T + rng.uniform(-0.3, 0.3, 3)).astype(np.float32)
    return rest, moved


def _bend(p, rng=None, noise=0.0):
    """A smooth bend of points ``p [M,3]``: a turn about z that grows with x, a sag in z, a shift; plus drawn noise."""
    p = np.asarray(p, np.float64)
    ang = 0.6 * p[:, 0] + 0.2
    c, s = np.cos(ang), np.sin(ang)
    out = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2] + 0.3 * np.sin(1.5 * p[:, 0]) + 0.1 * p[:, 1] ** 2], axis=1) + (0.05, -0.1, 0.2)
    if noise:
        out = out + rng.normal(0.0, noise, out.shape)
    return out.astype(np.float32)


def _drawn(m, seed):
    rng = np.random.default_rng(seed)
    nodes = rng.uniform(-1.0, 1.0, (m, 3)).astype(np.float32)
    return nodes, _bend(nodes, rng, 0.01)


POISON = {3: (0, np.nan), 77: (1, np.inf), 130: (2, np.nan), 200: (0, np.inf), 255: (1, 1e30)}   # node -> (coordinate, value) of `poisoned`
POISON_NONFINITE = (3, 77, 130, 200)


def _poisoned():
    nodes, moved = _drawn(257, 21)
    moved = moved.copy()
    for i, (c, v) in POISON.items():
        moved[i, c] = v
    moved[130] = np.nan
    return nodes, moved


def _grid9():
    from sim_a_splat_amd import deform
    nodes = deform.grid_nodes(((-0.5, -0.5, 0.0), (0.5, 0.5, 0.0)), 0.5)
    return nodes, _bend(nodes)


def _rigid2049():
    """2 049 drawn nodes on the 2^-12 lattice under ``rigid_motion``: a turn that permutes the axes and a dyadic shift, so every moved
    position is EXACT in binary32 and the one motion is the exact answer of every fit that determines a rotation."""
    nodes = (np.round(_drawn(2049, 23)[0].astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
    T = rigid_motion()
    moved = nodes.astype(np.float64) @ T[:, :3].T + T[:, 3]
    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
    return nodes, moved.astype(np.float32)


def rigid_motion() -> np.ndarray:
    """The one motion ``[3,4]`` of `rigid2049`: x -> y -> z -> x (a turn by 120 degrees about (1,1,1)) and a shift by (0.25, -0.5, 0.125)."""
    return np.array([[0.0, 0.0, 1.0, 0.25], [1.0, 0.0, 0.0, -0.5], [0.0, 1.0, 0.0, 0.125]])


def _steps3():
    nodes = _drawn(257, 21)[0]
    rng = np.random.default_rng(29)
    moved = np.stack([_bend(nodes, rng, 0.01), _bend(nodes * np.float32(0.5), rng, 0.01), nodes.copy()])
    return nodes, moved


def _padded():
    return _drawn(257, 27)


CASES = {   # name -> (nodes [M,3], moved [M,3] or [S,M,3]) float32
    "one": lambda: (np.array([[0.25, -0.5, 0.125]], np.float32), np.array([[1.0, 0.3, -0.7]], np.float32)),
    "two": lambda: _line(2, 75.0, 31),
    "line3": lambda: _line(3, 20.0, 32),
    "line5": lambda: _line(5, 170.0, 33),
    "grid9": _grid9,
    "coincident": lambda: (np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (5, 1)), np.random.default_rng(34).normal(size=(5, 3)).astype(np.float32)),
    "drawn257": lambda: _drawn(257, 21),
    "drawn2049": lambda: _drawn(2049, 22),
    "rigid2049": _rigid2049,
    "padded": _padded,
    "poisoned": _poisoned,
    "steps3": _steps3,
    "halfturn": lambda: (np.array([[0.375, -0.25, 0.75], [-0.375, 0.25, -0.75]], np.float32), np.array([[-0.375, 0.25, -0.75], [0.375, -0.25, 0.75]], np.float32)),
}
KNS = (0, 1, 6, 8)
WELL_CONDITIONED = ("grid9", "drawn257", "drawn2049", "rigid2049", "padded", "steps3")   # at kn = 6 and 8: kappa <= 100 is asserted
LINES = ("two", "line3", "line5")
KAPPA_MAX = 100.0


def table_for(name: str, nodes, kn: int) -> np.ndarray:
    """``[M,kn]`` int32: knn_points' table of the nodes (node_opt_ref.knn_table), padded with -1 where there are fewer than ``kn`` other nodes.
    `padded`: every third entry is replaced by -1 or by M, alternately."""
    M = nodes.shape[0]
    nb = np.full((M, kn), -1, np.int32)
    found = no.knn_table(nodes, kn)
    nb[:, :found.shape[1]] = found
    if name == "padded" and kn:
        flat = nb.reshape(-1)
        flat[1::3] = np.where(np.arange(flat[1::3].size) % 2 == 0, -1, M)
    return nb


def cleaned(nb) -> np.ndarray:
    """``nb`` with its entries outside [0, M) removed from their rows: the live ones moved to the front in order, -1 behind."""
    nb = np.asarray(nb)
    out = np.full_like(nb, -1)
    for i, row in enumerate(nb):
        keep = row[(row >= 0) & (row < nb.shape[0])]
        out[i, :keep.size] = keep
    return out


def without(nb, nodes_out) -> np.ndarray:
    """``nb`` with every entry that names one of ``nodes_out`` replaced by -1."""
    nb = np.asarray(nb).copy()
    nb[np.isin(nb, list(nodes_out))] = -1
    return nb


def kappa(S) -> np.ndarray:
    """``sigma1 / (sigma2 + s sigma3)`` of ``S [...,3,3]``, ``s`` the sign of its determinant: the condition of the polar factor."""
    S = np.asarray(S, np.float64)
    sv = np.linalg.svd(S, compute_uv=False)
    s = np.where(np.linalg.det(S) < 0, -1.0, 1.0)
    with np.errstate(all="ignore"):
        return sv[..., 0] / (sv[..., 1] + s * sv[..., 2])


def margins(info) -> dict:
    """The case's distances to the kernel's two thresholds, from ``fit_ref(..., parts=True)``'s dict: ``included`` the largest (top - eigenvalue) /
    threshold over the included eigenvalues, ``excluded`` the smallest over the others, ``half_lanes`` the number of lanes that took the half-turn fallback."""
    lam, top, scale, inc, own = (np.asarray(info[k]) for k in ("lam", "top", "scale", "included", "own"))
    thr = (FIT_GAP * scale)[..., None]
    on = own[..., None] & (thr > 0)
    with np.errstate(all="ignore"):
        ratio = np.where(on, (top[..., None] - lam) / np.where(thr > 0, thr, 1), np.nan).astype(np.float64)
    return dict(included=float(np.nanmax(np.where(inc, ratio, np.nan), initial=0.0)), excluded=float(np.nanmin(np.where(~inc, ratio, np.nan), initial=np.inf)),
                half_lanes=int((np.asarray(info["half"]) & own).sum()))


@functools.lru_cache(maxsize=None)
def case(name: str, kn: int = 6) -> dict:
    """``nodes``, ``moved``, the table ``nb [M,kn]``, ``ref`` = fit_ref(float64), ``wide`` = fit_ref(longdouble), the ``yardstick`` per entry
    and the margins, asserted."""
    nodes, moved = CASES[name]()
    nb = table_for(name, nodes, kn)
    ref, info = fit_ref(nodes, moved, nb, np.float64, parts=True)
    wide, winfo = fit_ref(nodes, moved, nb, np.longdouble, parts=True)
    with np.errstate(all="ignore"):
        err = np.abs(ref.astype(np.longdouble) - wide).astype(np.float64)
    yard = np.maximum(np.where(np.isfinite(err), err, 0.0), np.spacing(np.maximum(1.0, np.abs(ref))))
    mg = margins(info)
    assert mg["included"] <= 1e-3 and mg["excluded"] >= 1e3, (name, kn, mg)
    assert np.array_equal(info["included"], winfo["included"]) and np.array_equal(info["half"], winfo["half"]), (name, kn)
    # the half-turn fallback: taken only where the projection is an exact zero, missed by 1e3 everywhere else
    q_all = np.asarray(info["proj2"], np.float64)   # the squared norm of e0's projection, per lane
    taken = np.asarray(info["half"]) & info["own"]
    assert (q_all[taken] == 0.0).all() and (q_all[~taken & info["own"]] >= 1e3 * HALF_TURN).all(), (name, kn, q_all.min())
    assert bool(taken.any()) == (name == "halfturn" and kn >= 1), (name, kn)
    kap = None
    if name in WELL_CONDITIONED and kn >= 6:
        kap = float(np.max(kappa(info["S"])))
        assert kap <= KAPPA_MAX, (name, kn, kap)
    return dict(name=name, kn=kn, nodes=nodes, moved=moved, nb=nb, ref=ref, wide=wide, yardstick=yard, margins=mg, kappa=kap, info=info,
                min_projection=float(q_all[info["own"]].min()))


def ratios(c: dict, got) -> np.ndarray:
    """``|got - fit_ref(longdouble)| / yardstick`` per entry: the device is held to 4."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, np.float64).astype(np.longdouble) - c["wide"]).astype(np.float64)
    d = np.where(np.isfinite(c["wide"].astype(np.float64)), d, np.where(np.asarray(got, np.float64) == c["wide"].astype(np.float64), 0.0, np.inf))
    return d / c["yardstick"]


def landing_bound(Rt64, nodes) -> np.ndarray:
    """``[...,3]``: how far ``R32 rest + t32`` (evaluated in float64) may lie from the moved position.  ``t64 = moved - R64 rest`` up to float64
    roundings; rounding t and every R entry to binary32 moves them by half a unit in the last place at most, ``2^-24`` of the magnitude, so the
    sum moves by ``2^-24 (|t| + sum_b |R_ab| |rest_b|)`` at most; 16 float64 roundings of that magnitude cover the evaluation on both sides."""
    Rt = np.abs(np.asarray(Rt64, np.float64))
    g = np.abs(np.asarray(nodes, np.float32).astype(np.float64))
    mag = Rt[..., 3] + np.einsum("...ab,...b->...a", Rt[..., :3], np.broadcast_to(g, Rt.shape[:-2] + (3,)))
    return (2.0 ** -24 + 16.0 * 2.0 ** -53) * mag


def rotation_angle(R) -> np.ndarray:
    """The angle (radians) of rotations ``R [...,3,3]``, by atan2 of the skew part and the trace: accurate at every angle."""
    R = np.asarray(R, np.longdouble)
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    return np.arctan2(np.sqrt((v * v).sum(axis=-1)), R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)


def line_directions(c: dict):
    """``(d [3], e [M,3])`` unit vectors in longdouble of a collinear case: the rest line's direction, and per node the least-squares direction
    of ITS members' moved positions -- the one every optimal rotation of that neighbourhood maps d onto."""
    a, b = c["nodes"].astype(np.longdouble), c["moved"].astype(np.longdouble)
    d = LINE_DIR.astype(np.longdouble) / np.sqrt((LINE_DIR.astype(np.longdouble) ** 2).sum())
    e = np.zeros_like(a)
    for i in range(a.shape[0]):
        row = c["nb"][i]
        mem = np.concatenate([[i], row[(row >= 0) & (row < a.shape[0])]]).astype(int)
        da, db = a[mem] - a[mem].mean(axis=0), b[mem] - b[mem].mean(axis=0)
        v = ((da @ d)[:, None] * db).sum(axis=0)
        e[i] = v / np.sqrt((v * v).sum())
    return d, e


def angle_between(d, e):
    """The angle (radians) between unit vectors ``d [3]`` and ``e [...,3]``, by atan2."""
    cr = np.cross(np.broadcast_to(d, e.shape), e)
    return np.arctan2(np.sqrt((cr * cr).sum(axis=-1)), (d * e).sum(axis=-1))


def is_proper(Rt, tol=1e-14):
    """``(largest |R^T R - I|, smallest det)`` of rows ``[...,3,4]``."""
    R = np.asarray(Rt, np.float64)[..., :3]
    err = np.abs(np.einsum("...ki,...kj->...ij", R, R) - np.eye(3)).max()
    return float(err), float(np.linalg.det(R).min())


# ---- checks the CPU tests run on the restatement and the GPU tests on the device ---------------------------------------------------------------
def check_least_rotation(c: dict, Rt, what: str, say=print):
    """A collinear case: every node's rotation maps the rest line's direction onto ITS neighbourhood's moved direction to 1e-9, and its angle
    is the angle between the two to 1e-9 degrees -- of all the rotations that fit equally well, the least."""
    d, e = line_directions(c)
    R = np.asarray(Rt, np.float64)[:, :, :3].astype(np.longdouble)
    off = float(np.abs(R @ d - e).max())
    least = angle_between(d, e)
    excess = float(np.degrees(np.abs(rotation_angle(R) - least).max()))
    say(f"  {c['name']} kn={c['kn']} {what}: the line turns by up to {float(np.degrees(least).max()):.3f} deg; |R d - e| {off:.2e}; |angle - least| {excess:.2e} deg")
    assert off <= 1e-9 and excess <= 1e-9, (off, excess)
    return off, excess


def check_identity(c: dict, Rt):
    """S = 0 (no neighbours, one node, coincident members): R is the identity and t = moved - rest, exactly."""
    Rt = np.asarray(Rt, np.float64)
    assert (Rt[..., :3] == np.eye(3)).all()
    own = np.isfinite(c["moved"]).all(axis=-1)
    assert np.array_equal(Rt[..., 3][own], (c["moved"].astype(np.float64) - c["nodes"].astype(np.float64))[own])


def check_poisoned(fit, kn: int):
    """``fit(nodes, moved, table) -> [M,3,4]`` float64 on `poisoned`: [I | 0] at the nodes whose moved position is not finite; every other
    node's fit is the fit with those nodes removed from its table, bit for bit.  The node moved to 1e30 is FINITE: by the rule it stays a
    member, and every fit it is part of is still a finite, proper rotation."""
    c = case("poisoned", kn)
    got = np.asarray(fit(c["nodes"], c["moved"], c["nb"]), np.float64)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    for i in POISON_NONFINITE:
        assert np.array_equal(got[i], ident), i
    moved = c["moved"].copy()
    moved[list(POISON_NONFINITE)] = 0.0
    clean = np.asarray(fit(c["nodes"], moved, without(c["nb"], POISON_NONFINITE)), np.float64)
    others = np.setdiff1d(np.arange(c["nodes"].shape[0]), POISON_NONFINITE)
    assert np.array_equal(got[others], clean[others])
    assert kn == 0 or np.isin(c["nb"], list(POISON_NONFINITE)).any(axis=1)[others].any()   # (some fits did lose a member)
    assert np.isfinite(got).all()
    err, det = is_proper(got)
    assert err <= 1e-14 and det > 0, (err, det)


if __name__ == "__main__":
    print("fit_ref in float64 against np.longdouble (%d-bit significand); yardstick floor = 1 ulp of max(1, |entry|); SWEEPS = %d" % (np.finfo(np.longdouble).nmant, SWEEPS))
    print(f"{'case':12s} {'kn':>2s} {'yardstick':>10s} {'kappa':>8s} {'included<=':>10s} {'excluded>=':>10s} {'|proj|^2>=':>10s} half")
    mats = []
    for name in CASES:
        for kn in KNS:
            c = case(name, kn)
            mats.append(horn_matrix(c["info"]["S"]).reshape(-1, 4, 4))
            print(f"{name:12s} {kn:2d} {c['yardstick'].max():10.2e} {(c['kappa'] if c['kappa'] is not None else float('nan')):8.2f} {c['margins']['included']:10.2e} "
                  f"{c['margins']['excluded']:10.2e} {c['min_projection']:10.2e} {c['margins']['half_lanes']}")
    kit = sweeps_needed(np.concatenate(mats))
    D = drawn_matrices()
    each = np.array([sweeps_needed(D[k::50]) for k in range(50)])   # (fifty strided parts: which part holds the slowest matrices)
    drawn = int(each.max())
    slow = [int(i) for k in np.nonzero(each == drawn)[0] for i in range(k, DRAWN, 50) if sweeps_needed(D[i:i + 1]) == drawn]
    print(f"the drawn matrices that need {drawn} sweeps: {slow} (WITNESSES = {WITNESSES})")
    assert tuple(slow) == WITNESSES
    print(f"sweeps to the rounding floor ({FLOOR:.2e} of the largest |eigenvalue|): {kit} over the kit's {sum(m.shape[0] for m in mats)} matrices, {drawn} over "
          f"{DRAWN} drawn ones; SWEEPS = max + 2 = {max(kit, drawn) + 2}")
