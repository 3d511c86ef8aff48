"""The cases of the storage-order tests (tests/test_order_cpu.py, tests/test_gpu_zb_order.py): means and group ids drawn with fixed seeds,
and their order by tests/tools/order_ref.py.  Every finite coordinate lies within +-1e30, so hi - lo stays finite and the library's host
path is defined on all of them.

Sizes: 1 and 2; 63, 64, 65 (a wave); 255, 256, 257 (a workgroup); TILE - 1, TILE, TILE + 1 (TILE = SAS_ORDER_TILE of csrc/sas_internal.h, the
keys one workgroup of a sort pass ranks: restated here, tests/test_order_cpu.py holds it to the library's Python module); SCAN = 8193: the
sort's histogram table has 256 entries per workgroup and its scan takes SAS_ORDER_SCAN_ROUND = 1024 entries per round, so four workgroups
fill one round exactly and 4 * 2048 + 1 keys make a fifth workgroup, a table of 1280 entries and a second, ragged round; 65 795 = 256 * 257 + 3
as in densify_cases (33 workgroups, nine rounds, a ragged last tile)."""
import numpy as np

import order_ref

TILE = 2048          # SAS_ORDER_TILE
SCAN_ROUND = 1024    # SAS_ORDER_SCAN_ROUND
SCAN = 4 * TILE + 1
BIG = 256 * 257 + 3
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, SCAN, BIG)
assert 256 * ((SCAN + TILE - 1) // TILE) > SCAN_ROUND >= 256 * ((SCAN - 1 + TILE - 1) // TILE)

# distribution -> what its scene is (the properties tests/test_order_cpu.py checks)
KINDS = {
    "uniform": "uniform in the box [-3, 3] x [-2, 2] x [-1, 1], no groups",
    "groups3": "three groups; axes scaled by 1e30, 1e-30 and 1: the widest and the narrowest box the cases hold",
    "groups256": "256 groups, every id present (n >= 257): the group pass's histogram has no empty digit",
    "equal": "all means equal: every key is 0, the order is the identity",
    "lattice": "means on a 4 x 4 x 4 lattice: at most 64 distinct keys, stability decides nearly everything; three groups on top",
    "axis_constant": "the y axis constant: inv = 0 there",
    "nonfinite": "5 % of the coordinates NaN, +Inf or -Inf",
    "axis_nonfinite": "the z axis entirely non-finite: no bounds there, every cell 0",
    "zeros_denormals": "a third of the coordinates +0, -0 or denormal, of either sign, in a box of normal numbers",
    "at_maximum": "integer coordinates in [0, 1023] with 0 and 1023 present (n >= 2): inv = 1 and u == 1023.0f exactly on a fifth of them",
}
NAMES = tuple(f"{kind}_{n}" for kind in KINDS for n in SIZES if not (kind == "groups256" and n < 257))
SPECIALS = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))


def split(name):
    kind, n = name.rsplit("_", 1)
    return kind, int(n)


def case(name):
    """(means float32 [n,3], group ids uint8 [n] or None)."""
    kind, n = split(name)
    rng = np.random.default_rng(9000 + 100 * list(KINDS).index(kind) + SIZES.index(n))
    means = (rng.uniform(-1.0, 1.0, (n, 3)) * np.array([3.0, 2.0, 1.0])).astype(np.float32)
    gid = None
    if kind == "groups3":
        means = (rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1e30, 1e-30, 1.0])).astype(np.float32)
        gid = rng.integers(0, 3, n).astype(np.uint8)
    elif kind == "groups256":
        gid = rng.permutation(np.arange(n) % 256).astype(np.uint8)
    elif kind == "equal":
        means[:] = np.array([0.25, -1.5, 3.0], np.float32)
    elif kind == "lattice":
        means = (rng.integers(0, 4, (n, 3)) * 0.5 - 0.75).astype(np.float32)
        gid = rng.integers(0, 3, n).astype(np.uint8)
    elif kind == "axis_constant":
        means[:, 1] = np.float32(0.7)
    elif kind == "nonfinite":
        bad = rng.random((n, 3)) < 0.05
        means[bad] = rng.choice(SPECIALS, int(bad.sum()))
    elif kind == "axis_nonfinite":
        means[:, 2] = np.resize(np.array(SPECIALS, np.float32), n)
    elif kind == "zeros_denormals":
        tiny = np.array([0.0, -0.0, 1e-40, -1e-40, 3e-45, -3e-45, 1.1e-38, -1.1e-38], np.float32)
        pick = rng.random((n, 3)) < 1.0 / 3.0
        means[pick] = np.resize(tiny, int(pick.sum()))
    elif kind == "at_maximum":
        means = rng.integers(0, 1024, (n, 3)).astype(np.float32)
        means[rng.random((n, 3)) < 0.2] = np.float32(1023.0)
        if n >= 2:
            means[0], means[n - 1] = np.float32(0.0), np.float32(1023.0)
    return np.ascontiguousarray(means), gid


_RUNS = {}


def reference(name):
    """order_ref.storage_order of the case (computed once, never changed)."""
    if name not in _RUNS:
        means, gid = case(name)
        _RUNS[name] = order_ref.storage_order(means, gid)
        _RUNS[name].setflags(write=False)
    return _RUNS[name]


def dummy_scene(means, gid, n_groups, seed=1, cov=False):
    """What ``Rasterizer.upload`` takes beside the means, drawn: keyword arguments for ``upload(means, **kw)``."""
    n = means.shape[0]
    rng = np.random.default_rng(seed)
    kw = dict(opacities=rng.uniform(0.2, 0.9, n).astype(np.float32), colors=rng.uniform(0.0, 1.0, (n, 1, 3)).astype(np.float32), sh_degree=0)
    if cov:
        s = rng.uniform(0.01, 0.05, (n, 3)).astype(np.float32) ** 2
        kw["covariances"] = np.stack([s[:, 0], 0 * s[:, 0], 0 * s[:, 0], s[:, 1], 0 * s[:, 0], s[:, 2]], axis=1).astype(np.float32)
    else:
        kw.update(quats=rng.normal(size=(n, 4)).astype(np.float32), scales=rng.uniform(0.01, 0.05, (n, 3)).astype(np.float32))
    if gid is not None:
        kw.update(group_id=gid, n_groups=n_groups)
    return kw
