"""CPU: the storage-order restatement (tests/tools/order_ref.py) against itself, and the case table (tests/tools/order_cases.py) against the
properties its comments claim.  tests/test_gpu_zb_order.py holds the library to the restatement, bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import order_cases as oc  # noqa: E402
import order_ref  # noqa: E402


def test_constants_are_the_library_s():
    from sim_a_splat_amd import _capi
    assert (oc.TILE, oc.SCAN_ROUND) == (_capi.SAS_ORDER_TILE, _capi.SAS_ORDER_SCAN_ROUND)
    header = (Path(__file__).resolve().parent.parent / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()
    assert f"#define SAS_ORDER_TILE {oc.TILE} " in header and f"#define SAS_ORDER_SCAN_ROUND {oc.SCAN_ROUND} " in header


def test_hilbert_index_is_a_bijection_with_unit_steps():
    """Over the 8 x 8 x 8 grid (3 bits) the index visits every cell once and consecutive cells are face neighbours; at 10 bits the
    vectorised transform equals the scalar one on drawn cells and at the corners."""
    cells = np.array([(x, y, z) for x in range(8) for y in range(8) for z in range(8)])
    code = np.array([order_ref.hilbert3(*c, bits=3) for c in cells])
    assert sorted(code) == list(range(512))
    walk = cells[np.argsort(code)]
    assert np.all(np.abs(np.diff(walk, axis=0)).sum(axis=1) == 1)
    assert np.array_equal(order_ref.hilbert3_np(cells, bits=3), code.astype(np.uint64))
    q = np.random.default_rng(1).integers(0, 1024, (500, 3))
    q[:4] = [[0, 0, 0], [1023, 1023, 1023], [1023, 0, 0], [0, 0, 1023]]
    assert np.array_equal(order_ref.hilbert3_np(q), np.array([order_ref.hilbert3(*c) for c in q], np.uint64))


@pytest.mark.parametrize("name", [n for n in oc.NAMES if oc.split(n)[1] <= 257])
def test_restatement_equals_the_plain_loop(name):
    means, gid = oc.case(name)
    assert np.array_equal(oc.reference(name), order_ref.storage_order_loop(means, gid))


@pytest.mark.parametrize("kind", list(oc.KINDS))
def test_every_result_is_a_permutation_with_ties_in_ascending_index(kind):
    for name in oc.NAMES:
        if oc.split(name)[0] != kind:
            continue
        means, gid = oc.case(name)
        n = oc.split(name)[1]
        perm = oc.reference(name)
        assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(n))
        key = order_ref.keys(means, gid)[perm]
        assert np.all(key[1:] >= key[:-1])
        tie = key[1:] == key[:-1]
        assert np.all(perm[1:][tie] > perm[:-1][tie])


def test_case_table_has_the_properties_it_claims():
    assert len(set(oc.NAMES)) == len(oc.NAMES) == len(oc.KINDS) * len(oc.SIZES) - 7   # (groups256 starts at 257)
    for name in oc.NAMES:
        kind, n = oc.split(name)
        means, gid = oc.case(name)
        assert means.dtype == np.float32 and means.shape == (n, 3) and (gid is None or (gid.dtype == np.uint8 and gid.shape == (n,)))
        fin = np.isfinite(means)
        assert np.all(np.abs(means[fin]) <= 1e30)
        key = order_ref.keys(means, gid)
        distinct = len(np.unique(key))
        q = order_ref.quantise(means)
        if kind in ("uniform", "groups3") and n >= 255:
            assert distinct > 0.9 * n and (gid is None) == (kind == "uniform")
        if kind == "groups3":
            assert means[:, 0].max() > 1e29 or n < 63
        if kind == "groups256":
            assert np.array_equal(np.unique(gid), np.arange(256))
        if kind == "equal":
            assert distinct == 1 and np.array_equal(oc.reference(name), np.arange(n))
        if kind == "lattice":
            assert len(np.unique(key & np.uint64(0xffffffff))) <= 64 and (n < oc.TILE or distinct <= 192 < n / 10)
        if kind == "axis_constant":
            assert order_ref.bounds(means)[2][1] == 0 and np.all(q[:, 1] == 0)
        if kind == "nonfinite" and n >= 255:
            assert 0.03 < 1.0 - fin.mean() < 0.08 and np.isnan(means).any() and np.isposinf(means).any() and np.isneginf(means).any()
        if kind == "axis_nonfinite":
            assert not fin[:, 2].any() and fin[:, :2].all() and np.all(q[:, 2] == 0)
        if kind == "zeros_denormals" and n >= 63:
            z = means[means == 0]
            tiny = np.abs(means[(means != 0) & fin])
            assert np.signbit(z).any() and (~np.signbit(z)).any() and (tiny < np.finfo(np.float32).tiny).any()
        if kind == "at_maximum" and n >= 2:
            assert np.array_equal(order_ref.bounds(means)[2], np.ones(3, np.float32)) and np.all((q == 1023).any(axis=0))
            assert n < 63 or 0.15 < (q == 1023).mean() < 0.25
