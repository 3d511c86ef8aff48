"""CPU: the per-node rigid fit of the node driver (sas_nodes_fit_rigid; DESIGN.md 3, "Deformation") as tests/tools/node_fit_ref.py restates it,
against the host's Kabsch fits and against the rule it states for the cases an SVD leaves open."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import node_fit_ref as nf  # noqa: E402

from sim_a_splat_amd import deform  # noqa: E402


def test_entry_point_is_declared_bound_and_exported():
    from sim_a_splat_amd import _capi, build
    header = (ROOT / "include" / "sim_a_splat_amd.h").read_text()
    assert "sas_nodes_fit_rigid" in _capi.EXPORTS and "int sas_nodes_fit_rigid(sas_ctx *ctx" in header
    import ctypes
    L = ctypes.CDLL(str(build.build()))
    assert hasattr(L, "sas_nodes_fit_rigid")
    internal = (ROOT / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()
    for name, value in (("SAS_NODES_FIT_GAP", nf.FIT_GAP), ("SAS_NODES_FIT_HALF_TURN", nf.HALF_TURN), ("SAS_NODES_FIT_SWEEPS", nf.SWEEPS)):
        assert float(re.search(rf"#define {name} (\S+)", internal).group(1)) == value, name
    assert _capi.SAS_NODES_MAX_K == nf.MAX_K


@pytest.mark.parametrize("name", nf.WELL_CONDITIONED)
@pytest.mark.parametrize("kn", (6, 8))
def test_restatement_is_the_host_kabsch_fit_on_well_conditioned_cases(name, kn):
    """The polar factor moves by at most 2 |dS| / (sigma2 + s sigma3), |dS| a few tens of eps |S|; with kappa <= 100 (asserted by the kit)
    that is a few 1e-13 at most: 1e-12 per entry."""
    c = nf.case(name, kn)
    assert c["kappa"] is not None and c["kappa"] <= nf.KAPPA_MAX
    moved = c["moved"].reshape((-1,) + c["nodes"].shape)
    ref = c["ref"].reshape((-1,) + c["nodes"].shape[:1] + (3, 4))
    worst = 0.0
    for s in range(moved.shape[0]):
        host = deform._fit_positions64(c["nodes"], moved[s], table=c["nb"])
        worst = max(worst, float(np.abs(ref[s] - host).max()))
        assert np.array_equal(deform.transforms_from_positions(c["nodes"], moved[s], table=c["nb"]), host.astype(np.float32))   # (rounded once)
    print(f"  {name} kn={kn}: |fit_ref(float64) - host| <= {worst:.2e} (kappa {c['kappa']:.2f})")
    assert worst <= 1e-12


def _host_excess(c):
    """By how many degrees the host's rotation angle exceeds the least one, per node of a collinear case."""
    d, e = nf.line_directions(c)
    host = deform._fit_positions64(c["nodes"], c["moved"], table=c["nb"])
    return np.degrees((nf.rotation_angle(host[:, :, :3]) - nf.angle_between(d, e)).astype(np.float64)), float(np.abs(host[:, :, :3] @ d.astype(np.float64) - e.astype(np.float64)).max())


@pytest.mark.parametrize("name", nf.LINES)
def test_collinear_neighbourhoods_get_the_least_rotation(name):
    for kn in (1, 6, 8):
        c = nf.case(name, kn)
        nf.check_least_rotation(c, c["ref"], "fit_ref(float64)")
        more, off = _host_excess(c)
        print(f"    the host's fit (recorded, not asserted): |R d - e| {off:.2e}, its angle exceeds the least by {more.min():.2f} .. {more.max():.2f} deg")


def test_identity_without_neighbours_and_on_coincident_members():
    for name in nf.CASES:
        nf.check_identity(nf.case(name, 0), nf.case(name, 0)["ref"])
    for name in ("one", "coincident"):
        for kn in nf.KNS:
            nf.check_identity(nf.case(name, kn), nf.case(name, kn)["ref"])


@pytest.mark.parametrize("kn", nf.KNS)
def test_poisoned_positions(kn):
    nf.check_poisoned(lambda g, b, nb: nf.fit_ref(g, b, nb, np.float64), kn)


def test_every_case_is_a_proper_rotation_and_lands_its_node():
    for name in nf.CASES:
        for kn in nf.KNS:
            c = nf.case(name, kn)
            err, det = nf.is_proper(c["ref"])
            assert err <= 1e-14 and det > 0, (name, kn, err, det)


def test_sweep_count_is_the_floor_plus_two():
    """SAS_NODES_FIT_SWEEPS is the smallest count at which every kit case and 100 000 drawn matrices, the degenerate ones included, are at the
    rounding floor (and stay there), plus two.  The kit run as a script takes all 100 000 through the sweeps and names the slowest
    (WITNESSES); here every 20th of them and those witnesses are, which needs the same count in a twentieth of the time."""
    mats = [nf.horn_matrix(nf.case(name, kn)["info"]["S"]).reshape(-1, 4, 4) for name in nf.CASES for kn in nf.KNS]
    kit = nf.sweeps_needed(np.concatenate(mats))
    D = nf.drawn_matrices()
    drawn = nf.sweeps_needed(np.concatenate([D[::20], D[list(nf.WITNESSES)]]))
    print(f"  sweeps to the floor: {kit} over the kit's matrices, {drawn} over {D.shape[0] // 20} drawn ones and the witnesses; SWEEPS = {nf.SWEEPS}")
    assert max(kit, drawn) + 2 == nf.SWEEPS
    # and at SWEEPS the eigenvectors are orthonormal and reproduce the matrix
    N = nf.drawn_matrices(2000, seed=6)
    lam, V = nf.jacobi(N)
    scale = np.abs(lam).max(axis=1)[:, None, None]
    assert np.abs(np.einsum("nki,nkj->nij", V, V) - np.eye(4)).max() <= 1e-14
    assert (np.abs(np.einsum("nik,nk,njk->nij", V, lam, V) - N) <= 1e-14 * scale).all()


def test_table_takes_the_place_of_the_search_bit_for_bit():
    c = nf.case("grid9", 6)
    own = deform.transforms_from_positions(c["nodes"], c["moved"], neighbours=6)
    assert np.array_equal(own, deform.transforms_from_positions(c["nodes"], c["moved"], table=deform._neighbour_table(c["nodes"], 6)))
    assert np.array_equal(own, deform.transforms_from_positions(c["nodes"], c["moved"], table=c["nb"]))   # (spacing 0.5: knn_points' table is the same)
    assert own.dtype == np.float32 and own.shape == (9, 3, 4)
    with pytest.raises(ValueError, match="table must be"):
        deform.transforms_from_positions(c["nodes"], c["moved"], table=c["nb"][:5])
    none = deform.transforms_from_positions(c["nodes"], c["moved"], table=np.full((9, 2), -1))
    assert (none[:, :, :3] == np.eye(3, dtype=np.float32)).all()
