"""CPU: the kit of the node optimiser on the device (tests/tools/node_opt_ref.py; DESIGN.md 3, "Deformation": the node optimiser) and the host
code beside it: the reverse table, the gather form of the rigidity term against deform.rigidity(table=) within the derived rounding bound, the
default of deform.rigidity bit for bit, the two neighbour searches on the recovery case's grid, and the kernels' restatement of the twist step
within four yardsticks of deform._twist_step."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import node_opt_ref as no  # noqa: E402

from sim_a_splat_amd import deform  # noqa: E402


def _brute_reverse(nb, m):
    start, edges = [0], []
    for j in range(m):
        for e, target in enumerate(np.asarray(nb).reshape(-1)):
            if target == j:
                edges.append(e)
        start.append(len(edges))
    return start, edges


@pytest.mark.parametrize("name", ["m1", "m2", "grid3x3", "drawn257", "hub300", "holes"])
def test_reverse_table_is_the_brute_force_loop(name):
    if name == "holes":   # entries that name nobody, as knn_points writes them for missing neighbours, and one beyond the table
        nb = np.random.default_rng(5).integers(-1, 40, (40, 3)).astype(np.int32)
        nb[7, 1] = 40
    else:
        nb = no.rigidity_case(name)["nb"]
    m = nb.shape[0]
    start, edges = _brute_reverse(nb, m)
    for fn in (no.reverse_table, deform.reverse_table):
        rs, re = fn(nb)
        assert rs.dtype == np.int32 and re.dtype == np.int32 and rs.shape == (m + 1,) and re.shape == (nb.size,)
        assert rs.tolist() == start and re[:start[-1]].tolist() == edges and (re[start[-1]:] == -1).all()


@pytest.mark.parametrize("name", list(no.RIGIDITY_CASES))
def test_gather_form_is_the_host_rigidity_within_the_rounding_bound(name):
    c = no.rigidity_case(name)
    value, grad = no.rigidity_gather(c["nodes"], c["T"], c["nb"], c["rev"])
    assert abs(value - c["value"]) <= c["value_bound"]
    assert (np.abs(grad - c["grad"]) <= c["grad_bound"]).all()
    if c["nb"].shape[1] == 0:
        assert value == 0.0 and not grad.any() and c["value"] == 0.0 and not c["grad"].any()
    else:   # the bound is a rounding bound: many orders of magnitude under the values it guards
        assert c["value_bound"] < 1e-8 * c["value"] and c["grad_bound"].max() < 1e-8 * np.abs(c["grad"]).max()


def test_one_rigid_motion_of_all_nodes_costs_nothing():
    c = no.rigidity_case("drawn257")
    T = np.repeat(no.rigid_transforms(np.random.default_rng(3), 1), 257, axis=0)
    vb, gb = no.rigidity_bound(c["nodes"], T, c["nb"])
    for value, grad in (deform.rigidity(c["nodes"], T, table=c["nb"]), no.rigidity_gather(c["nodes"], T, c["nb"], c["rev"])):
        assert abs(value) <= vb and (np.abs(grad) <= gb).all()


def _rigidity_before(nodes, transforms, neighbours=6):
    """deform.rigidity as it stood before ``table=``."""
    g = np.asarray(nodes, np.float64).reshape(-1, 3)
    T = np.asarray(transforms, np.float64).reshape(-1, 3, 4)
    M = g.shape[0]
    nb = deform._neighbour_table(g, neighbours)
    d = np.zeros_like(T)
    k = nb.shape[1]
    if k == 0:
        return 0.0, d
    R, t = T[:, :, :3], T[:, :, 3]
    gj = g[nb]
    res = (np.einsum("mab,mkb->mka", R, gj) + t[:, None, :]) - (np.einsum("mkab,mkb->mka", R[nb], gj) + t[nb])
    scale = 1.0 / (M * k)
    value = float((res * res).sum() * scale)
    dres = 2.0 * scale * res
    d[:, :, :3] = np.einsum("mka,mkb->mab", dres, gj)
    d[:, :, 3] = dres.sum(axis=1)
    np.subtract.at(d[:, :, :3], nb.reshape(-1), np.einsum("mka,mkb->mkab", dres, gj).reshape(-1, 3, 3))
    np.subtract.at(d[:, :, 3], nb.reshape(-1), dres.reshape(-1, 3))
    return value, d


@pytest.mark.parametrize("name", ["m1", "m2", "grid3x3", "drawn257"])
def test_rigidity_without_a_table_keeps_its_bits_and_table_replaces_the_search(name):
    c = no.rigidity_case(name)
    v0, d0 = _rigidity_before(c["nodes"], c["T"])
    v1, d1 = deform.rigidity(c["nodes"], c["T"])
    assert v0 == v1 and np.array_equal(d0, d1)
    v2, d2 = deform.rigidity(c["nodes"], c["T"], table=deform._neighbour_table(c["nodes"], 6))
    assert v2 == v1 and np.array_equal(d2, d1)
    with pytest.raises(ValueError, match="table must be"):
        deform.rigidity(c["nodes"], c["T"], table=np.zeros((c["nodes"].shape[0] + 1, 2), np.int32))
    with pytest.raises(ValueError, match="table must be"):
        deform.rigidity(c["nodes"], c["T"], table=np.zeros((c["nodes"].shape[0], 2), np.float32))


def test_an_entry_that_names_nobody_is_no_edge():
    c = no.rigidity_case("drawn257")
    nb = c["nb"].copy()
    nb[5, 2], nb[200, 0] = -1, 257
    value, grad = deform.rigidity(c["nodes"], c["T"], table=nb)
    v, d = no.rigidity_gather(c["nodes"], c["T"], nb)
    vb, gb = no.rigidity_bound(c["nodes"], c["T"], nb)
    assert abs(v - value) <= vb and (np.abs(d - grad) <= gb).all()
    assert value < c["value"]   # (two residuals fewer, the normalisation unchanged)


def test_the_two_searches_agree_on_the_recovery_grid_and_may_differ_off_binary32():
    g = no.grid3x3()
    assert np.array_equal(no.knn_table(g, 6), deform._neighbour_table(g, 6))
    # the demo's grid, spacing 1/7: not representable in binary32; the tables may differ in equal-distance neighbours only
    g7 = deform.grid_nodes(((-0.5, -0.5, 0.0), (0.5, 0.5, 0.0)), 1.0 / 7.0)
    a, b = no.knn_table(g7, 6), deform._neighbour_table(g7, 6)
    d2 = ((g7[:, None, :].astype(np.float64) - g7[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    rows = np.arange(g7.shape[0])[:, None]
    print(f"  1/7 grid: {int((a != b).sum())} of {a.size} entries differ between the float32 and the float64 search")
    assert np.allclose(np.sort(d2[rows, a], axis=1), np.sort(d2[rows, b], axis=1), rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("name", list(no.STEP_CASES))
def test_kernel_restatement_of_the_step_within_four_yardsticks(name):
    c = no.step_case(name)
    it, per = c["it"], c["per"]
    decay = 0.05 ** (it / max(1, per - 1))
    T, m1, m2, T32 = no.twist_step_kernel(c["T"], c["d32"], c["d64"], c["weight"], c["nodes"], c["m1"], c["m2"], (c["step"][0] * decay, c["step"][1] * decay),
                                          1 - 0.9 ** (it + 1), 1 - 0.999 ** (it + 1))
    ratios = no.step_ratios(c, T, m1, m2)
    print(f"  {name}: restatement / yardstick " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 4.0
    assert np.array_equal(T32, T.astype(np.float32))
    y = no.step_yardstick(c)
    assert all(y[k] >= float(np.spacing(np.abs(ref).max())) for k, ref in zip(("T", "m1", "m2"), c["ref"]))
    if name.startswith("zero_node") or name.startswith("wide"):   # the series branch: a zero gradient and zero moments move nothing
        z = c["nodes"].shape[0] // 2
        assert np.allclose(T[z], c["T"][z], rtol=0, atol=1e-15) and not m1[z].any() and not m2[z].any()


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError, match="optimizer must be"):
        deform.fit_node_transforms(None, np.zeros((1, 4, 4, 3)), np.eye(4)[None], np.eye(3)[None], 4, 4, np.zeros((1, 3)), optimizer="gpu")
    with pytest.raises(ValueError, match="not with loss_and_grad"):
        deform.fit_node_transforms(None, np.zeros((1, 4, 4, 3)), np.eye(4)[None], np.eye(3)[None], 4, 4, np.zeros((1, 3)), optimizer="device",
                                   loss_and_grad=lambda *a: (0.0, np.zeros((1, 3, 4))))
    with pytest.raises(ValueError, match="optimizer must be"):
        deform.fit_dynamic_scene(None, [], np.zeros((1, 3)), optimizer="gpu")
