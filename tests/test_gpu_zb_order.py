"""GPU: the storage order computed on the device (sas_storage_order, sas_scene_order; Rasterizer.storage_order / read_order; behind upload,
densify and mcmc_refine; DESIGN.md 3, "Storage order") against tests/tools/order_ref.py, the numpy restatement, on the cases of
tests/tools/order_cases.py.  A permutation has no tolerance: every comparison is equality of int32 arrays.  A context created under
SAS_ORDER=0 computes the order with the library's host function, the device path's reference: both must give the restatement."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd.rasterizer import Rasterizer, SasError

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import densify_cases as dc  # noqa: E402
import fit_cases as fc  # noqa: E402
import mcmc_cases as mc  # noqa: E402
import order_cases as oc  # noqa: E402
import order_ref  # noqa: E402
import scene_cases as sc_kit  # noqa: E402

pytestmark = pytest.mark.gpu

OFF = dict(grow=False, prune_opacity_on=False, prune_scale_on=False)


def _context(host_order):
    """A context of its own; host_order: created under SAS_ORDER=0 (the setting is read when a context is created)."""
    old = os.environ.get("SAS_ORDER")
    if host_order:
        os.environ["SAS_ORDER"] = "0"
    else:
        os.environ.pop("SAS_ORDER", None)
    try:
        return Rasterizer(0)
    finally:
        if old is None:
            os.environ.pop("SAS_ORDER", None)
        else:
            os.environ["SAS_ORDER"] = old


@pytest.fixture(scope="module")
def arms():
    """(device-order context, host-order context)"""
    a, b = _context(False), _context(True)
    yield a, b
    a.close()
    b.close()


def _same(perm, ref):
    return perm.dtype == torch.int32 and torch.equal(perm.cpu(), torch.from_numpy(np.array(ref)))


def _order(r, name):
    means, gid = oc.case(name)
    return r.storage_order(torch.from_numpy(means).to(r.device), None if gid is None else torch.from_numpy(gid).to(r.device))


@pytest.mark.parametrize("kind", list(oc.KINDS))
def test_storage_order_is_the_restatement(arms, kind):
    r = arms[0]
    bad = [name for name in oc.NAMES if oc.split(name)[0] == kind and not _same(_order(r, name), oc.reference(name))]
    assert not bad, bad


def test_streams_repeats_and_scratch_reuse(arms):
    r = arms[0]
    big, small, other = f"groups3_{oc.BIG}", "groups256_257", f"nonfinite_{oc.TILE + 1}"
    # twice in a row; a large n and then small ones on one context (the scratch and the histogram table keep what the large call left)
    for name in (big, big, small, "lattice_63", other, small):
        assert _same(_order(r, name), oc.reference(name)), name
    # the default stream and a side stream
    side = torch.cuda.Stream(device=r.device)
    for name in (other, big):
        means, gid = oc.case(name)
        m, g = torch.from_numpy(means).to(r.device), None if gid is None else torch.from_numpy(gid).to(r.device)
        a = r.storage_order(m, g)
        torch.cuda.synchronize(r.device)
        with torch.cuda.stream(side):
            b = r.storage_order(m, g)
        c = r.storage_order(m, g)   # (on another stream than the call before, with nothing waited for in between)
        side.synchronize()
        assert _same(a, oc.reference(name)) and _same(b, oc.reference(name)) and _same(c, oc.reference(name)), name
    # NumPy inputs are copied; n = 0 is an empty tensor
    means, gid = oc.case(small)
    assert _same(r.storage_order(means, gid), oc.reference(small))
    assert _same(r.storage_order(means.tolist(), gid.tolist()), oc.reference(small))   # (and lists)
    with pytest.raises(ValueError, match="means must be"):
        r.storage_order(means[:, :2])
    empty = r.storage_order(np.zeros((0, 3), np.float32))
    assert empty.dtype == torch.int32 and tuple(empty.shape) == (0,) and empty.device == r.device
    with pytest.raises(ValueError, match="group_id must be"):
        r.storage_order(means, gid[:-1])


UPLOADS = [f"uniform_{n}" for n in (1, 257, oc.TILE + 1, oc.BIG)] + [f"groups3_{n}" for n in (1, 257, oc.TILE + 1, oc.BIG)] + \
          [f"groups256_{oc.BIG}", f"nonfinite_{oc.TILE + 1}", "lattice_257"]


@pytest.mark.parametrize("host_order", (False, True), ids=("device", "host"))
def test_upload_then_read_order(arms, host_order):
    r = arms[1 if host_order else 0]
    fresh = _context(host_order)
    try:
        with pytest.raises(SasError, match="status -3"):   # no scene yet
            fresh.read_order()
    finally:
        fresh.close()
    for k, name in enumerate(UPLOADS):
        means, gid = oc.case(name)
        G = 0 if gid is None else int(gid.max()) + 1
        r.upload(means, **oc.dummy_scene(means, gid, G, cov=k % 2 == 1))   # (quaternions and covariances take turns)
        perm = r.read_order()
        assert tuple(perm.shape) == (means.shape[0],) and _same(perm, oc.reference(name)), name
    dev = {k: (torch.from_numpy(v).to(r.device) if isinstance(v, np.ndarray) else v) for k, v in oc.dummy_scene(means, gid, G).items()}
    r.upload(torch.from_numpy(means).to(r.device), **dev)   # device tensors are staged and ordered alike
    assert _same(r.read_order(), oc.reference(name))


def test_bad_group_id_message_is_the_host_path_s(arms):
    name = f"groups3_{oc.TILE + 1}"
    means, gid = oc.case(name)
    gid = gid.copy()
    n = means.shape[0]
    gid[n // 2], gid[n // 2 + 700], gid[n - 1] = 7, 9, 200   # the first one is reported
    said = []
    for r in arms:
        with pytest.raises(SasError) as e:
            r.upload(means, **oc.dummy_scene(means, gid, 3))
        said.append(str(e.value))
        with pytest.raises(SasError, match="status -3"):   # the failed upload left no scene
            r.read_order()
    assert said[0] == said[1] and f"status -1): group_id[{n // 2}]=7 >= n_groups=3" in said[0], said
    gid[:] = 3   # every id bad: index 0
    with pytest.raises(SasError, match=r"group_id\[0\]=3 >= n_groups=3"):
        arms[0].upload(means, **oc.dummy_scene(means, gid, 3))


def _gradients(n, kk, steps, seed):
    rng = np.random.default_rng(seed)
    shapes = dict(means=(n, 3), opacities=(n,), colors=(n, kk, 3), quats=(n, 4), scales=(n, 3))
    return [{k: (10.0 ** rng.uniform(-4.0, 0.0, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32) for k, s in shapes.items()} for _ in range(steps)]


def _resident_order_is_restated(r, gid):
    means = r.read_scene()["means"].cpu().numpy()
    return _same(r.read_order(), order_ref.storage_order(means, gid))


@pytest.mark.parametrize("host_order", (False, True), ids=("device", "host"))
def test_order_after_density_control(arms, host_order):
    r = arms[1 if host_order else 0]
    # the order renewed alone, after steps that move the means far (test_gpu_w_densify.py: test_order_renewal_alone)
    sc, stats, _ = dc.case("n600_sh3")
    n, kk = sc["means"].shape[0], sc["colors"].shape[1]
    sc_kit.upload(r, sc)
    before = r.read_order().cpu().numpy()
    assert np.array_equal(before, order_ref.storage_order(sc["means"], None))
    for t, g in enumerate(_gradients(n, kk, 2, 43), start=1):
        r.adam_step({k: torch.tensor(v, device=r.device) for k, v in g.items()}, dict(fc.LRS, means=0.05), t)
    assert np.array_equal(r.read_order().cpu().numpy(), before)   # steps do not re-order
    out = r.densify({k: torch.tensor(v, device=r.device) for k, v in stats.items()}, **OFF)
    assert out["n"] == n and _resident_order_is_restated(r, None)
    assert not np.array_equal(r.read_order().cpu().numpy(), before)   # (the means moved far: the new order is another one)
    # a mixed clone / split / prune case with groups
    sc, stats, cfg = dc.case("n600_groups")
    sc_kit.upload(r, sc)
    out = r.densify({k: torch.tensor(v, device=r.device) for k, v in stats.items()}, **cfg)
    parents = out["parents"].cpu().numpy()
    assert out["cloned"] > 0 and out["split"] > 0 and out["pruned"] > 0 and _resident_order_is_restated(r, sc["gid"][parents])
    # relocation and growth
    sc, cfg = mc.case("n600_groups")
    sc_kit.upload(r, sc)
    out = r.mcmc_refine(**cfg)
    parents = out["parents"].cpu().numpy()
    assert out["relocated"] > 0 and out["added"] > 0 and _resident_order_is_restated(r, sc["gid"][parents])


def test_frames_and_hooks_are_the_host_arm_s(arms):
    """The same 2 000-Gaussian three-group scene on both contexts, one 64 x 48 view: the frames are the same bits, and read_projection /
    read_tile_lists -- which map slots to the caller's indices through the host copy of the permutation, made on demand -- agree, also
    after a densify call has replaced the permutation."""
    sc = sc_kit.synthetic(2000, 31, 0.04, n_groups=3)
    V, K, W, H = sc_kit.ring(64, 48, f=50.0, yaw=25.0, elev=0.2)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)

    def look(r):
        frame = sc_kit.to_numpy(r.render(V, K, W, H, fc.BACKGROUND, full_sort=True))
        return frame, r.read_projection(), r.read_tile_lists(tiles)

    for r in arms:
        sc_kit.upload(r, sc)
    for renewed in (False, True):
        if renewed:
            for r in arms:
                r.adam_step(dict(means=torch.tensor(_gradients(2000, 1, 1, 44)[0]["means"], device=r.device)), dict(means=0.05), 1)
                assert r.densify(r.new_density_stats(), **OFF)["n"] == 2000
        (fa, pa, ta), (fb, pb, tb) = look(arms[0]), look(arms[1])
        sc_kit.same(fa, fb, keys=("rgb", "alpha", "depth"))
        assert (pa["radii"] > 0).any() and len(ta["sorted_ids"]) > 2000
        for k in pa:
            assert np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)), (renewed, k)
        assert np.array_equal(ta["tile_offsets"], tb["tile_offsets"]) and np.array_equal(ta["sorted_ids"], tb["sorted_ids"]), renewed
        assert torch.equal(arms[0].read_order(), arms[1].read_order())


# ---- last: the bounds-checked build -------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernels above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    import ctypes
    from sim_a_splat_amd import _capi
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
