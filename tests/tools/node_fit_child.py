"""The device-side checks of tests/test_gpu_zh_node_fit.py on sas_nodes_fit_rigid, as functions the tests call one by one -- and, run as a
script, all of them in one fresh process: the way the test runs them once more under the bounds-checked build.

    SAS_LIB_PATH=variants/lib_bounds.so python tests/tools/node_fit_child.py

Prints ``node fit child ok`` behind the bounds counter's report (the product library has no counter: the checks alone)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import node_fit_ref as nf  # noqa: E402


def _dev(r, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(r.device)


def fit(r, nodes, moved, nb):
    """``(Rt64, Rt32)`` numpy of one node_fit_rigid call; the outputs are poisoned first, so that every entry must have been written."""
    shape = tuple(np.asarray(moved).shape) + (4,)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=r.device)
    out64 = torch.full(shape, float("nan"), dtype=torch.float64, device=r.device)
    res = r.node_fit_rigid(_dev(r, nodes), _dev(r, moved), _dev(r, nb, np.int32) if nb.shape[1] else None, out=out, out64=out64)
    assert res["transforms"] is out and res["transforms64"] is out64
    return out64.cpu().numpy(), out.cpu().numpy()


def check_case(r, name: str, kn: int, say=print) -> dict:
    """Every property the kernel owes on one case; returns the measured figures."""
    c = nf.case(name, kn)
    T64, T32 = fit(r, c["nodes"], c["moved"], c["nb"])
    # the yardstick: four times the float64 restatement's own error against np.longdouble
    ratio = nf.ratios(c, T64)
    differ = int((T64.view(np.uint64) != c["ref"].view(np.uint64)).sum())
    say(f"  {name} kn={kn}: largest |device - longdouble| / yardstick {ratio.max():.3f} (yardstick {c['yardstick'].max():.2e}); "
        f"{differ} of {T64.size} entries differ in bits from fit_ref(float64)")
    assert ratio.max() <= 4.0, (name, kn, float(ratio.max()))
    # rounded once
    assert np.array_equal(T32.view(np.uint32), T64.astype(np.float32).view(np.uint32))
    # a proper rotation everywhere
    err, det = nf.is_proper(T64)
    assert err <= 1e-14 and det > 0, (name, kn, err, det)
    # the node lands on its moved position, in the float32 rows deform takes
    own = np.isfinite(c["moved"]).all(axis=-1)
    g = np.broadcast_to(c["nodes"].astype(np.float64), c["moved"].shape)
    R32, t32 = T32[..., :3].astype(np.float64), T32[..., 3].astype(np.float64)
    landed = np.einsum("...ab,...b->...a", R32, g) + t32
    off = np.abs(landed - c["moved"].astype(np.float64))[own]
    bound = nf.landing_bound(T64, c["nodes"])[own]
    assert (off <= bound).all(), (name, kn, float((off / bound).max()))
    # no atomics: the same bits again
    again = fit(r, c["nodes"], c["moved"], c["nb"])
    assert np.array_equal(again[0].view(np.uint64), T64.view(np.uint64)) and np.array_equal(again[1].view(np.uint32), T32.view(np.uint32))
    # what the case is there for
    if kn == 0 or name in ("one", "coincident"):
        nf.check_identity(c, T64)
    if name in nf.LINES and kn >= 1:
        nf.check_least_rotation(c, T64, "device", say)
    if name == "rigid2049" and kn >= 6:   # (fewer than three members not on a line do not determine the motion)
        over = np.abs(T64 - nf.rigid_motion()) / c["yardstick"]   # the moved positions are exact in binary32: the motion is the exact answer
        say(f"    one rigid motion: every node's [R | t] within {over.max():.3f} yardsticks of the motion ({np.abs(T64 - nf.rigid_motion()).max():.2e})")
        assert over.max() <= 4.0
    if name == "padded":
        clean = fit(r, c["nodes"], c["moved"], nf.cleaned(c["nb"]))
        assert np.array_equal(clean[0].view(np.uint64), T64.view(np.uint64))
        assert kn == 0 or not np.array_equal(nf.cleaned(c["nb"]), c["nb"])
    if name == "steps3":
        for s in range(3):
            one = fit(r, c["nodes"], c["moved"][s], c["nb"])
            assert np.array_equal(one[0].view(np.uint64), T64[s].view(np.uint64)) and np.array_equal(one[1].view(np.uint32), T32[s].view(np.uint32)), s
    if name == "poisoned":
        nf.check_poisoned(lambda g, b, nb: fit(r, g, b, nb)[0], kn)
    if name == "halfturn" and kn >= 1:
        assert np.abs(np.trace(T64[:, :, :3], axis1=1, axis2=2) + 1.0).max() <= 1e-14   # a half turn: trace -1
    return dict(ratio=float(ratio.max()), differ=differ, entries=int(T64.size), yardstick=float(c["yardstick"].max()))


def bounds_report(say=print):
    """The bounds counter, if the library loaded has one: (reports, code, index, limit), or None."""
    from sim_a_splat_amd import _capi
    L = _capi.lib()
    if not hasattr(L, "sas_debug_bounds"):
        return None
    L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_ulonglong * 4)()
    assert L.sas_debug_bounds(out, 0) == 0
    say(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
    return tuple(int(v) for v in out)


def main():
    from sim_a_splat_amd.rasterizer import Rasterizer
    r = Rasterizer(0)
    for name in nf.CASES:
        for kn in nf.KNS:
            check_case(r, name, kn)
    rep = bounds_report()
    assert rep is None or rep[0] == 0, rep
    r.close()
    print("node fit child ok" + (" (bounds-checked)" if rep is not None else ""))


if __name__ == "__main__":
    main()
