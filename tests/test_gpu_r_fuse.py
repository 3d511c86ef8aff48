"""GPU: depth fusion (sas_fuse_depth / Rasterizer.fuse_depth; DESIGN.md 3, "Depth fusion") against tests/tools/fuse_ref.py, which
tests/test_fuse_cpu.py holds to its float64 form on cases where float32 arithmetic is exact.

Every comparison with ``fuse32``, the contract restated in NumPy float32, is BYTE-EQUAL on ``tsdf``, ``weight`` and ``color``: there is
no tolerance in any of them.  Shapes are the smallest that reach each edge: rows that are no multiple of the wave, a last wave and a
last workgroup that are partial, voxels one float either side of every threshold of the contract.  Every check prints what it
measured.  Every test fails without the feature: the entry point and the methods do not exist.  The file runs unchanged under the
bounds-checked build, and its last test reads that build's counter.
"""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from sim_a_splat_amd import _capi, reconstruct
from sim_a_splat_amd.rasterizer import cloud_keep_table, fuse_transforms

sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
import cloud_cases as cc  # noqa: E402
import fuse_cases as fc  # noqa: E402
import fuse_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("tsdf", "weight", "color")
WG = _capi.SAS_FUSE_THREADS
# per-view rows of one launch (the C ABI does not export it: read where the library defines it)
MAX_ROWS = int(re.search(r"#define SAS_FUSE_MAX_ROWS\s+(\d+)", (Path(__file__).resolve().parent.parent / "sim_a_splat_amd" / "csrc" / "sas_internal.h").read_text()).group(1))


def _equal(what, got, want):
    n = 0
    for name in NAMES:
        if want.get(name) is not None:
            g, w = got[name], want[name]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
            bad = int((g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1)).sum())
            assert bad == 0, (what, name, f"{bad} bytes differ", g.reshape(-1)[:8], w.reshape(-1)[:8])
            n += g.nbytes
    return n


def _device_volume(r, init):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(r.device) for a in init]


def _abi(r, c, init=None, views=None, color=True, rgb8=True, keep=None, near=0.01, max_weight=64.0, trunc=None, pixel_centre=None, trace=None):
    """sas_fuse_depth itself on a case that carries ``transform`` rows (dyadic, edge), and fuse32 on the same arguments:
    (got, want) as host arrays."""
    L = _capi.lib()
    v = slice(None) if views is None else views
    init = fr.empty_volume(c["dims"], color=color) if init is None else init
    vol = _device_volume(r, init)
    depth, T, Ks = c["depth"][v], np.ascontiguousarray(c["transform"][v]), np.ascontiguousarray(c["Ks"][v].reshape(-1, 9))
    C = depth.shape[0]
    c8 = c["rgb8"][v] if rgb8 else None
    lab = c["labels"][v] if keep is not None else None
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(r.device)
    d_, c8_, lab_ = dev(depth), dev(c8), dev(lab)
    ptr = lambda t: None if t is None else t.data_ptr()
    lo, dims = np.asarray(c["lo"], np.float32), np.asarray(c["dims"], np.int32)
    trunc = c["trunc"] if trunc is None else trunc
    pc = c.get("pixel_centre", 0.5) if pixel_centre is None else pixel_centre
    rc = L.sas_fuse_depth(r._ctx, C, c["W"], c["H"], ptr(d_), ptr(c8_), ptr(lab_), Ks.ctypes.data, T.ctypes.data, None if keep is None else keep.ctypes.data,
                          lo.ctypes.data, c["voxel"], dims.ctypes.data, trunc, near, pc, max_weight, 0, ptr(vol[0]), ptr(vol[1]), ptr(vol[2]), None)
    assert rc == 0, L.sas_last_error(r._ctx).decode()
    got = dict(zip(NAMES, (None if t is None else t.cpu().numpy() for t in vol)))
    want = fr.fuse32(*init, depth, Ks, T, lo, c["voxel"], trunc, rgb8=c8 if init[2] is not None else None, labels=lab, keep=keep, near=near,
                     pixel_centre=pc, max_weight=max_weight, trace=trace)
    return got, want


def _camera_trunc(viewmats, frame, trunc):
    """fuse_depth's documented rule: the truncation distance in camera units is trunc times the cube root of |det A| of the first view's
    volume-to-camera map (float64)."""
    A = np.asarray(viewmats, np.float64)[0]
    if frame is not None:
        A = A @ np.linalg.inv(np.asarray(frame, np.float64))
    return trunc * float(np.cbrt(abs(np.linalg.det(A[:3, :3]))))


def _method(r, c, init=None, views=None, color=True, frame=None, keep_labels=None, device_inputs=False, trace=None, **kw):
    """Rasterizer.fuse_depth through a TsdfVolume on a drawn case (view matrices), and fuse32: (got, want)."""
    v = slice(None) if views is None else views
    vol = reconstruct.TsdfVolume(r, c["lo"], c["voxel"], dims=c["dims"], color=color)
    init = fr.empty_volume(c["dims"], color=color) if init is None else init
    for t, a in zip((vol.tsdf, vol.weight, vol.color), init):
        if t is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    depth, V, Ks, c8 = c["depth"][v], c["viewmats"][v], c["Ks"][v], c["rgb8"][v]
    lab = c["labels"][v] if keep_labels is not None else None
    put = (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(r.device)) if device_inputs else (lambda a: a)
    trunc = kw.pop("trunc", c["trunc"])
    vol.integrate(put(depth), V, Ks, c["W"], c["H"], rgb8=put(c8), labels=put(lab), keep_labels=keep_labels, frame=frame, trunc=trunc, **kw)
    got = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=None if vol.color is None else vol.color.cpu().numpy())
    want = fr.fuse32(*init, depth, Ks, fuse_transforms(V, frame), c["lo"], c["voxel"], _camera_trunc(V, frame, trunc), rgb8=c8 if color else None, labels=lab,
                     keep=cloud_keep_table(keep_labels), near=kw.get("near", 0.01), pixel_centre=kw.get("pixel_centre", 0.5),
                     max_weight=kw.get("max_weight", 64.0), trace=trace)
    return got, want, vol


# ---- 1: shapes at the kernel's edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 70])
def test_row_lengths(rasterizer, nx):
    for (ny, nz), (H, W), C in (((3, 5), (12, 16), 1), ((5, 3), (32, 33), 2), ((3, 3), (12, 16), 7)):
        c = fc.drawn(C, H, W, seed=10 * nx + C, dims=(nx, ny, nz), voxel=0.02)
        got, want, _ = _method(rasterizer, c, keep_labels=[0, 1, 2])
        n = _equal(f"nx={nx}", got, want)
        print(f"  {nx} x {ny} x {nz} voxels, {C} views of {H}x{W}: {int((want['weight'] > 0).sum())} touched, {n} bytes equal")
        assert nx == 1 or (want["weight"] > 0).any()


def test_workgroup_edge(rasterizer):
    """nx ny nz one above a multiple of the workgroup size (and one below, and on it): the last workgroup holds one voxel."""
    for dims in ((WG + 1, 1, 1), (257, 3, 1), (3, 171, 1), (WG, 1, 2), (WG - 1, 1, 1)):      # 257, 771 = 3 * 256 + 3, 513, 512, 255
        c = fc.drawn(2, 12, 16, seed=sum(dims), dims=dims, voxel=1.6 / 300)
        got, want, _ = _method(rasterizer, c)
        n = _equal(f"dims={dims}", got, want)
        last = want["weight"].reshape(-1)[-1]
        print(f"  {dims}: {np.prod(dims)} voxels = {np.prod(dims) // WG} workgroups + {np.prod(dims) % WG}, last voxel's weight {last}, {n} bytes equal")
        assert (want["weight"] > 0).any()
    assert 513 % WG == 1 and 257 % WG == 1


# ---- 2: geometry edges ---------------------------------------------------------------------------------------------------------------
def test_behind_outside_and_nowhere(rasterizer):
    r = rasterizer
    # a volume that straddles the camera plane and the image borders
    c = fc.drawn(3, 12, 16, seed=21, dims=(70, 5, 9), voxel=0.5, centre=(0.0, 0.0, 0.5))
    trace = []
    got, want, _ = _method(r, c, trace=trace)
    n = _equal("straddling", got, want)
    behind = sum(int((~t["front"]).sum()) for t in trace)
    outside = sum(int((t["front"] & ~t["in_image"]).sum()) for t in trace)
    print(f"  straddling volume: {behind} voxel-views behind the camera, {outside} outside the image, {int((want['weight'] > 0).sum())} touched, {n} bytes equal")
    assert behind > 0 and outside > 0 and (want["weight"] > 0).any()
    # a volume outside every frustum: its bytes stay, a NaN the caller left there included
    c = fc.drawn(2, 12, 16, seed=22, dims=(65, 3, 5), voxel=0.05, centre=(0.0, 0.0, -40.0))
    init = list(fr.empty_volume(c["dims"]))
    rng = np.random.default_rng(3)
    init[0] = rng.normal(size=init[0].shape).astype(np.float32)
    init[0].reshape(-1)[::7] = np.nan
    init[1] = rng.integers(0, 5, init[1].shape).astype(np.float32)
    init[2] = rng.uniform(0, 255, init[2].shape).astype(np.float32)
    got, want, _ = _method(r, c, init=tuple(init))
    _equal("outside every frustum", got, want)
    assert all(got[k].tobytes() == a.tobytes() for k, a in zip(NAMES, init))
    print(f"  outside every frustum: {sum(a.nbytes for a in init)} bytes unchanged, {int(np.isnan(got['tsdf']).sum())} NaNs kept")


def _edge(r, what, variants, expect, **fixed):
    """The edge volume under three values of one parameter: bytes equal to fuse32 each time, and the updated voxel counts show that the
    threshold was really crossed."""
    counts = []
    for kw in variants:
        args = dict(fixed, **kw)
        case = fc.edge_volume(**{k: args.pop(k) for k in ("depth", "cx", "cy", "label") if k in args})
        trace = []
        got, want = _abi(r, case, trace=trace, **args)
        _equal(what, got, want)
        counts.append(int(trace[0]["updated"].sum()))
    print(f"  {what}: updated voxels {counts}")
    assert counts == expect, (what, counts)


def test_thresholds_one_float_apart(rasterizer):
    """fuse_cases.edge_volume: 27 voxels in the layers z = 3/4, 1, 5/4, columns x, y = -1/4, 0, 1/4, one identity camera with fx = fy = 8, an
    8 x 8 image of constant depth, trunc 1/2.  Each line moves ONE parameter one float below, onto and one float above a threshold that
    the nine (or three) voxels concerned sit on exactly; the counts of updated voxels are worked out by hand beside each line."""
    r = rasterizer
    # depth 1: sdf = 1/4, 0, -1/4 by layer, every voxel in the image: all 27 update.  near one float above 1 drops the layer z = 1 too
    _edge(r, "q_z around near_z", [dict(near=x) for x in fc.around(1.0)], [18, 18, 9])
    for pc in (0.5, 0.0):                                                                  # uf = ((fx x / z + cx) - pc) + 0.5
        # cx = 2: the column x = -1/4 has uf = -2 + 2 = 0 in the layer z = 1 (in), -2/3 in z = 3/4 (out), 2/5 in z = 5/4 (in): 24; one float less: 21
        _edge(r, f"uf around 0, pixel_centre {pc}", [dict(cx=x, pixel_centre=pc) for x in fc.around(2.0 + (pc - 0.5))], [21, 24, 24])
        _edge(r, f"vf around 0, pixel_centre {pc}", [dict(cy=x, pixel_centre=pc) for x in fc.around(2.0 + (pc - 0.5))], [21, 24, 24])
        # cx = 6: the column x = 1/4 has uf = 8 = W in the layer z = 1 (out), 8 2/3 in z = 3/4 (out), 7 3/5 in z = 5/4 (in): 21; one float less: 24
        _edge(r, f"uf around W, pixel_centre {pc}", [dict(cx=x, pixel_centre=pc) for x in fc.around(6.0 + (pc - 0.5))], [24, 21, 21])
        _edge(r, f"vf around H, pixel_centre {pc}", [dict(cy=x, pixel_centre=pc) for x in fc.around(6.0 + (pc - 0.5))], [24, 21, 21])
    # depth 1/2: sdf = -1/4 (updated), -1/2, -3/4 (skipped) by layer; the layer z = 1 is skipped iff -1/2 < -trunc: trunc one float below 1/2
    _edge(r, "sdf around -trunc", [dict(trunc=x, depth=0.5) for x in fc.around(0.5)], [9, 18, 18])
    # depth 3/2, every pixel carving: sdf = 3/4 (updated), 1/2, 1/4 (skipped); the layer z = 1 is updated iff 1/2 >= trunc
    _edge(r, "sdf around trunc (carving)", [dict(trunc=x, depth=1.5, keep=cloud_keep_table([])) for x in fc.around(0.5)], [18, 18, 9])


@pytest.mark.parametrize("pixel_centre", [0.0, 0.5])
def test_dyadic_cases(rasterizer, pixel_centre):
    for seed in (1, 2, 3):
        c = fc.dyadic(seed, C=3, pixel_centre=pixel_centre)
        keep = cloud_keep_table([0, 2])
        got, want = _abi(rasterizer, c, keep=keep)
        n = _equal(f"dyadic {seed}", got, want)
        one, w1 = _abi(rasterizer, c, views=[0], keep=keep)
        w64 = fr.fuse64(*fr.empty_volume(c["dims"]), c["depth"][:1], c["Ks"][:1], c["transform"][:1], c["lo"], c["voxel"], c["trunc"], rgb8=c["rgb8"][:1],
                        labels=c["labels"][:1], keep=keep, pixel_centre=pixel_centre)
        _equal(f"dyadic {seed}, one view", one, w1)
        assert np.array_equal(one["tsdf"].astype(np.float64), w64["tsdf"]) and np.array_equal(one["color"].astype(np.float64), w64["color"])
        print(f"  dyadic seed {seed}, pixel_centre {pixel_centre}: {int((want['weight'] > 0).sum())} voxels touched, {n} bytes equal; one view equals float64")
        assert (want["weight"] > 0).sum() > 30


# ---- 3: inputs -----------------------------------------------------------------------------------------------------------------------
def test_inputs(rasterizer):
    r = rasterizer
    c = fc.drawn(2, 12, 15, seed=30, dims=(33, 9, 7), holes=0.1)
    bad, where = fc.with_undefined(c["depth"], 71)
    got, want, _ = _method(r, dict(c, depth=bad))
    _equal("undefined depths", got, want)
    assert np.isfinite(got["tsdf"]).all()
    print(f"  {len(where)} NaN / Inf / 0 / negative depths: {int((want['weight'] > 0).sum())} voxels touched, all finite")
    # rgb8 with and without a colour volume
    for color in (True, False):
        got, want, _ = _method(r, c, color=color)
        _equal(f"color={color}", got, want)
        assert (got["color"] is not None) == color and (not color or (got["color"] > 0).any())
    # labels with keep: surface and carving pixels in one view
    trace = []
    got, want, _ = _method(r, c, keep_labels=[1, 3], trace=trace)
    _equal("keep [1, 3]", got, want)
    surf = sum(int((t["updated"] & t["surface"]).sum()) for t in trace)
    carve = sum(int((t["updated"] & ~t["surface"]).sum()) for t in trace)
    print(f"  keep [1, 3]: {surf} surface updates, {carve} carving updates")
    assert surf > 0 and carve > 0
    for keep in ([], [255], [0, 1, 2, 3, 255]):
        _equal(f"keep {keep}", *_method(r, c, keep_labels=keep)[:2])
    # max_weight = 2 with five views
    c5 = fc.drawn(5, 12, 16, seed=31, dims=(17, 9, 5), holes=0.0)
    got, want, _ = _method(r, c5, max_weight=2.0)
    _equal("max_weight 2", got, want)
    free = _method(r, c5)[1]
    assert got["weight"].max() == 2.0 and free["weight"].max() > 2.0
    print(f"  max_weight 2, 5 views: weights up to {got['weight'].max()} (uncapped {free['weight'].max()})")
    # a pre-filled volume: incremental use
    first = _method(r, c5, views=[0, 1, 2])[0]
    got, want, _ = _method(r, c5, init=(first["tsdf"], first["weight"], first["color"]), views=[3, 4])
    _equal("pre-filled", got, want)
    whole = _method(r, c5)[0]
    assert all(got[k].tobytes() == whole[k].tobytes() for k in NAMES)
    # an affine frame with scale; near and pixel_centre through the method
    F = cc.similarity(1.7, (1, 1, 0), 25.0, (0.1, 0.0, -0.2))
    cf = fc.drawn(3, 12, 16, seed=32, dims=(20, 11, 9), voxel=0.12, centre=tuple((F @ np.array([0.0, 0.0, 1.2, 1.0]))[:3]))
    trace = []
    got, want, _ = _method(r, cf, frame=F, trunc=0.3, near=0.7, pixel_centre=0.0, trace=trace)
    n = _equal("similarity frame", got, want)
    print(f"  frame with scale 1.7: {int((want['weight'] > 0).sum())} voxels touched, {n} bytes equal")
    assert (want["weight"] > 0).sum() > 50 and any((~t["front"]).any() for t in trace)


# ---- 4: determinism ------------------------------------------------------------------------------------------------------------------
def test_determinism(rasterizer):
    r = rasterizer
    c = fc.drawn(7, 12, 16, seed=40, dims=(65, 5, 3))
    a, want, _ = _method(r, c, keep_labels=[0, 1])
    b = _method(r, c, keep_labels=[0, 1], device_inputs=True)[0]
    _equal("7 views", a, want)
    assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)
    init = None
    for v in range(7):
        o = _method(r, c, init=init, views=[v], keep_labels=[0, 1])[0]
        init = (o["tsdf"], o["weight"], o["color"])
    assert all(a[k].tobytes() == x.tobytes() for k, x in zip(NAMES, init))
    print(f"  7 views at once, again from device inputs, and as 7 single-view calls: {sum(a[k].nbytes for k in NAMES)} bytes equal")


def test_more_views_than_one_launch(rasterizer):
    """SAS_FUSE_MAX_ROWS + 1 views: the call is served by two launches in view order, the second with the last view alone in rows packed
    afresh.  From the reference alone: the last view changes tsdf and colour, so the bytes cannot be equal without the second launch."""
    assert MAX_ROWS == 4096
    C = MAX_ROWS + 1
    c = fc.drawn(C, 4, 6, seed=77, dims=(5, 3, 3), voxel=0.02)
    got, want, _ = _method(rasterizer, c)
    n = _equal(f"{C} views", got, want)
    V = c["viewmats"]
    first = fr.fuse32(*fr.empty_volume(c["dims"]), c["depth"][:MAX_ROWS], c["Ks"][:MAX_ROWS], fuse_transforms(V[:MAX_ROWS]), c["lo"], c["voxel"],
                      _camera_trunc(V, None, c["trunc"]), rgb8=c["rgb8"][:MAX_ROWS])
    differ = {k: int((want[k].view(np.uint8).reshape(-1) != first[k].view(np.uint8).reshape(-1)).sum()) for k in NAMES}
    print(f"  {C} views of 4x6 into 5x3x3 voxels: {int((want['weight'] > 0).sum())} touched, {n} bytes equal; view {C} alone changes {differ} bytes of fuse32")
    assert differ["tsdf"] > 0 and differ["color"] > 0


# ---- 5: errors -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(rasterizer):
    import scene_cases as sc_kit
    r = rasterizer
    L = _capi.lib()
    C, H, W = 2, 6, 8
    c = fc.drawn(C, H, W, seed=50, dims=(9, 5, 3), holes=0.0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(r.device)
    depth, rgb8, labels = dev(c["depth"]), dev(c["rgb8"]), dev(c["labels"])
    init = fr.empty_volume(c["dims"])
    tsdf, weight, color = _device_volume(r, init)
    Ks = np.ascontiguousarray(c["Ks"].reshape(C, 9))
    T = fuse_transforms(c["viewmats"])
    keep = np.ones(256, np.uint8)
    lo = np.asarray(c["lo"], np.float32)
    dims = np.asarray(c["dims"], np.int32)
    ptr = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)

    def call(n_views=C, w=W, h=H, d=depth, c8=rgb8, lab=labels, ks=Ks, tr=T, kp=keep, lo_=lo, voxel=c["voxel"], dm=dims, trunc=0.2, near=0.01,
             pc=0.5, mw=64.0, flags=0, t=tsdf, wt=weight, col=color):
        rc = L.sas_fuse_depth(r._ctx, n_views, w, h, ptr(d), ptr(c8), ptr(lab), ptr(ks), ptr(tr), ptr(kp), ptr(lo_), voxel, ptr(dm), trunc, near, pc, mw,
                              flags, ptr(t), ptr(wt), ptr(col), None)
        return rc, L.sas_last_error(r._ctx).decode()

    def changed(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    nan, inf = float("nan"), float("inf")
    cases = {"negative n_views": dict(n_views=-1), "zero width": dict(w=0), "negative height": dict(h=-3),
             "more than 2^31 - 256 pixels": dict(n_views=2, w=32768, h=32768), "dims 0": dict(dm=changed(dims, 1, 0)),
             "dims 1025": dict(dm=changed(dims, 0, 1025)), "more than 2^27 voxels": dict(dm=np.array([1024, 1024, 129], np.int32)),
             "NaN lo": dict(lo_=changed(lo, 2, nan)), "Inf lo": dict(lo_=changed(lo, 0, inf)), "NaN transform": dict(tr=changed(T, 5, nan)),
             "Inf transform": dict(tr=changed(T, 15, inf)), "NaN K": dict(ks=changed(Ks, 2, nan)), "Inf K": dict(ks=changed(Ks, 14, -inf)),
             "fx 0": dict(ks=changed(Ks, 0, 0.0)), "fy negative": dict(ks=changed(Ks, 13, -1.0)), "voxel 0": dict(voxel=0.0), "NaN voxel": dict(voxel=nan),
             "infinite voxel": dict(voxel=inf), "trunc 0": dict(trunc=0.0), "negative trunc": dict(trunc=-0.1), "NaN trunc": dict(trunc=nan),
             "infinite trunc": dict(trunc=inf), "near 0": dict(near=0.0), "NaN near": dict(near=nan), "infinite near": dict(near=inf),
             "max_weight 0.5": dict(mw=0.5), "max_weight 0": dict(mw=0.0), "NaN max_weight": dict(mw=nan), "infinite max_weight": dict(mw=inf),
             "NaN pixel_centre": dict(pc=nan), "infinite pixel_centre": dict(pc=inf), "keep without labels": dict(lab=None),
             "color without rgb8": dict(c8=None), "no depth": dict(d=None), "no Ks": dict(ks=None), "no tsdf": dict(t=None), "no weight": dict(wt=None),
             "unknown flag": dict(flags=2), "async flag": dict(flags=_capi.SAS_ASYNC | _capi.SAS_TIMING)}
    for what, kw in cases.items():
        rc, msg = call(**kw)
        print(f"  {what}: status {rc}, {msg!r}")
        assert rc == -1 and msg, what
    # none of them touched the volume; no view is SAS_OK and changes nothing; then the call itself, with timing
    assert call(n_views=0, d=None, ks=None, tr=None)[0] == 0
    assert all(t.cpu().numpy().tobytes() == a.tobytes() for t, a in zip((tsdf, weight, color), init))
    assert call(flags=_capi.SAS_TIMING)[0] == 0
    ms = r.stage_times()
    print(f"  SAS_TIMING: {ms}")
    assert ms["blend"] > 0 and ms["total"] == ms["blend"] and ms["project"] == 0
    want = fr.fuse32(*init, c["depth"], Ks, T, lo, c["voxel"], 0.2, rgb8=c["rgb8"], labels=c["labels"], keep=keep)
    _equal("after the errors", dict(tsdf=tsdf.cpu().numpy(), weight=weight.cpu().numpy(), color=color.cpu().numpy()), want)
    # allowed: every optional array left out
    assert call(c8=None, lab=None, kp=None, tr=None, col=None)[0] == 0
    # the Python method's own checks
    vol = reconstruct.TsdfVolume(r, c["lo"], c["voxel"], dims=c["dims"])
    with pytest.raises(ValueError):
        vol.integrate(c["depth"][:1], c["viewmats"], c["Ks"], W, H, rgb8=c["rgb8"])
    with pytest.raises(ValueError):
        vol.integrate(c["depth"], c["viewmats"], c["Ks"], W, H, rgb8=c["rgb8"], keep_labels=[1])
    with pytest.raises(ValueError):
        vol.integrate(c["depth"], c["viewmats"], c["Ks"], W, H)                        # a colour volume needs rgb8
    with pytest.raises(_capi.SasError):
        vol.integrate(c["depth"], c["viewmats"], c["Ks"], W, H, rgb8=c["rgb8"], near=0.0)
    with pytest.raises(ValueError):
        reconstruct.TsdfVolume(r, c["lo"], c["voxel"])
    vol.integrate(c["depth"], c["viewmats"], c["Ks"], W, H, rgb8=c["rgb8"])
    assert (vol.weight > 0).any()
    vol.reset()
    assert (vol.tsdf == 1).all() and (vol.weight == 0).all() and (vol.color == 0).all()
    # the context still renders
    sc_kit.upload(r, sc_kit.synthetic(500, 5, 0.05))
    o = r.render(np.eye(4, dtype=np.float32), cc.intrinsics(32, 24, 30.0), 32, 24, want=("alpha",))
    assert o["alpha"].numel() == 24 * 32 and torch.isfinite(o["alpha"]).all()


# ---- 6: through the front ends ---------------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = np.array([-0.16, -0.12, -0.1]), np.array([0.16, 0.12, 0.14])
ICP = cc.similarity(0.8, (0, 0, 1), 30.0, (0.1, -0.2, 0.05))
VOXEL, BOUNDS = 0.025, ([-0.3, -0.3, -0.3], [0.3, 0.3, 0.3])
ORBIT = dict(n_azimuth=6, elevations=(-35, 35), radius=0.9, render_size=(60, 80))


@pytest.fixture(scope="module")
def handler():
    """A few Gaussians on a shell far behind a 12-triangle box from wherever the orbit looks, two of them robot links."""
    from sim_a_splat_amd.handler import SplatHandler
    rng = np.random.default_rng(60)
    d = rng.normal(size=(8, 3))
    means = (3.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    covs = np.broadcast_to((0.05 ** 2 * np.eye(3)).astype(np.float32), (8, 3, 3)).copy()
    masks = {"link0": np.arange(8) < 3, "link1": (np.arange(8) >= 3) & (np.arange(8) < 5)}
    h = SplatHandler.from_arrays(means, covs, rng.uniform(0.2, 0.9, (8, 3)).astype(np.float32), np.full(8, 0.9, np.float32), masks, ICP, [np.eye(4)] * 2, device=0)
    v, f = fc.box_mesh(BOX_LO, BOX_HI)
    h.scene.add_mesh_simple("box", v, f, (0.2, 0.7, 0.3))
    yield h
    h.scene.close()


def test_box_through_the_front_ends(handler):
    scene = handler.scene
    H, W = ORBIT["render_size"]
    cams = reconstruct.orbit_cameras(np.zeros(3), ORBIT["radius"], ORBIT["n_azimuth"], ORBIT["elevations"])
    vol = reconstruct.TsdfVolume(scene._raster, BOUNDS[0], VOXEL, hi=BOUNDS[1])
    assert vol.dims == (24, 24, 24)
    o = scene.fuse_views(vol, H, W, cams, keep=["box"])
    fr_ = {k: v.cpu().numpy() for k, v in o.items()}
    row = scene.row_names().index("box")
    q, p = np.array([c[0] for c in cams], float), np.array([c[1] for c in cams], float)
    V, Ks = scene._views_and_Ks(H, W, q, p, scene.camera.fov)
    trunc = 4 * VOXEL
    want = fr.fuse32(*fr.empty_volume(vol.dims), fr_["depth"], Ks, fuse_transforms(V), vol.lo, VOXEL, _camera_trunc(V, None, trunc), rgb8=fr_["rgb8"],
                     labels=fr_["labels"], keep=cloud_keep_table([row]))
    got = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=vol.color.cpu().numpy())
    n = _equal("box volume", got, want)
    seen = sorted(set(np.unique(fr_["labels"]).tolist()))
    v, f, col = vol.extract_mesh()
    dist = fc.box_distance(v, BOX_LO, BOX_HI)
    print(f"  box: {len(cams)} views of {H}x{W}, labels seen {seen} (box is row {row}), {n} volume bytes equal to fuse32; {len(v)} vertices, {len(f)} faces, "
          f"worst distance to the box {dist.max() / VOXEL:.2f} voxel (bound {(trunc + np.sqrt(3) * VOXEL) / VOXEL:.2f})")
    assert row in seen and len(v) > 100 and len(f) > 100 and np.isfinite(fr_["depth"]).all() and (fr_["depth"] > 0).all()
    assert dist.max() <= trunc + np.sqrt(3.0) * VOXEL
    for k in range(3):
        for plane in (BOX_LO[k], BOX_HI[k]):
            near = np.abs(v[:, k] - plane) <= VOXEL
            assert near.any(), (k, plane)
    assert col.shape == (len(v), 3) and col.dtype == np.uint8 and (col[:, 1].astype(int) > col[:, 0]).mean() > 0.9       # the box is green
    # the handler's chain returns the same mesh
    m = handler.reconstruct_mesh(["box"], BOUNDS, VOXEL, frame="scene", **ORBIT)
    assert m["vertices"].tobytes() == v.tobytes() and m["faces"].tobytes() == f.tobytes() and m["colors"].tobytes() == col.tobytes()
    # ... and in the robot's frame the box's image: bounds, voxel size and vertices are metres there
    F = handler.robot_frame()
    s = float(np.cbrt(abs(np.linalg.det(F[:3, :3]))))
    centre = F[:3, :3] @ (0.5 * (BOX_LO + BOX_HI)) + F[:3, 3]
    mr = handler.reconstruct_mesh(["box"], (centre - 0.3 * s, centre + 0.3 * s), VOXEL * s, frame="robot", n_azimuth=6, elevations=(-35, 35),
                                  radius=0.9 * s, render_size=(60, 80))
    Fi = np.linalg.inv(F)
    back = mr["vertices"] @ Fi[:3, :3].T + Fi[:3, 3]
    dr = fc.box_distance(back, BOX_LO, BOX_HI)
    print(f"  robot frame (scale {s:.3f}): {len(mr['vertices'])} vertices, worst distance to the box {dr.max() / VOXEL:.2f} scene voxel")
    assert len(mr["vertices"]) > 100 and dr.max() <= trunc + np.sqrt(3.0) * VOXEL


# ---- last: the bounds-checked build ------------------------------------------------------------------------------------------------------
def test_no_bounds_reports(rasterizer):
    """Under SAS_LIB_PATH=variants/lib_bounds.so every computed index of the kernel above was range-checked: none was out of range.
    (The product library has no counter, and nothing to read.)"""
    L = _capi.lib()
    if hasattr(L, "sas_debug_bounds"):
        L.sas_debug_bounds.argtypes = [ctypes.c_void_p, ctypes.c_int]
        out = (ctypes.c_ulonglong * 4)()
        assert L.sas_debug_bounds(out, 0) == 0
        print(f"  bounds-checked build: {out[0]} reports (first: code {out[1]}, index {out[2]}, limit {out[3]})")
        assert out[0] == 0
