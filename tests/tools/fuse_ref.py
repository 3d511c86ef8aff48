"""The depth-fusion contract ("Depth fusion"; sas_fuse_depth) restated in NumPy, op for op.

``fuse32`` computes in float32 -- every NumPy operation below is one rounded IEEE operation on float32 arrays, constants included, in
the contract's order, nothing fused -- vectorised over the voxels and sequential over the views; it is what the GPU tests hold the
kernel to byte for byte.  ``fuse64`` is the same text in float64 (the float32 inputs widened): on the dyadic cases of fuse_cases.py,
where float32 arithmetic is exact up to the first division, the two agree exactly (tests/test_fuse_cpu.py).  Both return the new
volume and leave their inputs unchanged; ``trace`` (a list) receives one dict per view with the intermediate chain.
"""
import numpy as np


def _fuse(dtype, tsdf, weight, color, depth, Ks, transform, lo, voxel, trunc, rgb8=None, labels=None, keep=None, near=0.01, pixel_centre=0.5,
          max_weight=64.0, trace=None):
    f = dtype
    depth = np.asarray(depth, np.float32)
    if depth.ndim == 4:
        depth = depth[..., 0]
    C, H, W = depth.shape
    nz, ny, nx = np.shape(tsdf)
    tsdf = np.array(tsdf, np.float32).astype(f).reshape(-1)
    weight = np.array(weight, np.float32).astype(f).reshape(-1)
    if color is not None:
        assert rgb8 is not None, "color needs rgb8"
        color = np.array(color, np.float32).astype(f).reshape(-1, 3)
        rgb = np.asarray(rgb8, np.uint8).reshape(-1, 3)
    if keep is not None:
        assert labels is not None, "keep needs labels"
        keep = np.asarray(keep, np.uint8).reshape(256)
        lab = np.asarray(labels, np.uint8).reshape(-1)
    Ks = np.asarray(Ks, np.float32).reshape(C, 9).astype(f)
    T = (np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (C, 1)) if transform is None else np.asarray(transform, np.float32)).reshape(C, 12).astype(f)
    lo = np.asarray(lo, np.float32).reshape(3).astype(f)
    voxel, trunc, near, pc, mw = (f(np.float32(v)) for v in (voxel, trunc, near, pixel_centre, max_weight))
    half, one, zero = f(0.5), f(1.0), f(0.0)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cx_ = lo[0] + (i.reshape(-1).astype(f) + half) * voxel
    cy_ = lo[1] + (j.reshape(-1).astype(f) + half) * voxel
    cz_ = lo[2] + (k.reshape(-1).astype(f) + half) * voxel
    for c in range(C):
        A = T[c]
        fx, cx, fy, cy = Ks[c, 0], Ks[c, 2], Ks[c, 4], Ks[c, 5]
        with np.errstate(all="ignore"):
            q = [((A[4 * m] * cx_ + A[4 * m + 1] * cy_) + A[4 * m + 2] * cz_) + A[4 * m + 3] for m in range(3)]
            front = q[2] >= near
            uf = ((fx * (q[0] / q[2])) + cx) - pc
            uf = uf + half
            vf = ((fy * (q[1] / q[2])) + cy) - pc
            vf = vf + half
            in_image = front & (uf >= zero) & (uf < f(W)) & (vf >= zero) & (vf < f(H))      # (a NaN fails every comparison)
            ok = in_image.copy()
            u = np.where(ok, np.floor(uf), zero).astype(np.int64)
            v = np.where(ok, np.floor(vf), zero).astype(np.int64)
            p = (c * H + v) * W + u
            d = depth.reshape(-1)[p].astype(f)
            ok &= (d > zero) & (d < f(np.inf))
            sdf = d - q[2]
            surface = np.ones(len(p), bool) if keep is None else keep[lab[p]] != 0
            upd = ok & np.where(surface, ~(sdf < -trunc), sdf >= trunc)
            val = np.where(surface, np.minimum(one, sdf / trunc), one)
            w = weight
            w1 = w + one
            new = ((tsdf * w) + val) / w1
            tsdf = np.where(upd, new, tsdf)
            if color is not None:
                newc = ((color * w[:, None]) + rgb[p].astype(f)) / w1[:, None]
                color = np.where((upd & surface)[:, None], newc, color)
            weight = np.where(upd, np.minimum(w1, mw), w)
        if trace is not None:
            trace.append(dict(q=np.stack(q, 1), uf=uf, vf=vf, front=front, in_image=in_image, p=np.where(in_image, p, -1), valid=ok, sdf=sdf,
                              surface=surface, updated=upd, val=val))
    out = dict(tsdf=tsdf.reshape(nz, ny, nx), weight=weight.reshape(nz, ny, nx))
    if color is not None:
        out["color"] = color.reshape(nz, ny, nx, 3)
    return out


def fuse32(tsdf, weight, color, depth, Ks, transform, lo, voxel, trunc, **kw):
    return _fuse(np.float32, tsdf, weight, color, depth, Ks, transform, lo, voxel, trunc, **kw)


def fuse64(tsdf, weight, color, depth, Ks, transform, lo, voxel, trunc, **kw):
    return _fuse(np.float64, tsdf, weight, color, depth, Ks, transform, lo, voxel, trunc, **kw)


def empty_volume(dims, color=True):
    """(tsdf ones, weight zeros, color zeros or None) of ``dims = (nx, ny, nz)``, float32, laid out [nz,ny,nx(,3)]."""
    nx, ny, nz = (int(d) for d in dims)
    return (np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 3), np.float32) if color else None)
