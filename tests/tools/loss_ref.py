"""The photometric loss of DESIGN.md 3, "Photometric loss", restated in numpy: the yardstick of tests/test_loss_cpu.py and
tests/test_gpu_v_loss.py.

    loss = (1 - lam) l1 + lam (1 - ssim),  l1 = sum w |x - y| / D,  ssim = sum w ssim_p / D,  mse = sum w (x - y)^2 / D,  D = max(3 sum w, 1)

with ssim_p the per pixel and channel SSIM map under the normalised 11x11 Gaussian window (sigma 1.5, zero padding), C1 = 0.01^2,
C2 = 0.03^2.  ``evaluate(..., dtype=np.float64)`` is the definition; ``dtype=np.float32`` is the FLOAT32 RESTATEMENT: every operation in
binary32 and in the kernels' order -- windowed sums separably, rows then columns, ``g[0] v[0]`` then ``+ g[k] v[k]``; the per-pixel
formulas operation by operation; the sums over pixels as the kernels take them (channels in order, a 256-lane tree per 16x16 tile, the
tiles in double).  Its error against the definition is what float32 costs on a case; the GPU bounds are four times it."""
import numpy as np

RADIUS, TILE = 5, 16
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    """The 11 coefficients in float64."""
    k = np.arange(2 * RADIUS + 1, dtype=np.float64)
    g = np.exp(-(k - RADIUS) ** 2 / (2.0 * 1.5 ** 2))
    return g / g.sum()


def blur(a, g):
    """g (x) g * a with zero padding, for a [H,W,...] in a's dtype: rows (along W) first, then columns, each a running sum from k = 0."""
    H, W = a.shape[:2]
    P = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS) + a.shape[2:], a.dtype)
    P[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = a
    rows = g[0] * P[:, 0:W]
    for k in range(1, len(g)):
        rows = rows + g[k] * P[:, k:k + W]
    out = g[0] * rows[0:H]
    for k in range(1, len(g)):
        out = out + g[k] * rows[k:k + H]
    return out


def _tile_sums(v):
    """The float32 kernels' sum of v [H,W] (float32): a fixed tree over the 256 lanes of each 16x16 tile (lanes outside the image hold 0),
    the tiles' sums added in double -- lane t of the tail takes tiles t, t + 256, ..., then the same tree."""
    H, W = v.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    P = np.zeros((ty * TILE, tx * TILE), np.float32)
    P[:H, :W] = v
    lanes = P.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, TILE * TILE).copy()
    s = 128
    while s:
        lanes[:, :s] = lanes[:, :s] + lanes[:, s:2 * s]
        s //= 2
    tail = np.zeros(256, np.float64)
    for b, p in enumerate(lanes[:, 0]):
        tail[b % 256] = tail[b % 256] + np.float64(p)
    s = 128
    while s:
        tail[:s] = tail[:s] + tail[s:2 * s]
        s //= 2
    return tail[0]


def ssim_parts(x, y, g):
    """(ssim_p, d/dmu_x, d/dsigma_x^2, d/dsigma_xy) [H,W,3] in x's dtype; the three partials hold g*x^2 and g*xy fixed (mu_x enters
    sigma_x^2 and sigma_xy), which is what the composition ``g*(d_mu) + 2 x g*(d_vx) + y g*(d_cxy)`` needs."""
    T = x.dtype.type
    mx, my = blur(x, g), blur(y, g)
    sxx, syy, sxy = blur(x * x, g), blur(y * y, g), blur(x * y, g)
    mx2, my2, mxy = mx * mx, my * my, mx * my
    vx, vy, cxy = sxx - mx2, syy - my2, sxy - mxy
    A1, A2, B1, B2 = T(2) * mxy + T(C1), T(2) * cxy + T(C2), (mx2 + my2) + T(C1), (vx + vy) + T(C2)
    den = B1 * B2
    ssim = (A1 * A2) / den
    d_vx = -(ssim / B2)
    d_cxy = (T(2) * A1) / den
    t = my * B1 - A1 * mx
    d_mu = (((T(2) * t) * A2) / (B1 * den) - (T(2) * mx) * d_vx) - my * d_cxy
    return ssim, d_mu, d_vx, d_cxy


def evaluate(x, y, mask=None, lam=0.2, background=None, dtype=np.float64, grad=True):
    """dict(terms=[loss, l1, ssim, mse], g_rgb [H,W,3] and, with ``background`` (the prechained form: autograd.prechain's rule with no
    depth gradient), g_alpha [H,W]) in ``dtype``.  ``mask [H,W]``: non-zero counts.  lam == 0 in float32 does no SSIM work (ssim: NaN)."""
    T = np.dtype(dtype).type
    f32 = np.dtype(dtype) == np.float32
    with np.errstate(all="ignore"):
        x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
        H, W = x.shape[:2]
        w = np.ones((H, W), dtype) if mask is None else (np.asarray(mask) != 0).astype(dtype)
        g = window().astype(dtype)
        lam_, oml = T(lam), T(1) - T(lam)
        d = x - y
        skip = f32 and lam == 0
        if not skip:
            ssim_p, d_mu, d_vx, d_cxy = ssim_parts(x, y, g)
        chan = lambda v: (v[..., 0] + v[..., 1]) + v[..., 2]
        total = (lambda v: _tile_sums(v)) if f32 else (lambda v: v.sum())
        wc = w[..., None]
        D = T(max(T(3) * T(total(w)), T(1)))
        l1 = T(total(chan(wc * np.abs(d)))) / D
        mse = T(total(chan(wc * (d * d)))) / D
        if skip:
            ssim, loss = T(np.nan), l1
        else:
            ssim = T(total(chan(wc * ssim_p))) / D
            loss = oml * l1 + lam_ * (T(1) - ssim)
        res = dict(terms=np.array([loss, l1, ssim, mse], dtype))
        if not grad:
            return res
        gx = ((oml * wc) * np.sign(d)) / D
        if not skip:
            gs = (blur(wc * d_mu, g) + (T(2) * x) * blur(wc * d_vx, g)) + y * blur(wc * d_cxy, g)
            gx = gx - (lam_ * gs) / D
        if background is not None:
            bg = np.asarray(background).astype(dtype)
            gx = np.where(x < 1, gx, T(0))
            res["g_alpha"] = T(0) - ((gx[..., 0] * bg[0] + gx[..., 1] * bg[1]) + gx[..., 2] * bg[2])
        res["g_rgb"] = gx
        return res


def rel_err(a, b):
    """max |a - b| / max |b| (0 / 0 = 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    top, scale = np.abs(a - b).max(), np.abs(b).max()
    return float(top / scale) if scale > 0 else float(top)
