"""float64 numpy restatement of urt_denoise (include/urt.h "denoising"): the edge-avoiding a-trous wavelet filter, literally as the header
states it.  Test helper only (not a conftest): tests/test_denoise_abi.py checks it on its own, tests/test_gpu_denoise.py and
tests/test_gpu_denoise_range.py check the library against it."""
import numpy as np

H = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
MAX_COLOR = np.float32(2.0 ** 120)      # rule 1: a larger demodulated colour passes through
DOMAIN = 2.0 ** 60                      # the accuracy bound is promised for |c / d|, the positive sigmas and z within 2^-60 .. 2^60


def demodulator(albedo, shape=None):
    """d_p (rule 2) as float32: fmaxf(albedo.rgb, 1e-3f) per channel (a NaN channel gives 1e-3), or ones of `shape` without an albedo."""
    if albedo is None:
        return np.ones(tuple(shape[:2]) + (3,), np.float32)
    return np.fmax(np.asarray(albedo, np.float32)[..., :3], np.float32(1e-3))


def surface_mask(color, hit, normal, albedo=None):
    """(h, w) bool: the surface pixels; every other pixel passes through (rule 1).  With `albedo`, the clause on the demodulated colour
    is taken on the float32 quotient c / d, as the library takes it."""
    c, n = np.asarray(color, np.float32), np.asarray(normal, np.float32)
    z = np.asarray(hit, np.float32)[..., 3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = c[..., :3] / demodulator(albedo, c.shape)                     # float32 / float32, correctly rounded
        return ((n[..., 3] != 0) & np.isfinite(z) & (z > 0) & np.isfinite(c[..., :3]).all(-1) & np.isfinite(n[..., :3]).all(-1) &
                (np.abs(q) <= MAX_COLOR).all(-1))                           # false for a NaN or inf quotient


def shifted(a, oy, ox, fill):
    """out[y, x] = a[y + oy, x + ox] where that is inside the image, else `fill`."""
    h, w = a.shape[:2]
    out = np.full(a.shape, fill, dtype=a.dtype)
    ys, yd = (slice(oy, h), slice(0, h - oy)) if oy >= 0 else (slice(0, h + oy), slice(-oy, h))
    xs, xd = (slice(ox, w), slice(0, w - ox)) if ox >= 0 else (slice(0, w + ox), slice(-ox, w))
    if yd.start < yd.stop and xd.start < xd.stop:
        out[yd, xd] = a[ys, xs]
    return out


def reach(iterations):
    """Chebyshev radius of the pixels that can contribute to one output pixel: pass i taps up to 2 * 2^i away."""
    return 2 * (2 ** iterations - 1)


def window_min_max(values, surf, radius):
    """(lo, hi), each shaped like `values` ((h, w) or (h, w, k)): per pixel and channel the smallest and largest of `values` over the
    surface pixels q with |q - p| <= radius in both axes (+inf / -inf where there is none)."""
    v = np.asarray(values, np.float64)
    m = surf if v.ndim == 2 else surf[..., None]
    lo, hi = np.where(m, v, np.inf), np.where(m, v, -np.inf)
    for axis in (0, 1):                                                  # a box is separable
        src_lo, src_hi = lo.copy(), hi.copy()
        for o in range(1, min(radius, v.shape[axis] - 1) + 1):
            for oy, ox in (((o, 0), (-o, 0)) if axis == 0 else ((0, o), (0, -o))):
                lo = np.minimum(lo, shifted(src_lo, oy, ox, np.inf))
                hi = np.maximum(hi, shifted(src_hi, oy, ox, -np.inf))
    return lo, hi


def denoise_ref(color, hit, normal, albedo=None, iterations=5, sigma_color=8.0, sigma_normal=0.5, sigma_depth=0.1):
    """(h, w, 4) float64: rgb = the filtered colour of each surface pixel, alpha = src alpha; pass-through pixels hold src (as float64;
    the library must give the src texel's bits there).  Inputs are (h, w, 4) float32 images in the urt_render_aov layouts.

    Rule 1 as include/urt.h states it: a pixel passes through when its kind is 0, its depth is not finite or <= 0, a component of its
    colour or normal is not finite, or a component of the float32 quotient c_p / d_p is not finite or exceeds 2^120 in magnitude.
    Domain: the library promises |result - this| <= 1e-4 (1 + |this|) where |c_p / d_p| <= 2^60 and every positive sigma (sigma_color
    2^-i for each pass i that runs) and z_p lie in [2^-60, 2^60].  Outside that, for finite inputs, it promises that every filtered
    value before remodulation is finite and within the hull of the demodulated colours in its reach (which holds for this formula too),
    and that c'_p d_p may overflow at its own pixel only."""
    color = np.asarray(color, np.float32)
    surf = surface_mask(color, hit, normal, albedo)
    s3 = surf[..., None]
    c = np.where(s3, color[..., :3].astype(np.float64), 0.0)
    n = np.where(s3, np.asarray(normal, np.float32)[..., :3].astype(np.float64), 0.0)
    z = np.where(surf, np.asarray(hit, np.float32)[..., 3].astype(np.float64), 1.0)
    d = demodulator(albedo, color.shape).astype(np.float64)
    sc, sn, sz = (float(np.float32(s)) for s in (sigma_color, sigma_normal, sigma_depth))
    cur = c / d
    for i in range(iterations):
        s = 2 ** i
        num = np.zeros_like(cur)
        den = np.zeros(surf.shape)
        for jy in range(5):
            for jx in range(5):
                oy, ox = s * (jy - 2), s * (jx - 2)
                valid = shifted(surf, oy, ox, False)
                qc, qn, qz = shifted(cur, oy, ox, 0.0), shifted(n, oy, ox, 0.0), shifted(z, oy, ox, 1.0)
                e = np.zeros(surf.shape)
                with np.errstate(over="ignore"):
                    if sc > 0:
                        e += ((cur - qc) ** 2).sum(-1) / (sc * 2.0 ** -i) ** 2
                    if sn > 0:
                        e += ((n - qn) ** 2).sum(-1) / sn ** 2
                    if sz > 0:
                        e += ((z - qz) / (sz * z)) ** 2
                w = np.where(valid, H[jy] * H[jx] * np.exp(-e), 0.0)
                num += w[..., None] * qc
                den += w
        cur = np.where(s3, num / np.where(surf, den, 1.0)[..., None], 0.0)
    out = color.astype(np.float64)
    out[..., :3] = np.where(s3, cur * d, out[..., :3])
    return out
