"""float64 numpy restatement of urt_denoise (include/urt.h "denoising"): the edge-avoiding a-trous wavelet filter, literally as the header
states it.  Test helper only (not a conftest): tests/test_denoise_abi.py checks it on its own, tests/test_gpu_denoise.py checks the
library against it."""
import numpy as np

H = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def surface_mask(color, hit, normal):
    """(h, w) bool: the surface pixels; every other pixel passes through (rule 1)."""
    c, n = np.asarray(color, np.float32), np.asarray(normal, np.float32)
    z = np.asarray(hit, np.float32)[..., 3]
    with np.errstate(invalid="ignore"):
        return ((n[..., 3] != 0) & np.isfinite(z) & (z > 0) & np.isfinite(c[..., :3]).all(-1) & np.isfinite(n[..., :3]).all(-1))


def shifted(a, oy, ox, fill):
    """out[y, x] = a[y + oy, x + ox] where that is inside the image, else `fill`."""
    h, w = a.shape[:2]
    out = np.full(a.shape, fill, dtype=a.dtype)
    ys, yd = (slice(oy, h), slice(0, h - oy)) if oy >= 0 else (slice(0, h + oy), slice(-oy, h))
    xs, xd = (slice(ox, w), slice(0, w - ox)) if ox >= 0 else (slice(0, w + ox), slice(-ox, w))
    if yd.start < yd.stop and xd.start < xd.stop:
        out[yd, xd] = a[ys, xs]
    return out


def denoise_ref(color, hit, normal, albedo=None, iterations=5, sigma_color=8.0, sigma_normal=0.5, sigma_depth=0.1):
    """(h, w, 4) float64: rgb = the filtered colour of each surface pixel, alpha = src alpha; pass-through pixels hold src (as float64;
    the library must give the src texel's bits there).  Inputs are (h, w, 4) float32 images in the urt_render_aov layouts."""
    color = np.asarray(color, np.float32)
    surf = surface_mask(color, hit, normal)
    s3 = surf[..., None]
    c = np.where(s3, color[..., :3].astype(np.float64), 0.0)
    n = np.where(s3, np.asarray(normal, np.float32)[..., :3].astype(np.float64), 0.0)
    z = np.where(surf, np.asarray(hit, np.float32)[..., 3].astype(np.float64), 1.0)
    if albedo is not None:
        d = np.fmax(np.asarray(albedo, np.float32)[..., :3], np.float32(1e-3)).astype(np.float64)   # fmaxf: NaN gives 1e-3
    else:
        d = np.ones_like(c)
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
