"""numpy restatement of urt_bloom (include/urt.h "bloom"): float32 with one rounding per operation, evaluated as the header writes it,
vectorised over the image.  Row 0 is the bottom, as everywhere; arrays are (H, W, channels).  The GPU results are compared with these
bit for bit."""
import numpy as np

F = np.float32
FLAG_ONLY = 1
HALF_MAX = F(65504.0)
TINY = F(1e-5)


def level_sizes(W, H, levels=6):
    """[(w_1, h_1), .., (w_L, h_L)]: w_l = (w_{l-1} + 1) >> 1, L = min(levels, the first l with w_l == h_l == 1)."""
    out, w, h = [], int(W), int(H)
    for _ in range(int(levels)):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
        if w == 1 and h == 1:
            break
    return out


def effective_exposure(exposure):
    """e: the state's exposure when 2^-60 <= s <= 2^60 (NaN fails), else 1; exposure None = no d_state."""
    if exposure is None:
        return F(1.0)
    s = F(exposure)
    with np.errstate(all="ignore"):
        return s if (s >= F(2.0 ** -60) and s <= F(2.0 ** 60)) else F(1.0)


def prefilter_ref(src, exposure=None, threshold=1.0, soft_knee=0.5, clamp=65504.0):
    """(H, W, 3): level 0, the prefiltered colour channels of src."""
    e = effective_exposure(exposure)
    t, cl = F(threshold) / e, F(clamp) / e
    k = t * F(soft_knee)
    c = np.ascontiguousarray(src, dtype=F)[..., :3]
    with np.errstate(all="ignore"):
        c = np.where(c > F(0.0), np.minimum(c, HALF_MAX), F(0.0)).astype(F)
        m = np.maximum(np.maximum(c[..., 0], c[..., 1]), c[..., 2])
        q = np.minimum(np.maximum((m - t) + k, F(0.0)), F(2.0) * k)
        q = (q * q) / (F(4.0) * k + TINY)
        g = np.maximum(q, m - t) / np.maximum(m, TINY)
        g = g * np.minimum(F(1.0), cl / np.maximum(m, TINY))
        return (c * g[..., None]).astype(F)


def downsample_ref(a):
    """D_l from level l-1: the binomial [1 3 3 1]^2 / 64, horizontal first, edges clamped."""
    h0, w0 = a.shape[:2]
    w1, h1 = (w0 + 1) >> 1, (h0 + 1) >> 1
    xs = [np.clip(2 * np.arange(w1) - 1 + j, 0, w0 - 1) for j in range(4)]
    ys = [np.clip(2 * np.arange(h1) - 1 + j, 0, h0 - 1) for j in range(4)]
    hrow = (a[:, xs[0]] + a[:, xs[3]]) + F(3.0) * (a[:, xs[1]] + a[:, xs[2]])
    return (((hrow[ys[0]] + hrow[ys[3]]) + F(3.0) * (hrow[ys[1]] + hrow[ys[2]])) * F(0.015625)).astype(F)


def upsample_ref(a, w, h):
    """up(a) on the w x h grid of the next finer level."""
    h1, w1 = a.shape[:2]
    x, y = np.arange(w), np.arange(h)
    nx, ny = x >> 1, y >> 1
    fx = np.clip(nx + np.where(x & 1, 1, -1), 0, w1 - 1)
    fy = np.clip(ny + np.where(y & 1, 1, -1), 0, h1 - 1)
    hrow = F(3.0) * a[:, nx] + a[:, fx]
    return ((F(3.0) * hrow[ny] + hrow[fy]) * F(0.0625)).astype(F)


def pyramid_ref(src, exposure=None, threshold=1.0, soft_knee=0.5, clamp=65504.0, scatter=0.7, levels=6):
    """(D, U): the lists D_1..D_L and U_1..U_L (index 0 is level 1), each (h_l, w_l, 3)."""
    H, W = src.shape[:2]
    a = prefilter_ref(src, exposure, threshold, soft_knee, clamp)
    D = []
    for _ in level_sizes(W, H, levels):
        a = downsample_ref(a)
        D.append(a)
    U = [None] * len(D)
    U[-1] = D[-1]
    for l in range(len(D) - 2, -1, -1):
        up = upsample_ref(U[l + 1], D[l].shape[1], D[l].shape[0])
        U[l] = (D[l] + (up - D[l]) * F(scatter)).astype(F)
    return D, U


def bloom_ref(src, exposure=None, threshold=1.0, soft_knee=0.5, clamp=65504.0, scatter=0.7, intensity=0.2, levels=6, flags=0):
    """urt_bloom: (dst, b) with b = up(U_1) on the W x H grid, (H, W, 3).  exposure None = no d_state, else the state's exposure."""
    src = np.ascontiguousarray(src, dtype=F)
    H, W = src.shape[:2]
    _, U = pyramid_ref(src, exposure, threshold, soft_knee, clamp, scatter, levels)
    b = upsample_ref(U[0], W, H)
    dst = src.copy()                                   # alpha: the same bits
    with np.errstate(all="ignore"):
        glow = b * F(intensity)
        dst[..., :3] = glow if flags & FLAG_ONLY else src[..., :3] + glow
    return dst, b
