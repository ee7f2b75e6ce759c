"""numpy restatement of urt_depth_of_field (include/urt.h "depth of field"): float32 with one rounding per operation, evaluated as the
header writes it, vectorised over the image and looped over the taps in the header's order (dy ascending outside, dx ascending inside).
No tiles: every pixel looks at all |dx|, |dy| <= 16.  Row 0 is the bottom, as everywhere; arrays are (H, W, channels).  The GPU results
are compared with these bit for bit."""
import numpy as np

F = np.float32
FLAG_COC = 1
MAX_REACH = 16
MAX_COLOR = F(2.0 ** 100)


def coc_ref(src, hit, focus_distance=10.0, scale=8.0, max_radius=8.0):
    """(a, z, lens): the blur radius (0 at a pass-through pixel, which no lens pixel has), hit.w and the class of every pixel.
    fminf / fmaxf are C's (np.fmin / np.fmax: of a NaN and a number, the number)."""
    src, hit = np.ascontiguousarray(src, dtype=F), np.ascontiguousarray(hit, dtype=F)
    z, c = hit[..., 3], src[..., :3]
    s, K, Rmax = F(focus_distance), F(scale), F(max_radius)
    with np.errstate(all="ignore"):
        lens = (z > F(0.0)) & (np.abs(c) <= MAX_COLOR).all(axis=-1)             # NaN fails every comparison
        a = np.fmax(np.fmin(np.abs(K * (F(1.0) - s / z)), Rmax), F(0.5)).astype(F)
    return np.where(lens, a, F(0.0)).astype(F), z, lens


def tile_reach(a, tile=16):
    """(ceil(H / tile), ceil(W / tile)) ints: the bound csrc/dof.hip puts on the loops of a tile — ceil(M - 0.5), M the largest a of the
    tile's 3 x 3 tile neighbourhood (a tap q counts only while d < a_q + 0.5)."""
    H, W = a.shape
    ty, tx = -(-H // tile), -(-W // tile)
    m = np.zeros((ty + 2, tx + 2), F)
    for j in range(ty):
        for i in range(tx):
            m[j + 1, i + 1] = a[j * tile:(j + 1) * tile, i * tile:(i + 1) * tile].max()
    M = np.max([m[j:j + ty, i:i + tx] for j in range(3) for i in range(3)], axis=0)
    return np.clip(np.ceil(M - F(0.5)), 0, MAX_REACH).astype(np.int32)


def dof_ref(src, hit, focus_distance=10.0, scale=8.0, max_radius=8.0, flags=0, reach=None):
    """urt_depth_of_field: dst (H, W, 4).  reach: None (all taps with |dx|, |dy| <= 16) or an (H, W) int array — a pixel then looks no
    further than its entry along an axis (the tile bound of the kernels, for the test that it changes nothing)."""
    src = np.ascontiguousarray(src, dtype=F)
    H, W = src.shape[:2]
    a, z, lens = coc_ref(src, hit, focus_distance, scale, max_radius)
    dst = src.copy()                                   # pass-through pixels and alpha: the same bits
    if flags & FLAG_COC:
        dst[..., :3] = a[..., None]
        return dst
    R = MAX_REACH
    ap = np.zeros((H + 2 * R, W + 2 * R), F)           # outside the image: a = 0, no tap
    zp = np.zeros_like(ap)
    cp = np.zeros((H + 2 * R, W + 2 * R, 3), F)
    ap[R:R + H, R:R + W], zp[R:R + H, R:R + W] = a, np.where(lens, z, F(0.0))
    cp[R:R + H, R:R + W] = np.where(lens[..., None], src[..., :3], F(0.0))
    S = np.zeros((H, W), F)
    A = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                aq, zq = ap[R + dy:R + dy + H, R + dx:R + dx + W], zp[R + dy:R + dy + H, R + dx:R + dx + W]
                take = lens & (aq > F(0.0))
                if reach is not None:
                    take = take & (reach >= max(abs(dx), abs(dy)))
                if not take.any():
                    continue
                d = np.sqrt(F(dx * dx + dy * dy))         # float32, correctly rounded: f_sqrt
                ae = np.where(zq > z, np.fmin(aq, a), aq).astype(F)
                cov = np.fmin(np.fmax((ae - d) + F(0.5), F(0.0)), F(1.0)).astype(F)
                take = take & (cov > F(0.0))           # a tap that does not count is skipped, not added as zero
                if not take.any():
                    continue
                w = (cov / (ae * ae)).astype(F)
                S = np.where(take, S + w, S)
                A = np.where(take[..., None], A + w[..., None] * cp[R + dy:R + dy + H, R + dx:R + dx + W], A)
        out = (A / S[..., None]).astype(F)
    dst[lens, :3] = out[lens]
    return dst
