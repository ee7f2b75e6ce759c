"""numpy restatement of urt_motion_blur (include/urt.h "motion blur"): float32 with one rounding per operation, evaluated as the header
writes it.  The velocities are vectorised over the image; the tile and neighbourhood maxima are plain loops over (value, index) keys;
the gather walks the tiles (the taps of a tile share their offsets, which is the header's rule, not a kernel's) and, inside one, the
header's k ascending.  It knows nothing of workgroups, waves or scratch.  Row 0 is the bottom, as everywhere; arrays are (H, W, channels).
The GPU results are compared with these bit for bit."""
import numpy as np

F = np.float32
FLAG_VELOCITY = 1
MAX_RADIUS = 16
TILE = 16
MAX_COLOR = F(2.0 ** 100)


def velocity_ref(src, motion, hit, shutter=0.5, max_radius=16.0):
    """(v, m, l, z, moving): the clamped half-shutter velocity (H, W, 2), its squared length and length (-1 at a pass-through pixel),
    hit.w and the class of every pixel.  fminf / fmaxf are C's (np.fmin / np.fmax)."""
    src, motion, hit = (np.ascontiguousarray(a, dtype=F) for a in (src, motion, hit))
    z, c = hit[..., 3], src[..., :3]
    h, R = F(shutter) * F(0.5), F(max_radius)
    with np.errstate(all="ignore"):
        moving = (z > F(0.0)) & (np.abs(c) <= MAX_COLOR).all(axis=-1)             # NaN fails every comparison
        valid = np.isfinite(motion[..., 0]) & np.isfinite(motion[..., 1]) & (motion[..., 2] > F(0.0))
        vx = np.where(valid, h * motion[..., 0], F(0.0)).astype(F)
        vy = np.where(valid, h * motion[..., 1], F(0.0)).astype(F)
        l = np.sqrt(vx * vx + vy * vy)                                            # float32, correctly rounded: f_sqrt
        s = R / l
        vx, vy = np.where(l > R, vx * s, vx).astype(F), np.where(l > R, vy * s, vy).astype(F)
        vx, vy = np.fmin(np.fmax(vx, -R), R), np.fmin(np.fmax(vy, -R), R)
        m = (vx * vx + vy * vy).astype(F)
        l = np.sqrt(m)
    v = np.stack([np.where(moving, vx, F(0.0)), np.where(moving, vy, F(0.0))], axis=-1).astype(F)
    return v, np.where(moving, m, F(-1.0)).astype(F), np.where(moving, l, F(-1.0)).astype(F), z, moving


def tile_velocity_ref(v, m):
    """(tv (ty, tx, 2), tm (ty, tx)): the v and m of each 16 x 16 tile's dominant pixel — the largest m, among equal m the lowest
    y * W + x.  A tile of pass-through pixels only: m = -1, v = (+0, +0)."""
    H, W = m.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    tv, tm = np.zeros((ty, tx, 2), F), np.full((ty, tx), -1.0, F)
    for j in range(ty):
        for i in range(tx):
            best = None
            for y in range(j * TILE, min((j + 1) * TILE, H)):
                for x in range(i * TILE, min((i + 1) * TILE, W)):
                    key = (-float(m[y, x]), y * W + x)                            # order-free: a minimum over (-m, index)
                    if best is None or key < best:
                        best = key
            y, x = divmod(best[1], W)
            tm[j, i] = m[y, x]
            if m[y, x] >= 0:
                tv[j, i] = v[y, x]
    return tv, tm


def neighbourhood_ref(tv, tm):
    """(n (ty, tx, 2), mn (ty, tx)): of the 3 x 3 tiles around each tile that lie inside the image, the one with the largest m, among
    equal m the first with dy ascending, then dx ascending."""
    ty, tx = tm.shape
    n, mn = np.zeros_like(tv), np.zeros_like(tm)
    for j in range(ty):
        for i in range(tx):
            best = None
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    jj, ii = j + dj, i + di
                    if 0 <= jj < ty and 0 <= ii < tx and (best is None or tm[jj, ii] > tm[best]):
                        best = (jj, ii)
            n[j, i], mn[j, i] = tv[best], tm[best]
    return n, mn


def line_offsets(nx, ny):
    """The (dx, dy) of a tile's taps for k = -M .. M, repeated pixels of the line left out."""
    nx, ny = F(nx), F(ny)
    M = int(np.ceil(np.fmax(np.abs(nx), np.abs(ny))))
    out, prev = [], None
    for k in range(-M, M + 1):
        dx = int(np.floor((F(k) * nx) / F(M) + F(0.5)))
        dy = int(np.floor((F(k) * ny) / F(M) + F(0.5)))
        if (dx, dy) != prev:
            out.append((dx, dy))
        prev = (dx, dy)
    return out


def motion_blur_ref(src, motion, hit, shutter=0.5, max_radius=16.0, flags=0):
    """urt_motion_blur: dst (H, W, 4)."""
    src = np.ascontiguousarray(src, dtype=F)
    H, W = src.shape[:2]
    v, m, l, z, moving = velocity_ref(src, motion, hit, shutter, max_radius)
    n, mn = neighbourhood_ref(*tile_velocity_ref(v, m))
    dst = src.copy()                                   # pass-through pixels, still tiles and alpha: the same bits
    R = MAX_RADIUS
    lp = np.full((H + 2 * R, W + 2 * R), -1.0, F)      # outside the image: no tap
    zp = np.zeros_like(lp)
    cp = np.zeros((H + 2 * R, W + 2 * R, 3), F)
    lp[R:R + H, R:R + W], zp[R:R + H, R:R + W], cp[R:R + H, R:R + W] = l, z, src[..., :3]
    for j in range(mn.shape[0]):
        for i in range(mn.shape[1]):
            y0, y1, x0, x1 = j * TILE, min((j + 1) * TILE, H), i * TILE, min((i + 1) * TILE, W)
            tile = (slice(y0, y1), slice(x0, x1))
            if flags & FLAG_VELOCITY:
                dst[tile][..., 0], dst[tile][..., 1] = n[j, i, 0], n[j, i, 1]
                dst[tile][..., 2] = np.where(moving[tile], l[tile], F(0.0))
                continue
            if not mn[j, i] >= F(0.25):                # a still tile
                continue
            l_p, z_p, mov = l[tile], z[tile], moving[tile]
            S = np.zeros(l_p.shape, F)
            A = np.zeros(l_p.shape + (3,), F)
            with np.errstate(all="ignore"):
                for dx, dy in line_offsets(n[j, i, 0], n[j, i, 1]):
                    q = (slice(R + y0 + dy, R + y1 + dy), slice(R + x0 + dx, R + x1 + dx))
                    l_q, z_q = lp[q], zp[q]
                    d = np.sqrt(F(dx * dx + dy * dy))
                    ae = np.where(z_q < z_p, np.fmax(l_q, F(0.5)), np.fmax(l_p, F(0.5))).astype(F)
                    cov = np.fmin(np.fmax(F(1.0) - d / ae, F(0.0)), F(1.0)).astype(F)
                    take = mov & (l_q >= F(0.0)) & (cov > F(0.0))                 # a tap that does not count is skipped, not added as zero
                    w = (cov / ae).astype(F)
                    S = np.where(take, S + w, S)
                    A = np.where(take[..., None], A + w[..., None] * cp[q], A)
                out = (A / S[..., None]).astype(F)
            dst[tile][..., :3] = np.where(mov[..., None], out, dst[tile][..., :3])
    return dst
