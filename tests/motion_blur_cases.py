"""Inputs the motion-blur tests share (tests/test_motion_blur_ref.py on the CPU, tests/test_gpu_motion_blur.py on the GPU): the motion
images and the small scenes.  The random colour and depth images are the depth-of-field tests' (tests/dof_cases.py).  Everything is cached
and never written."""
import functools

import numpy as np

from dof_cases import F, INF, NAN, U, assert_bits, bits, clean_image, hit_image, hit_of, image  # noqa: F401  (re-exported)

TWO_100 = float(2.0 ** 100)


def frozen(a):
    a = np.ascontiguousarray(a, F)
    a.setflags(write=False)
    return a


def motion_of(mx, my, valid=1.0):
    """A motion image as urt_reproject* writes it: (qx - x, qy - y, S, 0); mx, my (H, W) arrays."""
    mx, my = np.asarray(mx, F), np.asarray(my, F)
    px = np.zeros(mx.shape + (4,), F)
    px[..., 0], px[..., 1], px[..., 2] = mx, my, valid
    return frozen(px)


@functools.lru_cache(maxsize=None)
def pan(w, h, mx, my):
    return motion_of(np.full((h, w), mx, F), np.full((h, w), my, F))


@functools.lru_cache(maxsize=None)
def flat_hit(w, h, z=4.0):
    return hit_of(np.full((h, w), z, F))


@functools.lru_cache(maxsize=None)
def random_motion(w, h, seed=0, scale=12.0):
    """Smooth-less random vectors of up to `scale` pixels per axis; about 3 % of the texels hold a vector that is none: .z of 0, -1 or
    NaN, NaN and infinite components, a huge finite one."""
    rng = np.random.default_rng(500 * w + h + seed)
    px = np.zeros((h, w, 4), F)
    px[..., :2] = rng.uniform(-scale, scale, (h, w, 2))
    px[..., 2] = rng.choice(np.array([1.0, 3.0, 0.25], F), (h, w))
    px[..., 3] = rng.choice(np.array([0.0, NAN, 7.0], F), (h, w))                # (nothing reads it)
    odd = rng.uniform(size=(h, w)) < 0.03
    kinds = rng.integers(0, 7, (h, w))
    for k, (c, val) in enumerate(((2, 0.0), (2, -1.0), (2, NAN), (0, NAN), (1, INF), (0, -INF), (1, 3e38))):
        sel = odd & (kinds == k)
        px[..., c] = np.where(sel, F(val), px[..., c])
    return frozen(px)


# ---- the moving disc: a frame, its motion and depth, and the mean of the sub-frame positions ------------------------------------------
DISC = {"w": 96, "h": 64, "radius": 12.0, "move": 12.0, "centre": (48.0, 32.0), "subframes": 64}


def _disc_frame(cx, cy):
    w, h, r = DISC["w"], DISC["h"], DISC["radius"]
    y, x = np.mgrid[0:h, 0:w]
    board = (((x // 8) + (y // 8)) % 2).astype(F) * F(0.8) + F(0.1)
    inside = (x + 0.5 - cx) ** 2 + (y + 0.5 - cy) ** 2 <= r * r
    rgb = np.where(inside[..., None], np.array([1.0, 0.25, 0.05], F), board[..., None]).astype(F)
    return rgb, inside


@functools.lru_cache(maxsize=None)
def moving_disc():
    """(src, motion, hit, truth): a disc of radius 12 in front of a checkerboard, 12 pixels along +x per frame, as one frame shows it
    (src), with the motion image (the disc's points were 12 pixels to the left) and the depth; truth is the mean of the frame at 64
    disc positions spread evenly over the open shutter (shutter = 1: half the move to either side of the frame's position)."""
    cx, cy = DISC["centre"]
    rgb, inside = _disc_frame(cx, cy)
    src = np.ones(rgb.shape[:2] + (4,), F)
    src[..., :3] = rgb
    motion = motion_of(np.where(inside, F(-DISC["move"]), F(0.0)), np.zeros(inside.shape, F))
    hit = hit_of(np.where(inside, F(1.0), F(2.0)).astype(F))
    n = DISC["subframes"]
    offsets = (np.arange(n) + 0.5) / n * DISC["move"] - DISC["move"] / 2.0
    truth = np.mean([_disc_frame(cx + o, cy)[0].astype(np.float64) for o in offsets], axis=0)
    return frozen(src), motion, hit, truth


@functools.lru_cache(maxsize=None)
def still_disc_over_pan(w=64, h=48, mx=9.0, my=-4.0):
    """(src, motion, hit, interior): a still disc of radius 10 in front of a background that pans by (mx, my); interior marks the
    disc's pixels."""
    y, x = np.mgrid[0:h, 0:w]
    inside = (x + 0.5 - w / 2) ** 2 + (y + 0.5 - h / 2) ** 2 <= 100.0
    motion = motion_of(np.where(inside, F(0.0), F(mx)), np.where(inside, F(0.0), F(my)))
    hit = hit_of(np.where(inside, F(1.5), F(6.0)).astype(F))
    return clean_image(w, h, seed=5), motion, hit, inside


@functools.lru_cache(maxsize=None)
def moving_disc_over_still(w=64, h=48, mx=-7.0, my=10.0):
    """(src, motion, hit, interior): the reverse — the disc moves, the background is still."""
    src, _, hit, inside = still_disc_over_pan(w, h)
    motion = motion_of(np.where(inside, F(mx), F(0.0)), np.where(inside, F(my), F(0.0)))
    return src, motion, hit, inside


@functools.lru_cache(maxsize=None)
def one_fast_pixel(w=80, h=48, at=(40, 24), mx=36.0, my=10.0):
    """(src, motion, hit): everything still but one pixel, nearer than the rest, in the tile (2, 1) of a 5 x 3 tile grid: the tiles next
    to it take its velocity (at shutter = 1 its streak, clamped to 16 pixels, reaches into the tiles left and right of its own), the
    tiles two away stay copies."""
    mxs, mys = np.zeros((h, w), F), np.zeros((h, w), F)
    mxs[at[1], at[0]], mys[at[1], at[0]] = mx, my
    z = np.full((h, w), 4.0, F)
    z[at[1], at[0]] = 1.0
    return clean_image(w, h, seed=6), motion_of(mxs, mys), hit_of(z)


@functools.lru_cache(maxsize=None)
def equal_m_in_one_tile(w=33, h=31):
    """(src, motion, hit): two pixels of one tile with velocities of equal m and different direction, (6, 8) at the LATER index and
    (-8, 6) at the earlier one — the earlier one is dominant."""
    mxs, mys = np.zeros((h, w), F), np.zeros((h, w), F)
    mxs[5, 9], mys[5, 9] = -8.0, 6.0
    mxs[3, 12], mys[3, 12] = 6.0, 8.0                                            # y * W + x is lower here: row 3
    return clean_image(w, h, seed=7), motion_of(mxs, mys), flat_hit(w, h)


@functools.lru_cache(maxsize=None)
def equal_m_in_two_tiles(w=48, h=48):
    """(src, motion, hit): the tiles (0, 2) and (2, 0) (x, y) hold one pixel each of equal m; the centre tile and the other tiles
    that see both take the first in dy ascending, dx ascending order: (2, 0)'s."""
    mxs, mys = np.zeros((h, w), F), np.zeros((h, w), F)
    mxs[40, 4], mys[40, 4] = 3.0, -4.0                                           # tile x 0, y 2
    mxs[6, 44], mys[6, 44] = -4.0, 3.0                                           # tile x 2, y 0
    return clean_image(w, h, seed=8), motion_of(mxs, mys), flat_hit(w, h)


@functools.lru_cache(maxsize=None)
def sky_beside_surface(w=40, h=24):
    """(src, motion, hit): the left half a surface that moves, the right half the sky (z = +inf), still."""
    z = np.full((h, w), 3.0, F)
    z[:, w // 2:] = INF
    mxs = np.zeros((h, w), F)
    mxs[:, :w // 2] = 10.0
    return clean_image(w, h, seed=9), motion_of(mxs, np.zeros((h, w), F)), hit_of(z)


@functools.lru_cache(maxsize=None)
def bright_pan(w=48, h=48):
    """(src, motion, hit): every colour channel +-2^100 exactly, a diagonal pan at the full radius: 33 taps of the largest moving colour."""
    rng = np.random.default_rng(10)
    src = (rng.choice(np.array([TWO_100, -TWO_100], F), (h, w, 4))).astype(F)
    return frozen(src), pan(w, h, 40.0, -40.0), flat_hit(w, h)


@functools.lru_cache(maxsize=None)
def odd_colours_beside_moving(w=33, h=31):
    """(src, motion, hit): a panning image in which every fourth pixel has a colour that is none (NaN, inf, above 2^100) and passes
    through."""
    src = np.array(clean_image(w, h, seed=11))
    flat = src.reshape(-1, 4)
    for k, val in enumerate((NAN, INF, -INF, 2.0 ** 101, -3e38)):
        flat[k::20, k % 3] = val
    return frozen(src), pan(w, h, 6.0, 3.0), flat_hit(w, h)
