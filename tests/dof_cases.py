"""Inputs the depth-of-field tests share (tests/test_dof_ref.py on the CPU, tests/test_gpu_dof.py on the GPU): the random images and
depths, and the images built against the kernels' tile-reach bound.  Everything is cached and never written."""
import functools

import numpy as np

from dof_ref import dof_ref

F, U = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
# what test_gpu_bloom.py's image() mixes into the colours and the alpha
SPECIALS = np.array([NAN, INF, -INF, -1.0, -3e38, 0.0, -0.0, 1e-40, -1e-40, 1e-45, 3e38, 65504.0, 70000.0], F)
ALPHA_PAYLOADS = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], U)
DEPTH_SPECIALS = np.array([NAN, INF, -INF, 0.0, -0.0, -1.0, 1e-40], F)


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def assert_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    bad = g != r
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[0]}"


@functools.lru_cache(maxsize=None)
def image(w, h, seed=0):
    """Radiance log-uniform over 2^-20 .. 2^12; about 1 % of the colour channels, and the first texels as far as they fit, hold a value
    that is no radiance; alpha holds NaN payloads, -0, infinities and a denormal."""
    rng = np.random.default_rng(1000 * w + h + seed)
    px = np.exp2(rng.uniform(-20, 12, (h, w, 4))).astype(F)
    odd = rng.uniform(size=(h, w, 3)) < 0.01
    px[..., :3] = np.where(odd, rng.choice(SPECIALS, (h, w, 3)), px[..., :3])
    flat = px.reshape(-1, 4)
    for k, s in enumerate(SPECIALS[:max(0, min(SPECIALS.size, flat.shape[0] - 2))]):
        flat[k, k % 3] = s
    px[..., 3] = np.resize(ALPHA_PAYLOADS, w * h).view(F).reshape(h, w)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def hit_image(w, h, seed=0):
    """A hit target: .w log-uniform over 2^-2 .. 2^6 with about 1 % of DEPTH_SPECIALS (and each of them once where they fit, from the
    last texel backwards); .xyz, which nothing reads, holds NaN and large numbers."""
    rng = np.random.default_rng(7000 * w + h + seed)
    px = np.empty((h, w, 4), F)
    px[..., :3] = rng.choice(np.array([NAN, 3e38, -1.0, 0.5], F), (h, w, 3))
    z = np.exp2(rng.uniform(-2, 6, (h, w))).astype(F)
    z = np.where(rng.uniform(size=(h, w)) < 0.01, rng.choice(DEPTH_SPECIALS, (h, w)), z).astype(F)
    flat = z.reshape(-1)
    for k, s in enumerate(DEPTH_SPECIALS[:max(0, min(DEPTH_SPECIALS.size, flat.size - 2))]):
        flat[flat.size - 1 - k] = s
    px[..., 3] = z
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def clean_image(w, h, seed=0):
    """Finite positive radiance only, so that every pixel is a lens pixel wherever the depth allows and a missed tap changes bits."""
    px = np.exp2(np.random.default_rng(31 * w + h + seed).uniform(-6, 6, (h, w, 4))).astype(F)
    px.setflags(write=False)
    return px


def hit_of(z):
    px = np.zeros(z.shape + (4,), F)
    px[..., 3] = z
    px.setflags(write=False)
    return px


# ---- the reach shortcut: a 64 x 64 image in focus everywhere (a = 0.5) with one pixel of a = 16 --------------------------------------
REACH_SIZE = 64
REACH_FOCUS = 8.0
REACH_PARAMS = {"focus_distance": REACH_FOCUS, "scale": 16.0, "max_radius": 16.0}
_TILE = {"corner_%d_%d" % p: p for p in ((16, 16), (31, 16), (16, 31), (31, 31))}            # of the interior tile x, y in 16..31
_TILE.update({"edge_%d_%d" % p: p for p in ((24, 16), (16, 24), (31, 24), (24, 31))})
_IMAGE = {"image_%d_%d" % p: p for p in ((0, 0), (63, 0), (0, 63), (63, 63))}
# 16 and 17 pixels from a tile seam: a reach of 16 from x = 48 ends on the first column of the tile 32..47, from 47 on the last column of
# 16..31 and from 16 on column 0; 49 and 15 lie one pixel further along
_SEAM = {"seam_x_%d" % x: (x, 24) for x in (15, 16, 47, 48, 49)}
_SEAM.update({"seam_y_%d" % y: (24, y) for y in (15, 16, 47, 48, 49)})
_SEAM.update({"seam_diag_%d" % v: (v, v) for v in (15, 16, 47, 48, 49)})
REACH_POSITIONS = {**_TILE, **_IMAGE, **_SEAM}
REACH_PLANES = {"nearer": REACH_FOCUS / 2.0, "farther": INF}           # K * |1 - s / z| = 16 at half the focus distance and at infinity


@functools.lru_cache(maxsize=None)
def reach_case(position, plane):
    """(src, hit, reference) of one pixel of a = 16 at REACH_POSITIONS[position], in the plane REACH_PLANES[plane]."""
    x, y = REACH_POSITIONS[position]
    z = np.full((REACH_SIZE, REACH_SIZE), REACH_FOCUS, F)
    z[y, x] = REACH_PLANES[plane]
    src, hit = clean_image(REACH_SIZE, REACH_SIZE), hit_of(z)
    ref = dof_ref(src, hit, **REACH_PARAMS)
    ref.setflags(write=False)
    return src, hit, ref


@functools.lru_cache(maxsize=None)
def rounding_case():
    """(src, hit, params, reference): one pixel of a = 15.5 + 2^-20 at a tile's first column — M + 0.5 would round to 16.0 and lose the
    taps 16 columns away, whose cov is 2^-20; M - 0.5 is exact."""
    z = np.full((REACH_SIZE, REACH_SIZE), REACH_FOCUS, F)
    z[24, 48] = REACH_FOCUS / 2.0
    z[24, 32] = INF                                                     # (its own weight is 1 / a^2, small enough for that tap to show)
    params = {"focus_distance": REACH_FOCUS, "scale": float(F(15.5) + F(2.0 ** -20)), "max_radius": 16.0}
    src, hit = clean_image(REACH_SIZE, REACH_SIZE, seed=1), hit_of(z)
    ref = dof_ref(src, hit, **params)
    ref.setflags(write=False)
    return src, hit, params, ref


@functools.lru_cache(maxsize=None)
def in_focus_tile_case():
    """(src, hit, reference): everything at a = 16 (the sky) but the interior tile, which is in focus."""
    z = np.full((REACH_SIZE, REACH_SIZE), INF, F)
    z[16:32, 16:32] = REACH_FOCUS
    src, hit = clean_image(REACH_SIZE, REACH_SIZE, seed=2), hit_of(z)
    ref = dof_ref(src, hit, **REACH_PARAMS)
    ref.setflags(write=False)
    return src, hit, ref


# ---- the closed forms ----------------------------------------------------------------------------------------------------------------
def depth_step(w=70, h=38, focus=4.0):
    """(src, hit, params): the left half in focus at `focus`, the right half far behind it (a = max_radius)."""
    z = np.full((h, w), focus, F)
    z[:, w // 2:] = 4096.0
    return clean_image(w, h, seed=3), hit_of(z), {"focus_distance": focus, "scale": 12.0, "max_radius": 8.0}
