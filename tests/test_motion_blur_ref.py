"""CPU: properties of the numpy restatement of urt_motion_blur (tests/motion_blur_ref.py) itself — the closed forms of include/urt.h
"motion blur" and the quality of the result against a supersampled shutter.  The GPU tests compare the kernels with this restatement bit
for bit; these tests say that the restatement is worth comparing with."""
import numpy as np

import motion_blur_cases as cases
from motion_blur_cases import F, INF, NAN, assert_bits, bits
from motion_blur_ref import FLAG_VELOCITY, line_offsets, motion_blur_ref, neighbourhood_ref, tile_velocity_ref, velocity_ref


def test_zero_motion_and_a_closed_shutter_return_the_image_bit_for_bit():
    w, h = 70, 50
    src, hit = cases.image(w, h), cases.hit_image(w, h)
    assert_bits(motion_blur_ref(src, cases.pan(w, h, 0.0, 0.0), hit), src, "zero motion")
    assert_bits(motion_blur_ref(src, cases.random_motion(w, h), hit, shutter=0.0), src, "shutter 0")
    invalid = np.array(cases.random_motion(w, h))
    invalid[..., 2] = 0.0
    assert_bits(motion_blur_ref(src, invalid, hit, shutter=1.0), src, "motion.z == 0 everywhere")
    # below half a pixel of half-shutter velocity nothing is gathered either: 0.5 * 0.9 = 0.45
    assert_bits(motion_blur_ref(src, cases.pan(w, h, 0.9, 0.0), hit), src, "a streak below half a pixel")


def test_a_uniform_pan_of_a_constant_image_returns_the_constant():
    w, h = 48, 33
    const = np.full((h, w, 4), 3.0, F)
    for mx, my in ((32.0, 0.0), (0.0, -9.0), (7.0, 7.0), (6.4, -3.4), (100.0, 40.0)):
        out = motion_blur_ref(const, cases.pan(w, h, mx, my), cases.flat_hit(w, h))
        # A / S with A = sum(w * 3) and S = sum(w) over at most 33 taps: each sum carries at most 33 roundings of 2^-24 relative
        assert np.abs(out[..., :3] - 3.0).max() <= 3.0 * 2 * 33 * 2.0 ** -24, (mx, my)
        assert_bits(out[..., 3], const[..., 3], "alpha")


def test_pass_through_pixels_are_copied_and_never_gathered():
    src, motion, hit = cases.odd_colours_beside_moving()
    moving = velocity_ref(src, motion, hit)[4]
    assert (~moving).sum() > 20 and moving.sum() > 500
    out = motion_blur_ref(src, motion, hit)
    assert_bits(out[~moving], src[~moving], "pass-through pixels")
    assert np.isfinite(out[moving]).all()                                        # no NaN or inf colour reached a moving pixel
    changed = np.array(src)
    changed[~moving, :3] = np.where(np.isnan(src[~moving, :3]), F(INF), F(NAN))
    again = motion_blur_ref(changed, motion, hit)
    assert_bits(again[moving], out[moving], "moving pixels after the pass-through colours changed")
    # depth decides the class as well
    z = np.array(hit)
    z[5, 7, 3], z[6, 7, 3], z[7, 7, 3] = NAN, 0.0, -2.0
    out = motion_blur_ref(src, motion, z)
    assert_bits(out[5:8, 7], src[5:8, 7], "NaN, zero and negative hit.w")


def test_the_velocity_is_clamped_to_the_radius_and_the_offsets_to_16():
    w, h = 8, 8
    src, hit = cases.clean_image(w, h), cases.flat_hit(w, h)
    for R in (0.5, 4.0, 16.0):
        for mx, my in ((1000.0, 0.0), (-300.0, 400.0), (3e38, 3e38), (33.0, -33.0)):
            v, m, l, _, _ = velocity_ref(src, cases.pan(w, h, mx, my), hit, shutter=1.0, max_radius=R)
            assert (np.abs(v) <= R).all() and (l <= F(R) * F(1 + 2.0 ** -22)).all()
    for nx, ny in ((16.0, 16.0), (-16.0, 3.3), (0.4, -0.3), (15.999999, 0.5), (1.6, -0.85)):
        offs = line_offsets(nx, ny)
        assert (0, 0) in offs and len(offs) == len(set(offs)) <= 33
        assert max(max(abs(dx), abs(dy)) for dx, dy in offs) <= 16
    assert len(line_offsets(16.0, -16.0)) == 33
    assert len(line_offsets(3.2, -1.7)) < 9                                      # M = 4 and steps of (0.8, -0.425): repeated k


def test_tie_rules():
    src, motion, hit = cases.equal_m_in_one_tile()
    v, m, *_ = velocity_ref(src, motion, hit, shutter=1.0)
    tv, tm = tile_velocity_ref(v, m)
    assert tm[0, 0] == 25.0 and tuple(tv[0, 0]) == (3.0, 4.0)                    # the pixel of row 3, not the one of row 5
    src, motion, hit = cases.equal_m_in_two_tiles()
    v, m, *_ = velocity_ref(src, motion, hit, shutter=1.0)
    n, mn = neighbourhood_ref(*tile_velocity_ref(v, m))
    assert tuple(n[1, 1]) == (-2.0, 1.5) and mn[1, 1] == 6.25                    # dy ascending first: the tile of row 0
    assert tuple(n[2, 0]) == (1.5, -2.0) and tuple(n[0, 2]) == (-2.0, 1.5)       # each corner tile sees its own alone
    assert mn[0, 0] == 0.0 and mn[2, 2] == 0.0                                   # two away from one, diagonal to none


def test_a_fast_pixel_reaches_the_tiles_next_door_and_no_further():
    src, motion, hit = cases.one_fast_pixel()
    out = motion_blur_ref(src, motion, hit, shutter=1.0)
    same = (bits(out) == bits(src)).all(axis=-1)
    assert same[:, :16].all() and same[:, 64:].all()                             # tile columns 0 and 4: two away, copies
    assert not same[16:32, 32:48].all()                                          # its own tile is gathered along its velocity
    assert not same[16:32, 16:32].all() and not same[16:32, 48:64].all()         # 15 pixels along the line: the tiles left and right
    assert same[:16].all() and same[32:].all()                                   # gathered along a line that meets nothing: a lone tap returns its colour


def test_the_velocity_flag():
    src, motion, hit = cases.one_fast_pixel()
    out = motion_blur_ref(src, motion, hit, shutter=1.0, flags=FLAG_VELOCITY)
    v, m, l, _, _ = velocity_ref(src, motion, hit, shutter=1.0)
    assert_bits(out[..., 3], src[..., 3], "alpha")
    assert_bits(out[..., 2], l, "l_p")
    near = np.zeros(l.shape, bool)
    near[:, 16:64] = True
    assert (out[near][:, :2] == v[24, 40]).all() and (out[~near][:, :2] == 0).all()


def rmse(a, truth):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64)[..., :3] - truth) ** 2)))


def test_quality_against_the_mean_of_64_subframe_positions():
    src, motion, hit, truth = cases.moving_disc()
    out = motion_blur_ref(src, motion, hit, shutter=1.0)
    blurred, plain = rmse(out, truth), rmse(src, truth)
    print(f"moving disc: RMSE blurred {blurred:.4f}, unblurred {plain:.4f}, ratio {blurred / plain:.3f}")
    assert blurred <= 0.75 * plain
    assert_bits(out[..., 3], src[..., 3], "alpha")


def test_a_still_foreground_over_a_panning_background_keeps_its_interior():
    src, motion, hit, inside = cases.still_disc_over_pan()
    out = motion_blur_ref(src, motion, hit, shutter=1.0)
    # every tap of a disc pixel that lies behind it has ae = max(l_p, 0.5) = 0.5 and d >= 1: cov = 0; the disc's own pixels likewise
    assert inside.sum() > 250
    assert_bits(out[inside], src[inside], "the still disc")
    assert not (bits(out[~inside]) == bits(src[~inside])).all()
    # the reverse: a moving disc smears over the still background next to it
    src, motion, hit, inside = cases.moving_disc_over_still()
    out = motion_blur_ref(src, motion, hit, shutter=1.0)
    ring = ~inside & np.roll(inside, 3, axis=0)                                  # background pixels three rows above disc pixels: along (-7, 10)
    assert ring.any() and not (bits(out[ring]) == bits(src[ring])).all(axis=-1).all()
