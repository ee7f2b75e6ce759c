"""CPU: the closed forms of the depth-of-field restatement (tests/dof_ref.py, include/urt.h urt_depth_of_field) — what the header's
arithmetic gives exactly — and the legality of the kernels' tile-reach bound: restricting every pixel's loops to ceil(M - 0.5) changes no
bit, on the images built against that bound."""
import numpy as np
import pytest

import dof_cases as cases
from dof_cases import F, INF, NAN, assert_bits, bits
from dof_ref import FLAG_COC, coc_ref, dof_ref, tile_reach


def per_pixel_reach(src, hit, **params):
    a = coc_ref(src, hit, **params)[0]
    return np.repeat(np.repeat(tile_reach(a), 16, axis=0), 16, axis=1)[:a.shape[0], :a.shape[1]]


def test_scale_zero_returns_src():
    """Every lens pixel has a = 0.5 and only its own tap, w = 4: (4 c) / 4 = c, and +0 + 4 * -0 = +0.  focus_distance is small enough for
    s / z to stay finite at the denormal depth (the header: 0 * inf would be NaN and the radius max_radius)."""
    w, h = 70, 38
    src, hit = cases.image(w, h), cases.hit_image(w, h)
    out = dof_ref(src, hit, focus_distance=2.0 ** -10, scale=0.0, max_radius=16.0)
    lens = coc_ref(src, hit, focus_distance=2.0 ** -10, scale=0.0, max_radius=16.0)[2]
    neg_zero = (bits(src) == 0x80000000) & lens[..., None]                    # (a pass-through pixel keeps its bits)
    neg_zero[..., 3] = False
    assert neg_zero.any()
    assert_bits(out, np.where(neg_zero, F(0.0), src), "scale 0")
    assert np.array_equal(out[~np.isnan(src)], src[~np.isnan(src)])          # by value, every word
    a = coc_ref(src, hit, focus_distance=2.0 ** -10, scale=0.0, max_radius=16.0)[0]
    assert set(np.unique(a)) == {F(0.0), F(0.5)}
    assert (tile_reach(a) == 0).all()


def test_scale_zero_at_an_overflowing_distance_takes_max_radius():
    hit = cases.hit_of(np.array([[1e-40, 4.0]], F))
    a = coc_ref(np.ones((1, 2, 4), F), hit, focus_distance=10.0, scale=0.0, max_radius=3.0)[0]
    assert a.tolist() == [[3.0, 0.5]]                                         # fminf(NaN, Rmax) = Rmax


@pytest.mark.parametrize("params", [{}, {"scale": 0.0}, {"scale": 1e30, "max_radius": 16.0}, {"focus_distance": 0.3, "max_radius": 0.5},
                                    {"focus_distance": 3e38, "scale": 5.0, "max_radius": 3.0}], ids=str)
def test_a_constant_image_of_four_stays_four(params):
    """w * 4 is exact, so A = 4 S exactly, whatever the depths and the weights are."""
    w, h = 33, 17
    src = np.full((h, w, 4), 4.0, F)
    hit = cases.hit_image(w, h)
    out = dof_ref(src, hit, **params)
    assert_bits(out, src, f"constant {params}")


def test_a_sharp_foreground_stays_sharp_beside_a_blurred_background():
    src, hit, params = cases.depth_step()
    out = dof_ref(src, hit, **params)
    half = src.shape[1] // 2
    assert_bits(out[:, :half], src[:, :half], "the in-focus foreground")
    assert np.isfinite(out).all()
    far = out[:, half + 8:-8, :3]
    assert not np.array_equal(far, src[:, half + 8:-8, :3])
    assert far.std() < 0.25 * src[:, half + 8:-8, :3].std()                   # a disc of radius 8 averages some 200 pixels
    assert_bits(out[..., 3], src[..., 3], "alpha")
    a = coc_ref(src, hit, **params)[0]
    assert (a[:, :half] == 0.5).all() and (a[:, half:] == 8.0).all()


def test_pass_through_pixels_are_copied_and_are_never_taps():
    w, h = 33, 17
    src, hit = np.array(cases.image(w, h)), cases.hit_image(w, h)
    params = {"focus_distance": 4.0, "scale": 6.0, "max_radius": 16.0}
    a, _, lens = coc_ref(src, hit, **params)
    assert (~lens).sum() > 10 and lens.sum() > 100 and ((a == 0) == ~lens).all()
    out = dof_ref(src, hit, **params)
    assert_bits(out[~lens], src[~lens], "pass-through pixels")
    assert np.isfinite(out[lens][:, :3]).all()
    changed = src.copy()
    changed[~lens, :3] = np.where(np.isfinite(src[~lens, :3]) & (np.abs(src[~lens, :3]) <= 2.0 ** 100), F(NAN), F(3e38))   # still no lens pixel
    assert not coc_ref(changed, hit, **params)[2][~lens].any()
    again = dof_ref(changed, hit, **params)
    assert_bits(again[lens], out[lens], "lens pixels after the pass-through colours changed")
    coc = dof_ref(src, hit, flags=FLAG_COC, **params)
    assert_bits(coc[..., :3], np.repeat(a[..., None], 3, axis=2), "URT_DOF_FLAG_COC")
    assert_bits(coc[..., 3], src[..., 3], "alpha with URT_DOF_FLAG_COC")
    sky = coc_ref(np.ones((1, 1, 4), F), cases.hit_of(np.array([[INF]], F)), scale=6.0, max_radius=16.0)[0]
    assert sky[0, 0] == 6.0                                                   # min(K, Rmax), exactly


# ---- the tile-reach bound ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", sorted(cases.REACH_PLANES))
def test_tile_reach_changes_no_bit_around_one_wide_pixel(plane):
    for position in sorted(cases.REACH_POSITIONS):
        src, hit, ref = cases.reach_case(position, plane)
        reach = per_pixel_reach(src, hit, **cases.REACH_PARAMS)
        assert reach.max() == 16
        assert_bits(dof_ref(src, hit, reach=reach, **cases.REACH_PARAMS), ref, f"{position} {plane}")
        x, y = cases.REACH_POSITIONS[position]
        touched = (bits(ref[..., :3]) != bits(src[..., :3])).any(axis=2)
        if plane == "nearer":                                                 # the disc of radius 16.5 around it, and nothing outside
            yy, xx = np.mgrid[:cases.REACH_SIZE, :cases.REACH_SIZE]
            disc = (xx - x) ** 2 + (yy - y) ** 2 < 16.5 ** 2
            assert not touched[~disc].any() and touched.sum() > 0.95 * disc.sum()
            assert touched[y, min(x + 16, 63)] or touched[y, max(x - 16, 0)]  # as far as 16 columns away
        else:                                                                 # behind an in-focus image: it spreads onto nobody
            assert not touched.any()


def test_tile_reach_on_the_rounding_case_the_in_focus_tile_and_random_depths():
    src, hit, params, ref = cases.rounding_case()
    a = coc_ref(src, hit, **params)[0]
    assert a.max() == F(15.5) + F(2.0 ** -20) and tile_reach(a).max() == 16
    reach = per_pixel_reach(src, hit, **params)
    assert_bits(dof_ref(src, hit, reach=reach, **params), ref, "rounding case")
    short = dof_ref(src, hit, reach=np.minimum(reach, 15), **params)          # the tap 16 columns away counts, with cov = 2^-20
    assert (bits(short[24, 32, :3]) != bits(ref[24, 32, :3])).any()
    src, hit, ref = cases.in_focus_tile_case()
    reach = per_pixel_reach(src, hit, **cases.REACH_PARAMS)
    assert (reach == 16).all()
    assert_bits(dof_ref(src, hit, reach=reach, **cases.REACH_PARAMS), ref, "in-focus tile")
    for max_radius in (0.5, 3.0, 16.0):
        w, h = 70, 38
        src, hit = cases.image(w, h), cases.hit_image(w, h)
        params = {"focus_distance": 4.0, "scale": 6.0, "max_radius": max_radius}
        reach = per_pixel_reach(src, hit, **params)
        assert reach.max() == int(np.ceil(max_radius - 0.5))
        assert_bits(dof_ref(src, hit, reach=reach, **params), dof_ref(src, hit, **params), f"random depths, max_radius {max_radius}")
