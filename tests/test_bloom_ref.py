"""CPU: the numpy restatement of urt_bloom (tests/bloom_ref.py) held to include/urt.h "bloom" — the level sizes, the closed-form results
the header's arithmetic implies, every parameter's limit case, the exposure rule and the handling of values that are no radiance."""
import inspect

import numpy as np
import pytest

import bloom_ref as br
from bloom_ref import F, bloom_ref, downsample_ref, level_sizes, prefilter_ref, pyramid_ref, upsample_ref

U = np.uint32
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def hdr_image(w, h, seed=0, stops=(-6, 6)):
    """Positive radiance, log-uniform over the stops, alpha in [0, 1)."""
    rng = np.random.default_rng(100 * w + h + seed)
    px = np.exp2(rng.uniform(stops[0], stops[1], (h, w, 4))).astype(F)
    px[..., 3] = rng.uniform(0, 1, (h, w)).astype(F)
    return px


def test_level_sizes():
    assert level_sizes(1, 1) == [(1, 1)]                                           # L >= 1 always
    assert level_sizes(1, 9, 16) == [(1, 5), (1, 3), (1, 2), (1, 1)]
    assert level_sizes(17, 33, 8) == [(9, 17), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1)]
    assert level_sizes(17, 33, 3) == [(9, 17), (5, 9), (3, 5)]
    assert level_sizes(1920, 1080) == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    assert level_sizes(1920, 1080, 16) == level_sizes(1920, 1080, 6) + [(15, 9), (8, 5), (4, 3), (2, 2), (1, 1)]
    D, U_ = pyramid_ref(hdr_image(17, 33), levels=8)
    assert [(d.shape[1], d.shape[0]) for d in D] == level_sizes(17, 33, 8) and len(U_) == 6


def test_defaults_are_the_headers():
    sig = inspect.signature(bloom_ref).parameters
    assert {k: sig[k].default for k in ("threshold", "soft_knee", "clamp", "scatter", "intensity", "levels", "flags")} == \
        {"threshold": 1.0, "soft_knee": 0.5, "clamp": 65504.0, "scatter": 0.7, "intensity": 0.2, "levels": 6, "flags": 0}
    assert sig["exposure"].default is None and br.FLAG_ONLY == 1


def test_a_constant_image_blooms_to_a_constant():
    src = np.full((128, 64, 4), 4.0, F)
    dst, b = bloom_ref(src)
    assert (b == F(3.0)).all()                                                     # g = max(q, 3) / 4: every filter's weights sum to 1
    assert (dst[..., :3] == F(4.0) + F(3.0) * F(0.2)).all() and (dst[..., 3] == F(4.0)).all()
    only, _ = bloom_ref(src, flags=br.FLAG_ONLY)
    assert (only[..., :3] == F(3.0) * F(0.2)).all() and (only[..., 3] == F(4.0)).all()


@pytest.mark.parametrize("axis", [0, 1], ids=["y", "x"])
def test_mirroring_the_input_mirrors_the_bloom(axis):
    src = hdr_image(64, 128)                                                       # every level even down to 2 x 4
    _, b = bloom_ref(src, levels=5)
    _, bm = bloom_ref(np.flip(src, axis), levels=5)
    assert np.array_equal(bits(np.flip(bm, axis)), bits(b))


def test_below_the_threshold_nothing_is_added():
    src = hdr_image(33, 17, stops=(-8, -1.1))                                      # every channel below t - k = 0.5
    dst, b = bloom_ref(src)
    assert (bits(b) == 0).all()
    assert np.array_equal(bits(dst), bits(src))
    dst, b = bloom_ref(src, exposure=2.0, threshold=2.0)                           # t = 1 again
    assert (bits(b) == 0).all() and np.array_equal(bits(dst), bits(src))


def test_knee_zero_is_a_hard_threshold():
    src = hdr_image(40, 9, stops=(-2, 3))
    p = prefilter_ref(src, threshold=1.0, soft_knee=0.0)
    c = src[..., :3]
    m = c.max(axis=-1)
    assert (p[m <= F(1.0)] == 0).all()
    above = m > F(1.0)
    g = (m - F(1.0)) / m
    assert np.array_equal(bits(p[above]), bits(c[above] * g[above][:, None]))
    assert above.any() and (~above).any()


def test_threshold_zero_passes_the_image():
    src = hdr_image(40, 9, stops=(-20, 12))
    src[0, :4, :3] = [[1e-5, 1e-6, 0], [2e-5, 0, 0], [1e-7, 1e-7, 1e-7], [0, 0, 0]]
    p = prefilter_ref(src, threshold=0.0, soft_knee=0.7)
    c = src[..., :3]
    m = c.max(axis=-1)
    keep = m >= F(1e-5)
    assert np.array_equal(bits(p[keep]), bits(c[keep]))                            # g = m / m = 1
    assert (p[~keep] <= c[~keep]).all() and (~keep).sum() >= 2                     # below 1e-5 the gain is m / 1e-5 < 1


def test_clamp_bounds_every_prefiltered_channel():
    src = hdr_image(40, 9, stops=(-2, 14))
    for clamp, exposure in ((4.0, None), (0.5, None), (4.0, 8.0), (100.0, 1.0 / 64.0)):
        e = br.effective_exposure(exposure)
        cl = F(clamp) / e
        p = prefilter_ref(src, exposure, threshold=0.25, clamp=clamp)
        assert (p <= cl * (F(1.0) + F(4.0) * np.finfo(F).eps)).all(), (clamp, exposure, p.max(), cl)
        assert p.max() > F(0.9) * cl                                               # and the bound is reached


def test_values_that_are_no_radiance_give_a_finite_bloom():
    specials = np.array([NAN, INF, -INF, -1.0, -0.0, 0.0, 1e-40, 1e-45, 3e38, 70000.0], F)
    src = hdr_image(24, 20)
    rng = np.random.default_rng(3)
    src[..., :3] = np.where(rng.uniform(size=(20, 24, 3)) < 0.3, rng.choice(specials, (20, 24, 3)), src[..., :3])
    for img in (src, np.full((20, 24, 4), NAN, F), np.full((20, 24, 4), INF, F), np.full((20, 24, 4), -INF, F)):
        D, U_ = pyramid_ref(img, levels=16)
        assert all(np.isfinite(d).all() for d in D) and all(np.isfinite(u).all() for u in U_)
        dst, b = bloom_ref(img, levels=16)
        assert np.isfinite(b).all() and (b >= 0).all()
        assert np.array_equal(bits(dst[..., 3]), bits(img[..., 3]))                # alpha: the same bits, NaN payloads included
        assert np.array_equal(np.isnan(dst[..., :3]), np.isnan(img[..., :3]))      # NaN exactly where src is NaN
    _, b = bloom_ref(np.full((20, 24, 4), INF, F))
    assert (b > 0).all()                                                           # +inf counts as 65504
    for img in (np.full((20, 24, 4), NAN, F), np.full((20, 24, 4), -INF, F)):
        assert (bits(bloom_ref(img)[1]) == 0).all()


def test_scatter_limits():
    src = hdr_image(37, 21, stops=(-2, 6))
    D, U_ = pyramid_ref(src, scatter=0.0)
    assert all(np.array_equal(bits(u), bits(d)) for u, d in zip(U_, D))            # U_l = D_l + (..) * 0 = D_l
    _, b = bloom_ref(src, scatter=0.0)
    assert np.array_equal(bits(b), bits(upsample_ref(D[0], 37, 21)))
    D, U_ = pyramid_ref(src, scatter=1.0, levels=3)
    chain = D[2]
    for l in (1, 0):
        up = upsample_ref(chain, D[l].shape[1], D[l].shape[0])
        chain = (D[l] + (up - D[l]) * F(1.0)).astype(F)                            # the header's expression: up, but for its two roundings
        assert (np.abs(chain - up) <= np.finfo(F).eps * (np.abs(up - D[l]) + np.abs(up))).all()   # (each at most half an ulp of its result)
    assert np.array_equal(bits(U_[0]), bits(chain))


def test_levels_beyond_the_clip_change_nothing():
    src = hdr_image(17, 33, stops=(-2, 6))
    a, _ = bloom_ref(src, levels=6)
    for levels in (7, 8, 16):
        assert np.array_equal(bits(bloom_ref(src, levels=levels)[0]), bits(a))
    assert not np.array_equal(bits(bloom_ref(src, levels=5)[0]), bits(a))


def test_the_exposure_rule():
    one = F(1.0)
    for s in (0.0, -0.0, NAN, INF, -INF, -2.0, 2.0 ** -61, 2.0 ** 61, 1e-40):
        assert br.effective_exposure(s) == one, s
    for s in (2.0 ** -60, 2.0 ** 60, 0.5, 3.0):
        assert br.effective_exposure(s) == F(s), s
    assert br.effective_exposure(None) == one
    src = hdr_image(19, 11, stops=(-2, 6))
    plain = bloom_ref(src)[0]
    assert np.array_equal(bits(bloom_ref(src, exposure=2.0 ** -61)[0]), bits(plain))
    assert np.array_equal(bits(bloom_ref(src, exposure=NAN)[0]), bits(plain))
    assert np.array_equal(bits(bloom_ref(src, exposure=4.0)[0]), bits(bloom_ref(src, threshold=0.25, clamp=16376.0)[0]))
    assert not np.array_equal(bits(bloom_ref(src, exposure=4.0)[0]), bits(plain))
    assert np.isfinite(bloom_ref(src, exposure=2.0 ** -60, threshold=65504.0)[0]).all()    # t = 65504 * 2^60: finite


def test_the_filters_preserve_a_constant_and_the_mean_of_an_even_image():
    a = np.full((6, 10, 3), 0.37, F)
    assert (downsample_ref(a) == F(0.37)).all() and (upsample_ref(a, 20, 12) == F(0.37)).all()
    assert (upsample_ref(a, 19, 11) == F(0.37)).all()
    one = np.zeros((8, 8, 3), F)
    one[3, 4] = 64.0
    d = downsample_ref(one)                                                        # (4, 3) is fine column 1 of coarse x 2 / 3 ... the weights
    assert d.sum(axis=(0, 1)).tolist() == [16.0, 16.0, 16.0] and sorted(np.unique(d).tolist()) == [0.0, 1.0, 3.0, 9.0]
