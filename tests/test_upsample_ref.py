"""CPU: the float32 restatement of urt_upsample (tests/upsample_ref.py) against the properties include/urt.h promises — the GPU tests
(tests/test_gpu_upsample.py) then hold the kernel to the restatement bit for bit."""
import numpy as np

from upsample_ref import SKY_FROM_ALBEDO, WIDE_FALLBACK, low_grid_position, synthetic_case, synthetic_guides, upsample_ref

F = np.float32


def guides_and_color(w, h, W, H, seed=0):
    c = synthetic_case(w, h, W, H, seed, sprinkle=False)
    return c


def call(c, **kw):
    return upsample_ref(c["low_color"], c["low_hit"], c["low_normal"], c["low_id"], c["hit"], c["normal"], c["id"], **kw)


def test_equal_sizes_and_identical_guides_return_the_input():
    c = guides_and_color(16, 12, 16, 12, seed=3)
    r = call(c, low_count=c["low_count"])
    assert (r["surface"] | r["sky"]).all() and r["result"].all() and not r["stage2"].any()
    assert r["color"].tobytes() == c["low_color"].tobytes()
    assert r["count"].tobytes() == c["low_count"].tobytes()
    assert (low_grid_position(16, 16) == np.arange(16, dtype=F)).all()       # q = X exactly: one tap of weight 1


def test_all_ones_at_ratio_two_return_exactly_one():
    c = guides_and_color(12, 8, 24, 16, seed=1)
    c["low_color"][:] = 1.0
    q = low_grid_position(24, 12)
    assert set(np.unique(q - np.floor(q)).tolist()) == {0.25, 0.75}          # the weights 9/16, 3/16, 3/16, 1/16: exact in float32
    r = call(c)
    assert r["result"].mean() > 0.9
    assert (r["color"][r["result"]] == 1.0).all() and (r["count"][r["result"]][:, 0] == 1.0).all()
    assert (r["color"][~r["result"]] == 0).all() and (r["count"][~r["result"]] == 0).all()
    assert (r["count"][..., 1:] == 0).all()


def test_no_pixel_mixes_colours_across_an_id_boundary():
    w, h, W, H = 8, 6, 24, 18
    low_hit = np.zeros((h, w, 4), F)
    low_hit[..., 2], low_hit[..., 3] = 5.0, 5.0                              # one plane z = 5, facing the camera
    low_normal = np.zeros((h, w, 4), F)
    low_normal[..., 2], low_normal[..., 3] = -1.0, 3.0
    low_id = np.zeros((h, w, 4), np.int32)
    low_id[:, w // 2:, 0] = 1                                                # two objects, split down the middle
    hit = np.zeros((H, W, 4), F)
    hit[..., 2], hit[..., 3] = 5.0, 5.0
    normal = np.zeros((H, W, 4), F)
    normal[..., 2], normal[..., 3] = -1.0, 3.0
    ids = np.zeros((H, W, 4), np.int32)
    ids[:, W // 2:, 0] = 1
    low_color = np.zeros((h, w, 4), F)
    low_color[:, :w // 2] = (1.0, 0.0, 0.0, 1.0)                             # red left, blue right
    low_color[:, w // 2:] = (0.0, 0.0, 1.0, 1.0)
    r = upsample_ref(low_color, low_hit, low_normal, low_id.view(F), hit, normal, ids.view(F))
    assert r["result"].all()
    left = ids[..., 0] == 0
    assert (r["color"][left] == np.array([1, 0, 0, 1], F)).all() and (r["color"][~left] == np.array([0, 0, 1, 1], F)).all()
    # the plain bilinear weights would have mixed the two columns next to the boundary
    q = low_grid_position(W, w)
    assert ((np.floor(q) == w // 2 - 1) & (q - np.floor(q) > 0)).any()


def test_stage_two_serves_a_pixel_whose_four_taps_fail():
    c = guides_and_color(8, 8, 16, 16, seed=2)
    c["low_hit"][...] = c["low_hit"][0, 0]                                   # one flat ground everywhere, on both grids
    c["low_normal"][...] = c["low_normal"][0, 0]
    c["low_id"][...] = c["low_id"][0, 0]
    c["hit"][...] = c["low_hit"][0, 0]
    c["normal"][...] = c["low_normal"][0, 0]
    c["id"][...] = c["low_id"][0, 0]
    X, Y = 8, 8                                                              # q = (3.75, 3.75): taps (3..4, 3..4)
    c["low_count"][3:5, 3:5, 0] = 0.0
    with_flag = call(c, low_count=c["low_count"], flags=WIDE_FALLBACK)
    without = call(c, low_count=c["low_count"], flags=0)
    assert with_flag["stage2"][Y, X] and with_flag["result"][Y, X]
    ring = np.ones((4, 4), bool)
    ring[1:3, 1:3] = False
    block_c, block_n = c["low_color"][2:6, 2:6][ring], c["low_count"][2:6, 2:6, 0][ring]
    S, A, N = F(0), np.zeros(4, F), F(0)
    for col, n in zip(block_c, block_n):                                     # j outer, i inner: the order of the boolean mask
        S = S + F(1)
        A = A + col
        N = N + n
    assert with_flag["color"][Y, X].tobytes() == (A / S).astype(F).tobytes()
    assert with_flag["count"][Y, X, 0] == N / S
    assert not without["result"][Y, X]
    assert (without["color"][Y, X] == 0).all() and (without["count"][Y, X] == 0).all()
    # a pixel that has a stage-1 result is the same with and without the flag
    s1 = without["result"]
    assert s1.sum() > 200 and with_flag["color"][s1].tobytes() == without["color"][s1].tobytes()


def test_bad_colours_and_counts_are_skipped():
    c = guides_and_color(8, 8, 8, 8, seed=4)                                 # equal sizes: pixel (X, Y) has the one tap (X, Y)
    good = call(c, low_count=c["low_count"], flags=0)
    assert good["result"].all()
    bad = {k: v.copy() for k, v in c.items()}
    bad["low_color"][1, 1, 2] = np.nan
    bad["low_color"][2, 2, 0] = np.inf
    bad["low_color"][2, 3, 3] = -np.inf
    bad["low_count"][3, 3, 0] = 0.0
    bad["low_count"][4, 4, 0] = -2.0
    bad["low_count"][5, 5, 0] = np.nan
    bad["low_count"][6, 6, 0] = np.inf
    r = call(bad, low_count=bad["low_count"], flags=0)
    skipped = np.zeros((8, 8), bool)
    for y, x in ((1, 1), (2, 2), (2, 3), (3, 3), (4, 4), (5, 5), (6, 6)):
        skipped[y, x] = True
    assert (r["result"] == ~skipped).all()
    assert (r["color"][skipped] == 0).all() and (r["count"][skipped] == 0).all()
    assert r["color"][~skipped].tobytes() == good["color"][~skipped].tobytes()
    # with the fallback the neighbours serve those pixels, and never with a value that is not finite
    r = call(bad, low_count=bad["low_count"], flags=WIDE_FALLBACK)
    assert np.isfinite(r["color"]).all() and np.isfinite(r["count"]).all()
    # without a count image every texel counts 1
    r = call(bad, flags=0)
    assert r["result"][3, 3] and r["count"][3, 3, 0] == 1.0 and not r["result"][1, 1]


def test_sky_from_albedo_replaces_rgb_only_where_a_result_exists():
    c = guides_and_color(10, 10, 20, 20, seed=5)
    sky_low = c["low_normal"][..., 3] == 0
    assert sky_low.any()
    c["low_count"][sky_low & (np.arange(10)[None, :] < 5), 0] = 0.0          # the left half of the low sky holds nothing
    plain = call(c, low_count=c["low_count"], albedo=c["albedo"], flags=0)
    r = call(c, low_count=c["low_count"], albedo=c["albedo"], flags=SKY_FROM_ALBEDO)
    sky = r["sky"]
    take = sky & r["result"]
    assert take.any() and (sky & ~r["result"]).any()
    assert (r["color"][take][:, :3] == c["albedo"][take][:, :3]).all()
    assert r["color"][take][:, 3].tobytes() == plain["color"][take][:, 3].tobytes()          # alpha stays
    assert (r["color"][sky & ~r["result"]] == 0).all()
    assert r["color"][~sky].tobytes() == plain["color"][~sky].tobytes()
    assert r["count"].tobytes() == plain["count"].tobytes()
    # the flag without an image changes nothing
    assert call(c, low_count=c["low_count"], flags=SKY_FROM_ALBEDO)["color"].tobytes() == plain["color"].tobytes()


def test_synthetic_guides_cover_every_kind_on_both_grids():
    for size in ((13, 9), (37, 33)):
        hit, normal, ids, _ = synthetic_guides(*size, seed=0)
        assert set(np.unique(normal[..., 3]).tolist()) == {0.0, 1.0, 2.0, 3.0}
        assert len(np.unique(ids.view(np.int32)[..., 0])) >= 4
