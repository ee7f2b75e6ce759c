"""CPU: the restated tile hand-out (tests/workmap_ref.py) against the plain definition of what a dispatch owns — the pixels of the
region that lie in the group rows first_row, first_row + row_stride, ..., once per frame.  For every combination the multiset the
map hands out must equal that set: nothing twice, nothing missing, nothing outside (so x < width and y < height hold too).

Two sweeps, since the full product of every shape with every option is out of reach:
  shapes   every width x height x region x strip set, each under ONE option combination per map, taken in rotation from the full
           option lists (so every option value meets hundreds of shapes);
  options  the full product of the options at a handful of shapes: one tile, a few tiles, ragged both ways, a partial region, strip
           sets with an empty last cycle and with first_row in the last group row.
  strips   every first_row 0 - 9 x row_stride 1 - 9 at every height and three widths, options in rotation as in `shapes`.
SWEPT counts the combinations and the tests assert the totals, so a sweep that shrinks shows:
  shapes   18 widths x 13 heights x 3 regions x 14 strip sets = 9,828 dispatches, of which 3,564 launch; x 3 maps = 10,692
  strips   3 widths x 13 heights x 90 strip sets = 3,510 dispatches, of which 1,539 launch; x 3 maps = 4,617
  options  8 shapes x (24 direct + 112 one-frame persistent + 3,360 batched) = 27,968
"""
import itertools
from dataclasses import replace

import numpy as np
import pytest

import workmap_ref as wm
from unityraytracer_amd import strips

WIDTHS = sorted(set(range(1, 71, 6)) | {1, 7, 8, 9, 63, 64, 65, 70})
HEIGHTS = sorted(set(range(1, 51, 7)) | {1, 7, 8, 9, 63, 64, 65, 50})
STRIPS = [(0, 1), (1, 1), (0, 2), (1, 2), (2, 3), (0, 9), (9, 1), (5, 5), (3, 8), (7, 2), (9, 9), (4, 3), (6, 7), (8, 4)]   # (first_row, row_stride)
BLOCK_THREADS = [64, 128, 256]
XCD_RUN = [0, 1, 3, 4, 7, 8, 64, 4096]                             # 0 = auto
SHARDS = [1, 2, 4, 8, 16, 32, 64]
FRAME_GROUP = [1, 2, 3, 5, 64]
FRAMES = [1, 2, 5, 7, 11, 64]
TILE_ORDER = [0, 1]

SWEPT = {"shapes": 0, "shapes_dispatches": 0, "strips": 0, "strips_dispatches": 0, "options": 0}


def regions(w, h):
    """full, one group, and about half the groups each way (groups_x * 8 < w when w > 8)"""
    gx, gy = (w + 7) // 8, (h + 7) // 8
    return [(gx, gy), (1, 1), (max(1, gx // 2), max(1, (gy + 1) // 2))]


def check(P, got_keys, n_frames, what):
    size = n_frames * P.width * P.height
    assert got_keys.size == 0 or (got_keys.min() >= 0 and got_keys.max() < size), (what, P, "a key outside the frames")
    got = np.bincount(got_keys, minlength=size)                    # how often each (frame, y, x) was handed out
    want = np.zeros(size, dtype=got.dtype)
    want[wm.owned_pixels(P, n_frames)] = 1
    if not np.array_equal(got, want):
        raise AssertionError(f"{what}: {P}: {int((got > 1).sum())} handed out more than once, {int(((got == 0) & (want == 1)).sum())} missing, "
                             f"{int(((got > 0) & (want == 0)).sum())} outside; first differing key {np.flatnonzero(got != want)[:1]}")


def check_direct(P, what="direct"):
    xy = wm.direct(P)
    assert xy.size == 0 or (xy[:, 0].max() < P.width and xy[:, 1].max() < P.height and xy.min() >= 0), (what, P)
    check(P, wm.key(P, 0, xy[:, 0], xy[:, 1]), 1, what)


def check_persistent(P, n, what="persistent"):
    owed, ntiles = wm.owed_tiles(P)
    assert owed == ntiles, (what, P, owed, ntiles)                # the shards own every tile of the launch between them, and no more
    fxy = wm.persistent(P, n)
    assert fxy.size == 0 or (fxy[:, 1].max() < P.width and fxy[:, 2].max() < P.height and fxy.min() >= 0 and fxy[:, 0].max() < n), (what, P)
    check(P, wm.key(P, fxy[:, 0], fxy[:, 1], fxy[:, 2]), n, what)


def batched(P, n, opts):
    """the launch of n frames of modes 3 / 5: deferred (flush_pending) unless it is one frame of a dispatch that was not"""
    return wm.launch_params(P, n, batched=True, options=opts)


def rotating_options():
    return (itertools.cycle(itertools.product(BLOCK_THREADS, XCD_RUN)),
            itertools.cycle(itertools.product((2, 4), XCD_RUN, SHARDS, TILE_ORDER)),
            itertools.cycle(itertools.product((3, 5), XCD_RUN, SHARDS, FRAME_GROUP, FRAMES[:5], TILE_ORDER)))   # (64 frames: the options sweep)


def check_dispatch(w, h, gx, gy, first, stride, rotation, sweep):
    """one dispatch under the next option combination of each map; counts it"""
    direct_opts, one_opts, many_opts = rotation
    SWEPT[sweep + "_dispatches"] += 1
    group_rows = (min(gy * 8, h) + 7) // 8
    bt, run = next(direct_opts)
    P = wm.do_dispatch(w, h, gx, gy, first, stride, {"kernel_mode": 0, "block_threads": bt, "xcd_run": run})
    if first >= group_rows:                                        # a rank without a strip: nothing is launched, in any mode
        assert P is None and wm.do_dispatch(w, h, gx, gy, first, stride, {"kernel_mode": 3}) is None
        return
    assert P.n_strips == len(range(first, group_rows, stride)) and P.tiles_x * 8 >= P.region_w > (P.tiles_x - 1) * 8
    check_direct(P)
    mode, run, ns, order = next(one_opts)
    check_persistent(wm.do_dispatch(w, h, gx, gy, first, stride, {"kernel_mode": mode, "xcd_run": run, "work_shards": ns, "tile_order": order}), 1)
    mode, run, ns, fg, n, order = next(many_opts)
    opts = {"kernel_mode": mode, "xcd_run": run, "work_shards": ns, "frame_group": fg, "tile_order": order}
    check_persistent(batched(wm.do_dispatch(w, h, gx, gy, first, stride, opts), n, opts), n)
    SWEPT[sweep] += 3


def test_shapes_under_rotating_options():
    rotation = rotating_options()
    for w, h in itertools.product(WIDTHS, HEIGHTS):
        for (gx, gy), (first, stride) in itertools.product(regions(w, h), STRIPS):
            check_dispatch(w, h, gx, gy, first, stride, rotation, "shapes")
    assert (SWEPT["shapes_dispatches"], SWEPT["shapes"]) == (9828, 10692), SWEPT


def test_every_strip_set_under_rotating_options():
    rotation = rotating_options()
    for w, h in itertools.product((1, 9, 65), HEIGHTS):
        for first, stride in itertools.product(range(10), range(1, 10)):
            check_dispatch(w, h, (w + 7) // 8, (h + 7) // 8, first, stride, rotation, "strips")
    assert (SWEPT["strips_dispatches"], SWEPT["strips"]) == (3510, 4617), SWEPT


# (width, height, groups_x, groups_y, first_row, row_stride)
OPTION_SHAPES = [(8, 8, 1, 1, 0, 1), (24, 16, 3, 2, 0, 1), (65, 9, 9, 2, 0, 1), (70, 50, 9, 7, 0, 1), (65, 33, 3, 2, 0, 1),
                 (65, 33, 9, 5, 1, 3), (52, 44, 7, 6, 5, 6), (52, 44, 7, 6, 1, 2)]


@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_option_product(shape):
    w, h, gx, gy, first, stride = shape
    n = 0
    for bt, run in itertools.product(BLOCK_THREADS, XCD_RUN):
        check_direct(wm.do_dispatch(w, h, gx, gy, first, stride, {"kernel_mode": 0, "block_threads": bt, "xcd_run": run}))
        n += 1
    for run, ns, order in itertools.product(XCD_RUN, SHARDS, TILE_ORDER):
        check_persistent(wm.do_dispatch(w, h, gx, gy, first, stride, {"kernel_mode": 2, "xcd_run": run, "work_shards": ns, "tile_order": order}), 1)
        n += 1
    for run, ns, fg, frames, order in itertools.product(XCD_RUN, SHARDS, FRAME_GROUP, FRAMES, TILE_ORDER):
        opts = {"kernel_mode": 3, "xcd_run": run, "work_shards": ns, "frame_group": fg, "tile_order": order}
        P = wm.do_dispatch(w, h, gx, gy, first, stride, opts)
        check_persistent(batched(P, frames, opts), frames)
        if frames == 1:                                            # and the dispatch that is not deferred
            check_persistent(wm.launch_params(P, 1, batched=False, options=opts), 1)
        n += 1
    assert n == 24 + 112 + 3360, n
    SWEPT["options"] += n


def test_checker_notices_a_lost_strip_offset_and_a_lost_frame():
    """the comparison itself: a map made from parameters that differ from the dispatch's in one field is refused"""
    P = wm.do_dispatch(52, 44, 7, 6, 1, 2, {"kernel_mode": 3, "frame_group": 3, "xcd_run": 4})
    Q = replace(P, first_group_row=0)
    xy = wm.direct(Q)
    with pytest.raises(AssertionError):
        check(P, wm.key(P, 0, xy[:, 0], xy[:, 1]), 1, "direct without first_group_row")
    B = batched(P, 5, {"xcd_run": 4})
    fxy = wm.persistent(B, 5)
    check(B, wm.key(B, fxy[:, 0], fxy[:, 1], fxy[:, 2]), 5, "unchanged")
    with pytest.raises(AssertionError):
        check(B, wm.key(B, fxy[:-1, 0], fxy[:-1, 1], fxy[:-1, 2]), 5, "one slot short")


def test_host_side_restatements_agree_with_the_package():
    for h, world in itertools.product(range(1, 70), range(1, 10)):
        for rank in range(world + 2):
            assert wm.strip_count((h + 7) // 8, rank, world) == strips.n_strips(h, rank, world) == len(strips.strip_row_ranges(h, rank, world))
    # auto_run_length: 1 until every shard has 512 runs, then doubling up to 8
    P = wm.do_dispatch(1920, 1080, 240, 135, options={"kernel_mode": 3})
    assert P.xcd_run == 1 and [wm.launch_params(P, n, True).xcd_run for n in (1, 2, 4, 8, 64)] == [1, 2, 4, 8, 8]
    assert [wm.launch_params(P, n, True).frame_group for n in (1, 2, 5, 64)] == [1, 2, 5, 64]
    assert wm.batch_limit(P) == 64 and wm.batch_limit(P, {"frames_per_launch": 5}) == 5
    assert wm.batch_limit(wm.do_dispatch(32768, 32768, 4096, 4096, options={"kernel_mode": 3})) == 1   # 8 GiB of Result slots, 16 GiB per frame


@pytest.mark.parametrize("w,h,world", [(52, 44, 1), (52, 44, 3), (52, 44, 8), (9, 7, 3), (65, 33, 5), (1, 9, 2), (7, 1, 1)])
def test_pack_rows_restated_equals_the_host_pack(w, h, world):
    rng = np.random.default_rng(w * 100 + h)
    img = rng.random((h, w, 4), dtype=np.float32)
    seen = np.zeros((h, w), np.int32)
    for rank in range(world):
        i, row, col, inside = wm.pack_rows(w, h, rank, world)
        dense = np.zeros((i.size, 4), np.float32)
        assert ((col >= 0) & (col < w)).all() and (row[inside] < h).all() and (row >= 0).all()
        dense[i[inside]] = img[row[inside], col[inside]]           # to_dense; rows past the image stay zero
        n0 = strips.n_strips(h, rank, world)
        assert i.size == n0 * 8 * w
        want = strips.pack_rows_host(img, rank, world)[: n0 * 8]   # (the host pack pads to rank 0's strip count; the kernel packs its own)
        assert np.array_equal(dense.reshape(-1, w, 4), want), (rank, world)
        np.add.at(seen, (row[inside], col[inside]), 1)
    assert (seen == 1).all()                                       # the ranks' strips tile the image


def test_shard_moves_hand_out_every_slot_once_and_end():
    """wave_fetch_pixels up to `local`: whatever the grid and however many slots a wave asks for per fetch, every slot below a shard's
    count is handed out exactly once, slots at or above it to nobody, and every wave sees all shards dry after finitely many fetches."""
    wants = [lambda i, t: 64, lambda i, t: 1, lambda i, t: 1 + (i * 7 + t * 13) % 64]
    n = 0
    for ntiles, G, NS, (blocks, waves) in itertools.product([1, 6, 18, 65, 127], [1, 4, 7, 4096], [1, 2, 64], [(1, 1), (3, 4), (64, 1), (70, 4)]):
        for want in wants:
            handed, _ = wm.simulate_fetch(ntiles, G, NS, blocks, waves, want)
            for s in range(64):
                own = wm.shard_slots(ntiles, s, G, NS) if s < NS else 0
                assert sorted(handed[s]) == list(range(own)), (ntiles, G, NS, blocks, waves, s)
            n += 1
    assert n == 720
