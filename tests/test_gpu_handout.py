"""GPU: option "handout" of the scheduled trace kernel (csrc/kernels.hip k_sched, csrc/frame_device.h wg_fetch_pixels).  With it on
(the default) the four waves of a workgroup share a reservation of tiles in LDS and only the wave that drains it adds to the work
counter of the workgroup's shard; with it off every refill of every wave does (wave_fetch_pixels).  Only the ORDER in which pixels are
picked up may change, so at every case below, kernel mode 3:
    handout 1 == handout 0 == handout -1 == the oracle, bit for bit, the last traced frame and the accumulated image,
the launch reports the reservation it ran with (launch_info "handout": the largest divisor of the run length that is <= 16, or 0), and
the watchdog counter stays 0.  Cases: frame shapes from one pixel to 96 x 64, frames with fewer tiles than work-counter shards, with
exactly one run and with one run plus one tile; launches of 1, 2, 4 and 64 frames with the frames interleaved or not; run lengths 1, 2,
8, 24 (reservations of 12 tiles: two per run) and 4096 (longer than the launch); top-down tile order; both ranks of a two-rank strip
split; the scenes and extreme vote thresholds of tests/test_gpu_front_fuse.py (refills of 1 and of 64 lanes), the masked object-level
phase, three rays per pixel, one bounce.  With count_stats the counters equal the oracle's, `rays` included."""

import numpy as np
import pytest

from oracle import pyoracle
from test_gpu_front_fuse import HIGH, LOW, blobs, case, differing, same
from unityraytracer_amd import RayTraceMaster, UrtError, scenes, strips

pytestmark = pytest.mark.gpu

RESTORE = {"handout": -1, "count_stats": 0, "kernel_mode": 3, "front_list": -1, "top_front": -1, "refill_min": 16, "blas_min": 0, "blas_exit": 0,
           "shade_min": 32, "waves_per_cu": 0, "xcd_run": 0, "frame_group": 64, "frames_per_launch": 0, "tile_order": -1, "work_shards": 64}
NINE = ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky")

_scenes = {}


def scene(name):
    """Scenes by name, built once: "WxH" = the reduced C3 blob at that size, else a case of tests/test_gpu_front_fuse.py, or the two
    blobs with the object-level phase left to auto ("two-masked": the masked form)."""
    if name not in _scenes:
        if name == "two-masked":
            _scenes[name] = (blobs(96, 64, [(-2.0, -4.0, 1.6), (2.2, -2.5, 1.4)]), {}, 3)
        elif "x" in name and name.replace("x", "").isdigit():
            w, h = (int(v) for v in name.split("x"))
            _scenes[name] = (scenes.config3(w, h, slices=24, stacks=20, sky=scenes.make_sky(64, 32)), {}, 0)
        else:
            _scenes[name] = case(name)
    return _scenes[name]


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_option(k, v)


def frames_of(ctx, sc, frames, handout, rank=0, world=1):
    ctx.set_option("handout", handout)
    ctx.reset_counters()
    m = RayTraceMaster(ctx, sc, rank=rank, world_size=world)
    try:
        for _ in range(frames):
            m.OnRenderImage()
        t, c = m._target.GetPixels(), m._converged.GetPixels()
        info = ctx.launch_info()
        tree = ctx.read_scene_blas(len(sc.mesh_objects))[:3]
        return t, c, info, tree, ctx.counters()
    finally:
        m.OnDisable()


_oracle = {}


def oracle_frames(name, sc, tree, frames, rank=0, world=1):
    """(last traced frame, accumulated image) of `frames` frames of RayTraceMaster's protocol on the rows `rank` of `world` owns (the other
    rows keep the zeros of creation and are blended like every pixel); the frames of a scene are rendered once and shared."""
    per_scene = _oracle.setdefault(name, [])
    if len(per_scene) < frames:
        o = pyoracle.Oracle(sc)
        o.set_blas(*tree)
        for f in range(len(per_scene), frames):
            ox, oy, sd = scenes.frame_uniforms(f)
            o.set_frame((ox, oy), sd)
            img = o.render(mode=1, threads=8)
            img.setflags(write=False)
            per_scene.append(img)
    own = np.zeros(sc.height, bool)
    for y0, y1 in strips.strip_row_ranges(sc.height, rank, world):
        own[y0:y1] = True
    acc, last = np.zeros((sc.height, sc.width, 4), np.float32), None
    for f in range(frames):
        last = np.where(own[:, None, None], per_scene[f], np.float32(0))
        acc = pyoracle.accumulate(last, acc, f)
    return last, acc


def expected_handout(run):
    c = min(run, 16)
    while run % c:
        c -= 1
    return c


def check(ctx, name, frames=4, opts=None, rank=0, world=1, n_frames=None):
    sc, scene_opts, front = scene(name)
    what = f"{name} x{frames} {opts or {}} rank {rank}/{world}"
    try:
        for k, v in {**scene_opts, **(opts or {})}.items():
            ctx.set_option(k, v)
        t0, c0, i0, tree, g0 = frames_of(ctx, sc, frames, 0, rank, world)
        t1, c1, i1, _, g1 = frames_of(ctx, sc, frames, 1, rank, world)
        ta, ca, ia, _, ga = frames_of(ctx, sc, frames, -1, rank, world)
        for i in (i0, i1, ia):
            assert i["kernel_mode"] == 3 and i["front_mode"] == front and i["kernel"].startswith("k_sched<false, "), (what, i)
            assert i["n_frames"] == (n_frames if n_frames is not None else frames), (what, i)
        assert i0["handout"] == 0 and i1["handout"] == ia["handout"] == expected_handout(i1["xcd_run"]), (what, i0, i1, ia)
        assert i0["xcd_run"] == i1["xcd_run"] and i0["frame_group"] == i1["frame_group"] and i0["lds_bytes"] == i1["lds_bytes"], (what, i0, i1)
        img, acc = oracle_frames(name, sc, tree, frames, rank, world)
        assert same(t1, t0) and same(c1, c0), f"{what}: handout 1 differs from 0 in {differing(t1, t0)} / {differing(c1, c0)} pixels"
        assert same(ta, t1) and same(ca, c1), f"{what}: handout -1 differs from 1 in {differing(ta, t1)} / {differing(ca, c1)} pixels"
        assert same(t1, img) and same(c1, acc), f"{what}: handout 1 differs from the oracle in {differing(t1, img)} / {differing(c1, acc)} pixels"
        for g in (g0, g1, ga):
            assert g["watchdog_trips"] == 0, what
        assert g1["rays"] == g0["rays"], (what, g1["rays"], g0["rays"])     # (the plain counter every instantiation keeps)
        return i1
    finally:
        restore(ctx)


# 40 x 24: 15 tiles, fewer than the 64 shards.  64 x 8 with runs of 8: the frame is exactly one run; 72 x 8: one run and one tile.
@pytest.mark.parametrize("name,opts", [("1x1", {}), ("65x3", {}), ("7x130", {}), ("96x64", {}), ("40x24", {}), ("40x24", {"xcd_run": 8}),
                                       ("64x8", {"xcd_run": 8}), ("72x8", {"xcd_run": 8}), ("64x8", {"xcd_run": 8, "frame_group": 1}),
                                       ("72x8", {"xcd_run": 8, "frame_group": 1}), ("72x8", {"xcd_run": 8, "work_shards": 1})])
def test_frame_shapes(gpu_ctx, name, opts):
    check(gpu_ctx, name, 4, opts)


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("frames", [1, 2, 4, 64])
def test_frames_per_launch(gpu_ctx, frames, group):
    """one launch of 1, 2, 4 and 64 frames (frames_per_launch; the 64 are what auto takes), interleaved (frame_group auto = all) or frame after frame"""
    i = check(gpu_ctx, "40x24", frames, {"frame_group": group, "frames_per_launch": frames})
    assert i["frame_group"] == min(group, frames), i


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("run", [1, 2, 8, 24, 4096])
def test_run_lengths(gpu_ctx, run, group):
    """96 x 64 = 96 tiles, four frames per launch: runs of 1, 2, 8 tiles are one reservation each, runs of 24 two of 12, runs of 4096 (longer than the launch) are handed out 16 tiles at a time"""
    i = check(gpu_ctx, "96x64", 4, {"xcd_run": run, "frame_group": group})
    assert i["xcd_run"] == run and i["handout"] == {1: 1, 2: 2, 8: 8, 24: 12, 4096: 16}[run], i


@pytest.mark.parametrize("opts", [{"tile_order": 1}, {"tile_order": 1, "frame_group": 1, "xcd_run": 8}])
def test_top_down_order(gpu_ctx, opts):
    check(gpu_ctx, "96x64", 4, opts)


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("name", ["96x64", "65x3"])
def test_strips_of_a_two_rank_split(gpu_ctx, name, rank):
    if not strips.strip_row_ranges(scene(name)[0].height, rank, 2):
        check_nothing_traced(gpu_ctx, name, rank)
    else:
        check(gpu_ctx, name, 4, {"xcd_run": 2}, rank=rank, world=2)


def check_nothing_traced(ctx, name, rank):
    """a rank without a strip (65 x 3 has one group row): nothing is launched and nothing written, whatever the hand-out"""
    sc = scene(name)[0]
    try:
        for handout in (0, 1):
            t, c, _, _, g = frames_of(ctx, sc, 4, handout, rank, 2)
            assert not t.view(np.uint32).any() and g["rays"] == 0 and g["watchdog_trips"] == 0
    finally:
        restore(ctx)


@pytest.mark.parametrize("name", ["C3-spheres", "two-meshes", "two-masked", "three-rays", "one-bounce", "thresholds-low", "thresholds-high"])
def test_scenes_and_thresholds(gpu_ctx, name):
    check(gpu_ctx, name, 4)


@pytest.mark.parametrize("name,opts", [("thresholds-low", {"xcd_run": 8, "frame_group": 1}), ("thresholds-high", {"xcd_run": 8, "frame_group": 1}),
                                       ("thresholds-low", {"xcd_run": 1}), ("thresholds-high", {"xcd_run": 4096})])
def test_thresholds_across_run_lengths(gpu_ctx, name, opts):
    check(gpu_ctx, name, 4, opts)


@pytest.mark.parametrize("name", ["96x64", "C3-spheres", "two-meshes", "two-masked"])
def test_counters_equal_the_oracles(gpu_ctx, name):
    sc, opts, front = scene(name)
    try:
        for k, v in opts.items():
            gpu_ctx.set_option(k, v)
        gpu_ctx.set_option("count_stats", 1)
        t, _, info, tree, gc = frames_of(gpu_ctx, sc, 1, 1)
        assert info["count_stats"] == 1 and info["front_mode"] == front and info["handout"] > 0 and info["kernel"].startswith("k_sched<true, "), info
        o = pyoracle.Oracle(sc)
        o.set_blas(*tree)
        o.set_frame(scenes.frame_uniforms(0)[:2], scenes.frame_uniforms(0)[2])
        ref, oc = o.render(mode=1, threads=8, counters=True)
        assert same(t, ref)
        for k in NINE:
            assert gc[k] == oc[k], (k, gc[k], oc[k])
        assert gc["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


def test_other_kernel_modes_keep_the_counters(gpu_ctx):
    """kernel modes 2 and 5 draw from the work counters whatever the option says (mode 5 keeps the dword for its own threshold)"""
    sc = scene("96x64")[0]
    try:
        gpu_ctx.set_option("handout", 1)
        for mode in (2, 5):
            gpu_ctx.set_option("kernel_mode", mode)
            m = RayTraceMaster(gpu_ctx, sc)
            m.OnRenderImage()
            t, info = m._target.GetPixels(), gpu_ctx.launch_info()
            tree = gpu_ctx.read_scene_blas(len(sc.mesh_objects))[:3]
            m.OnDisable()
            assert info["kernel_mode"] == mode and info["handout"] == 0, info
            assert same(t, oracle_frames("96x64", sc, tree, 1)[0]), mode
            assert gpu_ctx.counters()["watchdog_trips"] == 0
    finally:
        restore(gpu_ctx)


def test_option_range(gpu_ctx):
    try:
        for bad in (-2, 2):
            with pytest.raises(UrtError):
                gpu_ctx.set_option("handout", bad)
    finally:
        restore(gpu_ctx)
