"""GPU: which lane computes which pixel of which frame, in all six kernel modes, at frame shapes down to one pixel — below one tile,
fewer tiles than work-counter shards or than one run, partial dispatches, strip sets with ragged last strips and ranks that own
nothing, and the hand-out options (work_shards, xcd_run, tile_order, frame_group, frames_per_launch, sched_block, block_threads) at
1, 6 and 18 tiles.  The arithmetic of the kernels is held to the oracle elsewhere (tests/test_gpu_parity.py); here the oracle is
the witness of the index arithmetic (csrc/frame_batch.cpp do_dispatch, csrc/frame_device.h, csrc/front_device.h launch_tiles):

  - the image is bit-equal to the oracle's, alpha included: a pixel nobody computed keeps the alpha 0 of creation;
  - the nine device counters are equal to the oracle's: a pixel computed twice shows in them (`pixels` is accumulated on the host
    and is not looked at);
  - watchdog_trips == 0.

The reference is the scalar oracle with the product's triangle BVH, mode 1, computed once per (size, frame count).  Part e ties
tests/workmap_ref.py (the CPU restatement of the same arithmetic) to the device."""
import contextlib
import functools
import itertools

import numpy as np
import pytest

import workmap_ref as wm
from oracle import pyoracle
from test_gpu_options import DEFAULTS
from unityraytracer_amd import RayTraceMaster, debug_build_blas, scenes, strips

pytestmark = pytest.mark.gpu

NINE = ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky")
MODES = [0, 1, 2, 3, 4, 5]


# ---- the reference -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(w, h):
    return scenes.mixed_test_scene(w, h)


def new_oracle(w, h):
    sc = scene(w, h)
    o = pyoracle.Oracle(sc)
    nodes, tri, root, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
    o.set_blas(nodes, tri, root)
    return o


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_frames(w, h, n):
    """((image, counters) of frame 0 .. n - 1 of RayTraceMaster's protocol), computed once"""
    o, sc, out = new_oracle(w, h), scene(w, h), []
    for f in range(n):
        ox, oy, seed = scenes.frame_uniforms(f) if f else (sc.pixel_offset[0], sc.pixel_offset[1], sc.seed)     # RayTraceMaster.SetShaderParameters
        o.set_frame((ox, oy), seed)
        img, c = o.render(mode=1, threads=8, counters=True)
        out.append((frozen(img), c))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ref_rect(w, h, rw, rh):
    """frame 0 inside [0, rw) x [0, rh): (image of the rect, counters of the rect)"""
    img, c = new_oracle(w, h).render(rect=(0, 0, rw, rh), mode=1, threads=8, counters=True)
    return frozen(img), c


@functools.lru_cache(maxsize=None)
def ref_mean(w, h, n, rank=0, world=1):
    """(running mean after n frames, last frame, the frames' counters summed) of the rows `rank` of `world` owns; other rows: the zeros
    of creation, blended like every pixel (AdditionShader's alpha does not depend on the source)"""
    own = own_rows(h, rank, world)
    conv = np.zeros((h, w, 4), np.float32)
    total = dict.fromkeys(NINE, 0)
    last = None
    o, sc = new_oracle(w, h), scene(w, h)
    for f, (img, c) in enumerate(ref_frames(w, h, n)):
        last = np.where(own[:, None, None], img, np.float32(0))
        conv = pyoracle.accumulate(last, conv, f)
        if world > 1:                                              # the counters of the rank's strips alone
            o.set_frame(scenes.frame_uniforms(f)[:2] if f else sc.pixel_offset, scenes.frame_uniforms(f)[2] if f else sc.seed)
            c = dict.fromkeys(NINE, 0)
            for y0, y1 in strips.strip_row_ranges(h, rank, world):
                part, cs = o.render(rect=(0, y0, w, y1), mode=1, threads=8, counters=True)
                assert same_bits(part, img[y0:y1])                 # (a rect of the oracle is that rect of its frame)
                for k in NINE:
                    c[k] += cs[k]
        for k in NINE:
            total[k] += c[k]
    return frozen(conv), frozen(last), total


def own_rows(h, rank, world):
    own = np.zeros(h, bool)
    for y0, y1 in strips.strip_row_ranges(h, rank, world):
        own[y0:y1] = True
    return own


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_image(got, ref, what):
    if not same_bits(got, ref):
        bad = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2))
        unwritten = int(((got[..., 3] == 0) & (ref[..., 3] != 0)).sum())
        raise AssertionError(f"{what}: {len(bad)} pixels differ ({unwritten} of them never written), first (y, x) {bad[:4].tolist()}")


def assert_counters(gc, oc, what):
    diff = {k: (gc[k], oc[k]) for k in NINE if gc[k] != oc[k]}
    assert not diff, f"{what}: device counters (got, oracle) {diff}"
    assert gc["watchdog_trips"] == 0, what


@contextlib.contextmanager
def options(ctx, **kv):
    try:
        for k, v in kv.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kv:
            ctx.set_option(k, DEFAULTS[k])


@pytest.fixture(autouse=True)
def counting(gpu_ctx):
    try:
        gpu_ctx.set_option("count_stats", 1)
        yield
    finally:
        gpu_ctx.set_option("count_stats", DEFAULTS["count_stats"])
        gpu_ctx.set_option("kernel_mode", DEFAULTS["kernel_mode"])


def render(ctx, sc, mode, frames=1, rank=0, world=1):
    ctx.set_option("kernel_mode", mode)
    ctx.reset_counters()
    m = RayTraceMaster(ctx, sc, rank=rank, world_size=world)
    try:
        for _ in range(frames):
            m.OnRenderImage()                                      # (raises unless every call returned URT_OK)
        return m._target.GetPixels(), m._converged.GetPixels(), ctx.counters()
    finally:
        m.OnDisable()


def dispatch_once(ctx, sc, mode, gx, gy, first=None, stride=None):
    """one Dispatch / DispatchRows of (gx, gy, 1) groups into a fresh Result: its pixels and the counters"""
    ctx.set_option("kernel_mode", mode)
    ctx.reset_counters()
    m = RayTraceMaster(ctx, sc)
    try:
        m._bind_for_queries()                                      # RebuildTrees + SetShaderParameters
        m.InitRenderTexture()
        m.RayTraceShader.SetTexture(0, "Result", m._target)
        if first is None:
            m.RayTraceShader.Dispatch(0, gx, gy, 1)
        else:
            m.RayTraceShader.DispatchRows(0, gx, gy, 1, first, stride)
        return m._target.GetPixels(), ctx.counters()
    finally:
        m.OnDisable()


# ---- a. shapes x modes ---------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 1), (1, 9), (8, 8), (9, 8), (8, 9), (63, 7), (65, 9), (17, 33)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_frame_at_tiny_and_ragged_sizes(gpu_ctx, size, mode):
    w, h = size
    (ref, oc), = ref_frames(w, h, 1)
    got, _, gc = render(gpu_ctx, scene(w, h), mode)
    assert_image(got, ref, f"{w}x{h} mode {mode}")
    assert_counters(gc, oc, f"{w}x{h} mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(8, 9), (65, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_frames_accumulated(gpu_ctx, size, mode):
    w, h = size
    conv_ref, last_ref, oc = ref_mean(w, h, 3)
    last, conv, gc = render(gpu_ctx, scene(w, h), mode, frames=3)
    assert_image(conv, conv_ref, f"{w}x{h} mode {mode}: _converged after 3 frames")
    assert_image(last, last_ref, f"{w}x{h} mode {mode}: _target of frame 2")
    assert_counters(gc, oc, f"{w}x{h} mode {mode}, 3 frames")


# ---- b. partial dispatches x modes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("groups", [(1, 1), (3, 2), (8, 4), (9, 5), (1000, 1000)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_partial_dispatch_writes_its_region_only(gpu_ctx, groups, mode):
    w, h = 65, 33
    gx, gy = groups
    rw, rh = min(gx * 8, w), min(gy * 8, h)
    ref, oc = ref_rect(w, h, rw, rh)
    got, gc = dispatch_once(gpu_ctx, scene(w, h), mode, gx, gy)
    full = np.zeros((h, w, 4), np.float32)                         # every other pixel keeps the zeros of creation
    full[:rh, :rw] = ref
    assert_image(got, full, f"Dispatch(0, {gx}, {gy}, 1) mode {mode}")
    assert_counters(gc, oc, f"Dispatch(0, {gx}, {gy}, 1) mode {mode}")


# ---- c. strips x modes ---------------------------------------------------------------------------------------------------------
STRIP_CASES = [(52, 44, world) for world in (1, 2, 3, 5, 6, 8)] + [(9, 7, 2), (9, 7, 3)]     # 52x44: 6 group rows, the last of 4 pixel rows; 9x7: one


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", STRIP_CASES, ids=lambda c: f"{c[0]}x{c[1]}-world{c[2]}")
def test_every_rank_of_a_strip_set(gpu_ctx, case, mode):
    w, h, world = case
    (ref, oc), = ref_frames(w, h, 1)
    union = np.zeros_like(ref)
    total = dict.fromkeys(NINE, 0)
    for rank in range(world):
        part, _, gc = render(gpu_ctx, scene(w, h), mode, rank=rank, world=world)
        own = own_rows(h, rank, world)
        assert not part[~own].view(np.uint32).any(), f"rank {rank} of {world}, mode {mode}: wrote rows it does not own"
        if not own.any():                                          # a rank with no strip: nothing written, nothing traced
            assert all(gc[k] == 0 for k in NINE), (rank, world, mode, {k: gc[k] for k in NINE})
        assert gc["watchdog_trips"] == 0
        union[own] = part[own]
        for k in NINE:
            total[k] += gc[k]
    assert_image(union, ref, f"{w}x{h} union of {world} ranks, mode {mode}")
    total["watchdog_trips"] = 0
    assert_counters(total, oc, f"{w}x{h} sum over {world} ranks, mode {mode}")


# ---- d. hand-out options at few tiles ------------------------------------------------------------------------------------------
FEW_TILES = [(8, 8), (24, 16), (65, 9)]                            # 1 tile; 6 tiles; 18 tiles, ragged both ways
N_PROTOCOL = 7
WORK_SHARDS, XCD_RUN, TILE_ORDER, FRAME_GROUP, SCHED_BLOCK, BLOCK_THREADS = [1, 2, 64], [0, 1, 4, 7, 4096], [0, 1], [1, 3, 64], [64, 256], [64, 128, 256]


def run_protocol(ctx, m, want, what, fpl=None):
    """N_PROTOCOL frames of RayTraceMaster's protocol on `m`, restarted (the first blend of a restarted mean has weight 1: nothing
    of the last run is left); both images, the rays — and the other eight counters — and the launch count"""
    conv_ref, last_ref, oc = want
    m.ResetAccumulation()
    m._frame = 0
    ctx.reset_counters()
    launches = ctx.counters()["launches"]
    for _ in range(N_PROTOCOL):
        m.OnRenderImage()
    conv, last, gc = m._converged.GetPixels(), m._target.GetPixels(), ctx.counters()
    assert_image(conv, conv_ref, f"{what}: _converged")
    assert_image(last, last_ref, f"{what}: last _target")
    assert_counters(gc, oc, what)
    if fpl == 5:
        assert gc["launches"] - launches < N_PROTOCOL, (what, gc["launches"] - launches)
    return gc


def assert_last_launch_is_the_restated_one(ctx, sc, mode, opts, rank, world, what):
    """urt_debug_launch_info of the protocol's last launch against tests/workmap_ref.py's restatement of the host side: do_dispatch's
    parameters; for modes 3 and 5 the launch flush_pending submits (7 frames in launches of 5: the last holds 2, frame_group clamped to
    it, the automatic run length taken with it) or, with one frame per launch, the dispatch that is not deferred (frame_group 1)."""
    info = ctx.launch_info()
    w, h = sc.width, sc.height
    P = wm.do_dispatch(w, h, (w + 7) // 8, (h + 7) // 8, rank, world, dict(opts, kernel_mode=mode), n_meshes=len(sc.mesh_objects))
    if mode in (3, 5):
        limit = wm.batch_limit(P, opts)
        assert limit == opts["frames_per_launch"]
        P = wm.launch_params(P, N_PROTOCOL % limit or limit, batched=limit > 1, options=opts)
    got = {k: info[k] for k in ("kernel_mode", "n_frames", "frame_group", "xcd_run", "tile_order")}
    assert got == {"kernel_mode": mode, "n_frames": P.n_frames, "frame_group": P.frame_group, "xcd_run": P.xcd_run, "tile_order": P.tile_order}, (what, got, P)
    waves = info["block_threads"] // 64
    if mode == 0:
        assert (info["n_blocks"], info["block_threads"]) == (wm.blocks_for_tiles(P), P.block_threads), (what, info)
    elif mode in (2, 3, 5):                                        # (far fewer tiles than resident waves: one workgroup slot per `waves` tiles)
        assert info["block_threads"] == (256 if mode == 5 else opts["sched_block"] if mode == 3 else P.block_threads), (what, info)
        assert info["n_blocks"] == (P.tiles_x * P.n_strips * P.n_frames + waves - 1) // waves, (what, info)


def sweep(ctx, sc, mode, want, names, lists, fixed=None, rank=0, world=1):
    ctx.set_option("kernel_mode", mode)
    fixed = fixed or {}
    m = RayTraceMaster(ctx, sc, rank=rank, world_size=world)
    n = 0
    try:
        for k, v in fixed.items():
            ctx.set_option(k, v)
        for combo in itertools.product(*lists):
            for k, v in zip(names, combo):
                ctx.set_option(k, v)
            opts = dict(fixed, **dict(zip(names, combo)))
            what = f"{sc.width}x{sc.height} mode {mode} rank {rank} of {world} {opts}"
            run_protocol(ctx, m, want, what, fixed.get("frames_per_launch"))
            assert_last_launch_is_the_restated_one(ctx, sc, mode, opts, rank, world, what)
            n += 1
    finally:
        for k in list(names) + list(fixed):
            ctx.set_option(k, DEFAULTS[k])
        m.OnDisable()
    return n


@pytest.mark.parametrize("fpl", [1, 5])
@pytest.mark.parametrize("mode", [3, 5])
@pytest.mark.parametrize("size", FEW_TILES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batched_hand_out_options_at_few_tiles(gpu_ctx, size, mode, fpl):
    w, h = size
    n = sweep(gpu_ctx, scene(w, h), mode, ref_mean(w, h, N_PROTOCOL), ("work_shards", "xcd_run", "tile_order", "frame_group", "sched_block"),
              (WORK_SHARDS, XCD_RUN, TILE_ORDER, FRAME_GROUP, SCHED_BLOCK), {"frames_per_launch": fpl})
    assert n == 180


@pytest.mark.parametrize("mode", [2, 4])
@pytest.mark.parametrize("size", FEW_TILES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_frame_hand_out_options_at_few_tiles(gpu_ctx, size, mode):
    w, h = size
    n = sweep(gpu_ctx, scene(w, h), mode, ref_mean(w, h, N_PROTOCOL), ("work_shards", "xcd_run", "tile_order", "block_threads"),
              (WORK_SHARDS, XCD_RUN, TILE_ORDER, BLOCK_THREADS))
    assert n == 90


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("size", FEW_TILES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_block_permutation_at_few_tiles(gpu_ctx, size, mode):
    w, h = size
    n = sweep(gpu_ctx, scene(w, h), mode, ref_mean(w, h, N_PROTOCOL), ("xcd_run", "block_threads"), ([0, 1, 4, 7], BLOCK_THREADS))
    assert n == 12


def test_batched_hand_out_options_on_one_strip_set(gpu_ctx):
    """world 3, rank 1 at 65x33 (5 group rows: strips 1 and 4, the last of one pixel row), mode 3, five frames per launch"""
    w, h = 65, 33
    n = sweep(gpu_ctx, scene(w, h), 3, ref_mean(w, h, N_PROTOCOL, rank=1, world=3), ("work_shards", "xcd_run", "tile_order", "frame_group", "sched_block"),
              (WORK_SHARDS, XCD_RUN, TILE_ORDER, FRAME_GROUP, SCHED_BLOCK), {"frames_per_launch": 5}, rank=1, world=3)
    assert n == 180


# ---- e. restatement <-> device -------------------------------------------------------------------------------------------------
# (what, width, height, groups_x, groups_y, first_row, row_stride, options) — chosen with the maps of tests/workmap_ref.py:
#   - 52x44, group rows 2, 6, ... of 6: one strip of 7 tiles, this rank's second cycle of strips is empty; dealt to 2 shards in runs of 4, the
#     second shard's run is one tile short; mode 0: 4 blocks of 2 waves padded to a window of 32, top strip first in mode 3
#   - 65x33, Dispatch(0, 3, 2, 1): 6 of the 45 tiles
#   - 65x9: 18 tiles in runs of 7 over 2 shards — one full cycle of 14, then a last run of 4 for shard 0 and none for shard 1; mode 0: 9 blocks
#     of 2 waves in a window of 56
WORKMAP_CASES = [
    ("strip set with an empty last cycle", 52, 44, 7, 6, 2, 4, {"work_shards": 2, "xcd_run": 4, "block_threads": 128, "tile_order": 1}),
    ("partial region", 65, 33, 3, 2, None, None, {"work_shards": 4, "xcd_run": 1, "block_threads": 256, "tile_order": 0}),
    ("ragged last run", 65, 9, 9, 2, None, None, {"work_shards": 2, "xcd_run": 7, "block_threads": 128, "tile_order": 0}),
]


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("case", WORKMAP_CASES, ids=lambda c: c[0].replace(" ", "-"))
def test_restated_map_is_the_set_the_device_writes(gpu_ctx, case, mode):
    what, w, h, gx, gy, first, stride, opts = case
    P = wm.do_dispatch(w, h, gx, gy, first or 0, stride or 1, dict(opts, kernel_mode=mode), n_meshes=len(scene(w, h).mesh_objects))
    if mode == 0:
        xy = wm.direct(P)
    else:
        xy = wm.persistent(wm.launch_params(P, 1, batched=False, options=opts), 1)[:, 1:]      # frames_per_launch 1: traced at once, frame_group 1
    restated = np.zeros((h, w), np.int32)
    np.add.at(restated, (xy[:, 1], xy[:, 0]), 1)
    assert restated.max() == 1 and restated.sum() > 0, what
    with options(gpu_ctx, frames_per_launch=1, **opts):
        got, gc = dispatch_once(gpu_ctx, scene(w, h), mode, gx, gy, first, stride)
    written = got[..., 3] == 1.0
    assert np.array_equal(written, restated == 1), \
        f"{what}, mode {mode}: {int((written & (restated == 0)).sum())} pixels written outside the restated map, {int((~written & (restated == 1)).sum())} of it not written"
    assert not got[~written].view(np.uint32).any() and gc["watchdog_trips"] == 0
