"""Which lane computes which pixel of which frame: a numpy restatement, function by function, of the index arithmetic the six trace
kernel modes share.  Host side: csrc/context.cpp strip_count, csrc/frame_batch.cpp do_dispatch (region, tiles_x, n_strips),
auto_run_length, batch_limit and flush_pending (which clamps frame_group and recomputes xcd_run for the launch that
launch_sched_frames enqueues), csrc/launch_host.h blocks_for_tiles.  Device side: csrc/frame_device.h tile_pixel, shard_slots,
shard_tile, slot_pixel and wave_fetch_pixels, csrc/front_device.h launch_tiles.  Gather: csrc/kernels.hip k_pack_rows.

Two maps come out of it:

    direct(P)                -> (x, y) of every pixel a launch of modes 0 and 1 computes, one row per lane that passes tile_pixel
    persistent(P, n_frames)  -> (frame, x, y) of every slot the work counters of modes 2 - 5 can hand out that reaches a pixel

Unsigned device arithmetic is carried in int64 and checked to stay below 2^32 (`_u32`): a value that would wrap on the device raises
here and names itself, instead of being restated silently.  tests/test_workmap_ref.py sweeps the maps against the plain definition
of the pixels a dispatch owns; tests/test_gpu_frame_shapes.py ties them to the device.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

K_WORK_SHARDS = 64             # csrc/urt_device.h kWorkShards
K_MAX_FRAMES_PER_LAUNCH = 64   # csrc/urt_device.h kMaxFramesPerLaunch
K_AUTO_FRAMES = 64             # csrc/frame_batch.cpp kAutoFrames

# what a fresh context holds (csrc/context_impl.h urt_context::Options), of the options the hand-out reads
DEFAULT_OPTIONS = {"kernel_mode": 3, "block_threads": 64, "xcd_run": 0, "work_shards": 64, "frame_group": 64, "tile_order": -1,
                   "frames_per_launch": 0}


@dataclass(frozen=True)
class Params:
    """The fields of csrc/urt_device.h FrameParams that decide where a lane works."""
    width: int
    height: int
    region_w: int
    region_h: int
    tiles_x: int
    first_group_row: int
    row_stride: int
    n_strips: int
    block_threads: int
    xcd_run: int
    n_shards: int
    frame_group: int
    tile_order: int
    n_frames: int
    kernel_mode: int


def _u32(a, what: str):
    if isinstance(a, int):
        if not 0 <= a < 2**32:
            raise OverflowError(f"{what} leaves 32 unsigned bits: {a}")
        return a
    a = np.asarray(a, dtype=np.int64)
    if a.size and (a.min() < 0 or a.max() >= 2**32):
        raise OverflowError(f"{what} leaves 32 unsigned bits: [{a.min()}, {a.max()}]")
    return a


# csrc/context.cpp:strip_count
def strip_count(group_rows: int, first_row: int, row_stride: int) -> int:
    return (group_rows - first_row + row_stride - 1) // row_stride if first_row < group_rows else 0


# csrc/frame_batch.cpp:auto_run_length
def auto_run_length(P: Params, n_frames: int) -> int:
    runs = P.tiles_x * P.n_strips * max(1, n_frames) // (max(1, P.n_shards) * 256)
    g = 1
    while g < 8 and 2 * g <= runs:
        g *= 2
    return g


# csrc/frame_batch.cpp:do_dispatch — the part that fills FrameParams.  None: the dispatch launches nothing (and returns URT_OK).
# n_meshes decides the automatic tile_order only.
def do_dispatch(width: int, height: int, gx: int, gy: int, first_row: int = 0, row_stride: int = 1, options=None, n_meshes: int = 1):
    opt = dict(DEFAULT_OPTIONS)
    opt.update(options or {})
    if gx < 0 or gy < 0 or first_row < 0 or row_stride < 1:
        raise ValueError("negative thread-group count or bad strip arguments")
    if gx == 0 or gy == 0:
        return None
    region_w, region_h = min(gx * 8, width), min(gy * 8, height)
    tiles_x = (region_w + 7) // 8
    n_strips = strip_count((region_h + 7) // 8, first_row, row_stride)
    if n_strips == 0 or tiles_x == 0:
        return None
    mode = opt["kernel_mode"]
    P = Params(width=width, height=height, region_w=region_w, region_h=region_h, tiles_x=tiles_x, first_group_row=first_row,
               row_stride=row_stride, n_strips=n_strips, block_threads=64 if mode == 4 else opt["block_threads"], xcd_run=opt["xcd_run"],
               n_shards=opt["work_shards"], frame_group=opt["frame_group"],
               tile_order=opt["tile_order"] if opt["tile_order"] >= 0 else (1 if n_meshes == 0 else 0), n_frames=1, kernel_mode=mode)
    if opt["xcd_run"] <= 0:
        P = replace(P, xcd_run=auto_run_length(P, 1) if mode >= 2 else 1)
    if P.tiles_x * P.n_strips * 64 >= 0xffffffff:
        raise ValueError("Dispatch: too many pixel slots in one dispatch")
    return P


# csrc/frame_batch.cpp:batch_limit — frames one launch may hold, on the library's own stream
def batch_limit(P: Params, options=None) -> int:
    opt = dict(DEFAULT_OPTIONS)
    opt.update(options or {})
    lim = opt["frames_per_launch"]
    if lim == 0:
        frame_bytes = P.width * P.height * 16
        lim = min(K_AUTO_FRAMES, max(1, (8 << 30) // max(1, frame_bytes)))
    slots = max(1, (P.tiles_x * P.n_strips + max(64, opt["xcd_run"])) * 64)
    lim = min(lim, max(1, 0xfffffffe // slots // 2))
    return max(1, min(lim, K_MAX_FRAMES_PER_LAUNCH))


# What launch_sched_frames is handed for a launch of n frames of modes 3 and 5.  n == 1 out of a dispatch that was not deferred
# (csrc/frame_batch.cpp:do_dispatch, limit <= 1): frame_group 1.  A deferred batch (csrc/frame_batch.cpp:flush_pending): frame_group
# clamped to [1, n], the automatic run length taken again with the launch's frame count.
def launch_params(P: Params, n: int, batched: bool, options=None) -> Params:
    opt = dict(DEFAULT_OPTIONS)
    opt.update(options or {})
    if not batched:
        assert n == 1
        return replace(P, n_frames=1, frame_group=1)
    Q = replace(P, n_frames=n, frame_group=max(1, min(P.frame_group, n)))
    if opt["xcd_run"] <= 0:
        Q = replace(Q, xcd_run=auto_run_length(Q, n))
    return Q


# csrc/launch_host.h:blocks_for_tiles
def blocks_for_tiles(P: Params) -> int:
    waves = P.block_threads // 64
    ntiles = P.tiles_x * P.n_strips
    nblocks = (ntiles + waves - 1) // waves
    q = 8 * P.xcd_run
    return ((nblocks + q - 1) // q) * q


# csrc/frame_device.h:tile_pixel — for every (block, wave, lane) of the grid at once; returns x, y, the predicate it returns and
# `tile < ntiles` on its own
def tile_pixel(P: Params, block, wave, lane, block_dim: int):
    b = np.asarray(block, dtype=np.int64)
    G = P.xcd_run
    sb = ((b // (8 * G)) * 8 + (b & 7)) * G + ((b >> 3) % G)
    tile = sb * (block_dim >> 6) + wave
    ntiles = P.tiles_x * P.n_strips
    in_range = tile < ntiles
    ty = tile // P.tiles_x
    tx = tile - ty * P.tiles_x
    x = tx * 8 + (lane & 7)
    y = (P.first_group_row + ty * P.row_stride) * 8 + (lane >> 3)
    return x, y, in_range & (x < P.region_w) & (y < P.region_h), in_range


def direct(P: Params) -> np.ndarray:
    """(n, 2) int64 (x, y): what the grid of modes 0 and 1 computes — blocks_for_tiles blocks of block_threads / 64 waves
    (csrc/kernels_basic.hip launch_mega, launch_wavefront's k_generate), every lane through tile_pixel."""
    nb, waves = blocks_for_tiles(P), P.block_threads // 64
    if nb * P.block_threads >= 2**31:
        raise OverflowError("grid of more than 2^31 threads")
    b, w = np.meshgrid(np.arange(nb, dtype=np.int64), np.arange(waves, dtype=np.int64), indexing="ij")
    some = tile_pixel(P, b, w, 0, P.block_threads)[3]             # waves past the last tile return false in every lane: not expanded
    x, y, ok, _ = tile_pixel(P, b[some][:, None], w[some][:, None], np.arange(64, dtype=np.int64)[None, :], P.block_threads)
    return np.stack([x[ok], y[ok]], axis=1)


# csrc/frame_device.h:shard_slots
def shard_slots(ntiles: int, shard: int, G: int, NS: int) -> int:
    cycle = int(_u32(NS * G, "shard_slots cycle"))
    full = ntiles // cycle
    rem = ntiles - full * cycle
    extra = min(rem - shard * G, G) if rem > shard * G else 0
    return int(_u32((full * G + extra) * 64, "shard_slots"))


# csrc/frame_device.h:shard_tile
def shard_tile(shard, q, G: int, NS: int):
    q = np.asarray(q, dtype=np.int64)
    run = q // G
    return _u32((run * NS + shard) * G + (q - run * G), "shard_tile")


# csrc/frame_device.h:slot_pixel
def slot_pixel(P: Params, tile, l):
    ty = tile // P.tiles_x
    tx = tile - ty * P.tiles_x
    x = tx * 8 + (l & 7)
    y = (P.first_group_row + ty * P.row_stride) * 8 + (l >> 3)
    return x, y, (x < P.region_w) & (y < P.region_h)


# csrc/front_device.h:launch_tiles
def launch_tiles(P: Params):
    tiles_per_frame = int(_u32(P.tiles_x * P.n_strips, "tiles_per_frame"))
    if P.frame_group <= 1:
        return int(_u32(tiles_per_frame * P.n_frames, "launch_tiles")), tiles_per_frame
    groups = (P.n_frames + P.frame_group - 1) // P.frame_group
    runs = (tiles_per_frame + P.xcd_run - 1) // P.xcd_run
    return int(_u32(groups * P.frame_group * runs * P.xcd_run, "launch_tiles")), tiles_per_frame


# csrc/frame_device.h:wave_fetch_pixels, from `local` (a slot of shard `shard` below shard_slots) on: the tile, its frame
# (batched launches: frame-major, or de-interleaved in groups of frame_group), tile_order.  Returns frame, tile and the predicate
# `the slot is not dropped here`; slot_pixel follows.
def slot_tile(P: Params, shard, q, ntiles: int, tiles_per_frame=None):
    G, NS = P.xcd_run, P.n_shards
    tile = shard_tile(shard, q, G, NS)
    frame = np.zeros_like(tile)
    ok = np.ones(tile.shape, dtype=bool)
    if tiles_per_frame is not None:
        FG = P.frame_group
        if FG <= 1:
            frame = tile // tiles_per_frame
            tile = tile - frame * tiles_per_frame
        else:
            rg = tile // G
            w = tile - rg * G
            runs_pf = (tiles_per_frame + G - 1) // G
            group_runs = int(_u32(runs_pf * FG, "group_runs"))
            grp = rg // group_runs
            r = rg - grp * group_runs
            frame = _u32(grp * FG + r % FG, "frame")
            tile = _u32((r // FG) * G + w, "tile of frame")
            ok = (tile < tiles_per_frame) & (frame < P.n_frames)
        ntiles = tiles_per_frame
    if P.tile_order == 1:
        tile = np.where(ok, ntiles - 1 - tile, tile)
    return frame, tile, ok


def persistent(P: Params, n_frames: int = 1) -> np.ndarray:
    """(n, 3) int64 (frame, x, y): every slot of every shard through shard_tile, the frame decode, tile_order and slot_pixel.
    Modes 3 and 5 (csrc/kernels.hip k_sched, csrc/kernels_serve.hip k_serve) take ntiles from launch_tiles; modes 2 and 4
    (csrc/kernels_basic.hip k_persist, csrc/kernels_pool.hip k_pool) hand out tiles_x * n_strips tiles of one frame."""
    if P.kernel_mode in (3, 5):
        assert P.n_frames == n_frames
        ntiles, tpf = launch_tiles(P)
    else:
        assert n_frames == 1
        ntiles, tpf = int(_u32(P.tiles_x * P.n_strips, "ntiles")), None
    own = np.array([shard_slots(ntiles, s, P.xcd_run, P.n_shards) for s in range(P.n_shards)], dtype=np.int64)
    per = own >> 6                                                # slots local < own: local >> 6 = q below, local & 63 = the 64 lanes
    shard = np.repeat(np.arange(P.n_shards, dtype=np.int64), per)
    q = np.arange(per.sum(), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    frame, tile, ok = slot_tile(P, shard, q, ntiles, tpf)
    frame, tile = frame[ok], tile[ok]
    bound = tpf if tpf is not None else ntiles
    if tile.size and (tile.min() < 0 or tile.max() >= bound):
        bad = shard[ok][(tile < 0) | (tile >= bound)][0]
        raise IndexError(f"shard {bad}: tile outside [0, {bound}): [{tile.min()}, {tile.max()}]")
    x, y, inside = slot_pixel(P, tile[:, None], np.arange(64, dtype=np.int64)[None, :])
    f = np.broadcast_to(frame[:, None], x.shape)
    return np.stack([f[inside], x[inside], y[inside]], axis=1)


def owed_tiles(P: Params) -> int:
    """Tiles the shards own between them: must be the launch's ntiles (every slot below it is some shard's)."""
    ntiles = launch_tiles(P)[0] if P.kernel_mode in (3, 5) else P.tiles_x * P.n_strips
    return sum(shard_slots(ntiles, s, P.xcd_run, P.n_shards) for s in range(P.n_shards)) // 64, ntiles


# csrc/frame_device.h:wave_fetch_pixels, the part before `local`: the atomic on the wave's shard, the dry-shard probe and the move to
# the next shard with work.  Waves take turns (any order is a legal schedule); wave i of block b starts at shard b & (NS - 1) and asks
# for want(i, trip) slots per fetch.  Returns, per shard, the `local` values handed to lanes, in the order they were handed out, and
# the number of fetches; raises if a wave is still fetching after `max_fetches`.
def simulate_fetch(ntiles: int, G: int, NS: int, n_blocks: int, waves_per_block: int, want, max_fetches: int = 1_000_000):
    own = [shard_slots(ntiles, s, G, NS) if s < NS else 0 for s in range(K_WORK_SHARDS)]
    nxt = [0] * K_WORK_SHARDS
    handed = [[] for _ in range(K_WORK_SHARDS)]
    waves = [{"shard": b & (NS - 1), "exhausted": False} for b in range(n_blocks) for _ in range(waves_per_block)]
    fetches = 0
    while not all(w["exhausted"] for w in waves):
        for i, w in enumerate(waves):
            if w["exhausted"]:
                continue
            fetches += 1
            if fetches > max_fetches:
                raise RuntimeError("the waves never see every shard dry")
            n = want(i, fetches)
            assert 1 <= n <= 64
            shard = w["shard"]
            base = nxt[shard]
            nxt[shard] = int(_u32(base + n, "work counter"))
            if base + n >= own[shard]:
                avail = [lane for lane in range(64) if lane < NS and nxt[lane] < own[lane] and lane != shard]
                if not avail:
                    w["exhausted"] = True
                else:
                    after = [a for a in avail if a > shard]
                    w["shard"] = (after or avail)[0]
            handed[shard].extend(l for l in range(base, base + n) if l < own[shard])
    return handed, fetches


# csrc/kernels.hip:k_pack_rows (k_pack_rows_rgb indexes alike): dense element i <-> image (row, col); `inside` is its row < height
def pack_rows(width: int, height: int, first_group_row: int, row_stride: int):
    n_strips = strip_count((height + 7) // 8, first_group_row, row_stride)      # csrc/context.cpp pack_impl
    per_strip = width * 8
    i = np.arange(per_strip * n_strips, dtype=np.int64)
    j = i // per_strip if per_strip else i
    r = i - j * per_strip
    row = (first_group_row + j * row_stride) * 8 + (r // width if width else r)
    col = r % width if width else r
    return i, row, col, row < height


def owned_pixels(P: Params, n_frames: int = 1) -> np.ndarray:
    """The plain definition the maps are held to (not a restatement): pixels of the region in the group rows first_group_row,
    first_group_row + row_stride, ..., once per frame; sorted (frame, y, x) keys as key()."""
    rows = np.arange(P.region_h, dtype=np.int64)
    g = rows // 8
    mine = rows[(g >= P.first_group_row) & ((g - P.first_group_row) % P.row_stride == 0)]
    xs = np.arange(P.region_w, dtype=np.int64)
    per_frame = (mine[:, None] * P.width + xs[None, :]).reshape(-1)
    f = np.arange(n_frames, dtype=np.int64)
    return (f[:, None] * (P.width * P.height) + per_frame[None, :]).reshape(-1)


def key(P: Params, frame, x, y) -> np.ndarray:
    return (np.asarray(frame, dtype=np.int64) * P.height + y) * P.width + x
