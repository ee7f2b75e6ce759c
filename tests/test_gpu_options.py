"""GPU (needs a context, renders nothing): urt_set_option accepts exactly the values it accepted before its strcmp chain became a table.
The bounds below are literals copied from that chain, arm by arm — not read from the table; the same file runs unchanged against a
library built from the chain (URT_LIB_PATH)."""
import os

import pytest

from unityraytracer_amd import Context, UrtError

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2**31, 2**31 - 1

# name: (lowest accepted, highest accepted); None = no bound at that end
RANGES = {
    "blas_builder": (-1, 3), "frames_per_launch": (0, 64), "kernel_mode": (0, 5), "block_threads": (64, 256), "blas_leaf_max": (1, 8),
    "blas_min": (0, 256), "blas_exit": (0, 64), "refill_min": (1, 64), "waves_per_cu": (0, 32), "sched_block": (0, 256),
    "stack_pad": (0, 96), "shade_min": (1, 64), "front_list": (-1, 2), "shade_split": (-1, 1), "serve_refill": (1, 64),
    "sky_min": (1, 64), "tile_order": (-1, 1), "top_front": (-1, 1), "top_nodes": (-1, 256), "pool_k": (1, 4), "pool_refill": (1, 256),
    "pool_blas_min": (1, 256), "pool_blas_exit": (1, 64), "pool_other_min": (1, 64), "pool_inloop": (1, 64), "frame_group": (1, 64),
    "work_shards": (1, 64), "qnodes": (-1, 1), "lbvh_slack": (0, 16), "overlap_launches": (0, 2), "front_cull": (0, 1),
    "watchdog_cap": (0, None), "xcd_run": (0, 4096),
    # any value, stored as 0 / 1
    "count_stats": (None, None), "time_dispatch": (None, None), "lds_tlas": (None, None), "refit": (None, None),
}
# values inside the range that the chain refused all the same, and their neighbours it took
HOLES = {"block_threads": ([65, 100, 127, 129, 255], [128]), "sched_block": ([1, 63, 65, 128, 255], [64]),
         "work_shards": ([3, 5, 6, 24, 63], [2, 4, 8, 16, 32])}
# what a fresh context holds (the struct's default member initialisers): set last, so that the context leaves as it came
DEFAULTS = {
    "blas_builder": -1, "frames_per_launch": 0, "kernel_mode": 3, "block_threads": 64, "blas_min": 0, "blas_exit": 0, "refill_min": 16,
    "waves_per_cu": 0, "sched_block": 0, "stack_pad": 0, "shade_min": 32, "front_list": -1, "shade_split": -1, "serve_refill": 16,
    "sky_min": 32, "tile_order": -1, "top_front": -1, "top_nodes": -1, "pool_k": 2, "pool_refill": 32, "pool_blas_min": 48,
    "pool_blas_exit": 8, "pool_other_min": 24, "pool_inloop": 16, "frame_group": 64, "work_shards": 64, "qnodes": 0, "lbvh_slack": 6,
    "overlap_launches": 1, "front_cull": 1, "watchdog_cap": 0, "xcd_run": 0, "count_stats": 0, "time_dispatch": 0, "lds_tlas": 1, "refit": 1,
}


def refused(ctx, name, value):
    with pytest.raises(UrtError) as e:
        ctx.set_option(name, value)
    assert e.value.code == 1, (name, value, str(e.value))           # URT_ERR_INVALID_ARGUMENT
    return str(e.value)


def test_every_option_accepts_exactly_its_range():
    assert len(RANGES) == 37
    env = os.environ.get("URT_BLAS_LEAF_MAX", "")
    leaf_max = int(env) if env.isdigit() and 1 <= int(env) <= 8 else 2   # "blas_leaf_max" is process-wide (csrc/blas_builder.cpp)
    with Context(0) as ctx:
        try:
            for name, (lo, hi) in RANGES.items():
                ctx.set_option(name, INT_MIN if lo is None else lo)     # raises unless URT_OK
                ctx.set_option(name, INT_MAX if hi is None else hi)
                if lo is not None:
                    assert name in refused(ctx, name, lo - 1)
                    refused(ctx, name, INT_MIN)
                if hi is not None:
                    assert name in refused(ctx, name, hi + 1)
                    refused(ctx, name, INT_MAX)
            for name, (bad, good) in HOLES.items():
                for v in bad:
                    assert name in refused(ctx, name, v)
                for v in good:
                    ctx.set_option(name, v)
            msg = refused(ctx, "no_such_option", 1)
            assert "unknown option no_such_option" in msg
            assert set(DEFAULTS) == set(RANGES) - {"blas_leaf_max"}
        finally:
            ctx.set_option("blas_leaf_max", leaf_max)
            for name, v in DEFAULTS.items():
                ctx.set_option(name, v)
