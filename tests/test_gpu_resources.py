"""GPU: a context, a group and a failed creation give back every device byte, pinned byte, event and stream they took.

The holders of csrc/owned.h keep a process-wide tally (urt_debug_live_resources).  Each test takes the tally with the session's
context alive, drives every site that allocates or creates something — once, and again at a larger size where the site grows — and
compares the tally after close() with the one before.  A site that is never reached leaves the tally where it was too, so the
streams, the events and the growth of a read slot are also counted before close().  Device-wide free memory on a shared card says
nothing; the tally is exact."""
import numpy as np
import pytest

from unityraytracer_amd import Context, DeviceGroup, RayTraceMaster, RenderTexture, UrtError, live_resources, scenes

pytestmark = pytest.mark.gpu

W, H = 64, 40


def frames(m, n, flush=False):
    for _ in range(n):
        m.OnRenderImage()
        if flush:
            m.ctx.flush()


def test_a_context_returns_everything_it_took(gpu_ctx):
    import torch
    base = live_resources()
    ctx = Context(0)
    mid = live_resources()
    assert mid["device_bytes"] > base["device_bytes"] and mid["streams"] == base["streams"] + 1
    sc = scenes.mixed_test_scene(W, H)
    m = RayTraceMaster(ctx, sc)
    frames(m, 3)                                             # deferred frames: the Result slab, the frame tables, the work counters
    ctx.synchronize()
    ctx.set_option("overlap_launches", 2)                    # the two trace streams and their events
    frames(m, 4, flush=True)
    ctx.set_option("overlap_launches", 1)
    theirs = torch.cuda.Stream(device="cuda:0")
    ctx.set_stream(theirs.cuda_stream)                       # the event that orders the old stream before the new one
    ctx.set_stream(None)
    ctx.set_option("time_dispatch", 1)                       # the event pool: two events per timed launch
    launches = ctx.counters()["launches"]
    frames(m, 2)
    c = ctx.counters()
    timed = c["launches"] - launches
    assert c["dispatches"] == 9 and timed >= 1
    ctx.set_option("time_dispatch", 0)
    for mode in (1, 5, 3):                                   # the path queues (1), the mailbox (5)
        ctx.set_option("kernel_mode", mode)
        frames(m, 1)
    for builder in (3, 0):                                   # two full preparations: free_scene, the GPU builder's output, the host builder's uploads
        ctx.set_option("blas_builder", builder)
        frames(m, 1)
        assert ctx.launch_info()["blas_builder"] == builder
    moved = sc.mesh_objects[0]["localToWorldMatrix"].copy().reshape(16)
    moved[12] += 0.25                                        # a translation: the refit tables
    refits = ctx.refit_stats()[0]
    m.MoveObjects(mesh_edits={0: moved})
    frames(m, 1)
    assert ctx.refit_stats()[0] == refits + 1
    sky, m.SkyboxTexture = m.SkyboxTexture, None             # _SkyboxTexture unbound: the one black texel
    frames(m, 1)
    m.SkyboxTexture = sky
    small, large = RenderTexture(ctx, W, H), RenderTexture(ctx, 96, 64)
    for t in (small, small, small, large):                   # the three read slots, the sRGB table, the copy stream; the fourth read regrows slot 0
        before = live_resources()
        assert t.ReadEnd(t.ReadBegin("RGBA8_SRGB")).shape == (t.height, t.width, 4)
    grown = {k: live_resources()[k] - before[k] for k in before}
    assert grown == {"device_bytes": (96 * 64 - W * H) * 16, "pinned_bytes": (96 * 64 - W * H) * 16, "events": 0, "streams": 0}
    rng = np.random.default_rng(7)
    for n in (64, 4096):                                     # the ray-query pair, regrown
        o = np.tile(np.float32([0, 1, -10]), (n, 1))
        assert len(ctx.ray_query(o, rng.standard_normal((n, 3)).astype(np.float32))) == n
    m.ResamplePixels(np.zeros((16, 2), np.int32))            # binds Result; the radiance-query pair and its work counter ...
    xy = np.stack([np.arange(2048) % W, np.arange(2048) // W % H], axis=1).astype(np.int32)
    assert ctx.radiance_query_pixels(xy, 1, 2).shape == (2048, 4)     # ... regrown
    assert ctx.render_aov_arrays(W, H)["kind"].shape == (H, W)
    for h, w in ((16, 16), (H, W)):                          # the denoiser's three images, regrown
        z = np.zeros((h, w, 4), np.float32)
        assert ctx.denoise_arrays(z, z, z).shape == (h, w, 4)
    z = np.zeros((H, W, 4), np.float32)
    ident = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (3, 1))
    for rows in (1, 3):                                      # the motion table, regrown
        ctx.reproject_arrays(z, z, z, z, z, z, z, z, np.eye(4, dtype=np.float32).reshape(16), sc.camera_to_world, sc.camera_inverse_projection,
                             mesh_motion=ident[:rows])
    dst, count = RenderTexture(ctx, W, H), RenderTexture(ctx, W, H)
    count.SetPixels(z)
    assert ctx.resample_below(dst, count, 1.0, 1, 2) == W * H     # the block counts, the pinned total, the pixel list and its samples
    mine = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    RenderTexture(ctx, W, H, external_ptr=mine.data_ptr())            # not the library's memory: never counted, never freed
    end = live_resources()
    assert end["device_bytes"] > mid["device_bytes"] and end["pinned_bytes"] > mid["pinned_bytes"]
    assert end["streams"] == base["streams"] + 1 + 2 + 1     # the context's own, the two trace streams, the copy stream
    # frame tables 4, trace streams 2 + 2 + 1, two per timed launch, read slots 3 x 2, the stream switch 1
    assert end["events"] == base["events"] + 4 + 5 + 2 * timed + 6 + 1
    small.Release()                                          # one texture released early; large, dst, count, the external one and the master's are left to close()
    ctx.close()
    assert live_resources() == base
    assert float(mine.sum()) == 0.0                          # the caller's memory is still the caller's


def test_a_group_returns_everything_it_took(gpu_ctx):
    base = live_resources()
    g = DeviceGroup([0, 0])
    sc = scenes.mixed_test_scene(W, H)
    m = RayTraceMaster(g, sc)
    full = RenderTexture(g, W, H)
    frames(m, 1)
    g.gather(m._converged, full)
    a, b = RenderTexture(g, 96, 64), RenderTexture(g, 96, 64)
    g.gather(a, b)                                           # a larger image: the staging buffers grow
    g.synchronize()
    assert live_resources()["events"] >= base["events"] + 2 * 2 * 16
    g.close()
    assert live_resources() == base


def test_a_failed_create_holds_nothing(gpu_ctx):
    """A device ordinal out of range is refused before a context exists: this holds the refusal to the tally, not the unwinding of a
    partly built context, which no test reaches (it takes an allocation that fails)."""
    base = live_resources()
    with pytest.raises(UrtError):
        Context(10 ** 6)
    assert live_resources() == base
