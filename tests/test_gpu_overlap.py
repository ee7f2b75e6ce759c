"""GPU: overlapped launches (include/urt.h option "overlap_launches" — here 2 = always, so that the pipelined readbacks the tests observe the
frames with do not switch it off as the default "auto" would; frame_batch.cpp flush_pending).

A host that presents or reads back EVERY frame (RM:798-821 once per displayed frame — how the reference really runs) submits one-frame
launches; the library alternates them between two trace streams of its own, takes their Result slots round-robin from the slab and lets
launch L+1 start without waiting for launch L, while blends / presents / readbacks stay on the main stream in program order.  The
observable sequence must not change:

  * every frame delivered by the pipelined readback == the same sequence with overlap off and one launch per frame, bit for bit, in all
    three present formats, `_target` and the counters too; the last frame == the oracle;
  * the same with everything that forces the narrow dependency to widen mixed in: objects moved between frames (refit), SetPixels /
    GetPixels on the images, a second camera (another Result texture), small batches of 2..5 frames per submission, a slab wrap;
  * and the launches really overlap (urt_debug_launch_info: trace stream 1 / 2 alternating, `overlapped` set, slots rotating)."""
import copy

import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import RayTraceMaster, RenderTexture, debug_build_blas, host_io, scenes

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_stream(ctx, sc, n, overlap, fpl, script=None, fmt="RGBA32F", group=1):
    """n submissions of `group` frames each through RM's protocol with a pipelined readback of `destination` after every submission (two in
    flight); script(i, m, dest) may disturb the main stream before submission i.  Returns the frames read, the final images, counters, infos."""
    ctx.set_option("kernel_mode", 3)
    ctx.set_option("overlap_launches", overlap)
    ctx.set_option("frames_per_launch", fpl)
    try:
        m = RayTraceMaster(ctx, sc)
        dest = RenderTexture(ctx, sc.width, sc.height)
        ctx.reset_counters()
        got, infos, tickets = [], [], []
        for i in range(n):
            if script:
                script(i, m, dest)
            for _ in range(group):
                m.OnRenderImage(dest)
            tickets.append(dest.ReadBegin(fmt))
            infos.append(ctx.launch_info())
            if len(tickets) > 2:
                got.append(dest.ReadEnd(tickets.pop(0)))
        while tickets:
            got.append(dest.ReadEnd(tickets.pop(0)))
        c = ctx.counters()
        final = (dest.GetPixels(), m._converged.GetPixels(), m._target.GetPixels())
        m.OnDisable()
        dest.Release()
        return got, final, c, infos
    finally:
        ctx.set_option("frames_per_launch", 0)
        ctx.set_option("overlap_launches", 1)


@pytest.mark.parametrize("fmt", ["RGBA32F", "RGBA8_SRGB", "RGBA16F"])
def test_every_frame_presented_and_read_back(gpu_ctx, fmt):
    sc = scenes.mixed_test_scene(200, 120)
    n = 70 if fmt == "RGBA32F" else 12                      # 70 one-frame launches: the slot cursor wraps around the 64-slot slab
    got, final, c, infos = run_stream(gpu_ctx, sc, n, 2, 0, fmt=fmt)
    ref, rfinal, rc, rinfos = run_stream(gpu_ctx, sc, n, 0, 1, fmt=fmt)
    assert len(got) == n and len(ref) == n
    for i in range(n):
        assert bits_equal(got[i], ref[i]), (fmt, i)
    for a, b in zip(final, rfinal):
        assert bits_equal(a, b)
    for k in ("rays", "tri_tests", "blas_nodes", "hit_sky", "dispatches", "launches"):
        assert c[k] == rc[k], k
    assert c["launches"] == n and c["watchdog_trips"] == 0
    # the launches alternate between the two trace streams, rotate through the slab and (from the second on) do not wait for their predecessor
    assert [i["trace_stream"] for i in infos[:6]] in ([1, 2, 1, 2, 1, 2], [2, 1, 2, 1, 2, 1]), infos[:3]
    bases = [i["slab_base"] for i in infos]
    # (the cursor goes on from wherever the previous test left it; the slab may hold more than 64 slots of this size when it was cut for a
    # bigger image before)
    assert all(i["n_frames"] == 1 for i in infos) and all(b == a + 1 or (b == 0 and a == infos[0]["slab_frames"] - 1) for a, b in zip(bases, bases[1:])), bases
    assert infos[0]["overlapped"] == 0 and all(i["overlapped"] == 1 for i in infos[1:]), [i["overlapped"] for i in infos]
    if n > infos[0]["slab_frames"]:
        assert 0 in bases[1:]                                # wrapped around the slab
    assert all(i["trace_stream"] == 0 and i["overlapped"] == 0 for i in rinfos)
    if fmt == "RGBA32F":                                    # and the stream is the documented frame sequence: the last _target == the oracle's frame n-1
        o = pyoracle.Oracle(sc)
        nodes, tri, root, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
        o.set_blas(nodes, tri, root)
        ox, oy, sd = scenes.frame_uniforms(n - 1)
        o.set_frame((ox, oy), sd)
        assert bits_equal(final[2], o.render(mode=1, threads=8))


def test_disturbances_between_the_frames(gpu_ctx):
    """Everything that is NOT the frame loop's own work widens the dependency of the next launch; the sequence stays the same."""
    sc = scenes.mixed_test_scene(160, 104, blob=(40, 31))
    moves = [scenes.trs(translate=(-1.2, 1.6, 0.4), scale=(1.2, 1.0, 0.9), yaw_deg=33.0),
             scenes.trs(translate=(-1.0, 1.5, 0.2), scale=(2.1, 0.45, 1.3), yaw_deg=-71.0),
             scenes.trs(translate=(-0.8, 1.7, 0.5), scale=(1.0, 1.0, 1.0), yaw_deg=10.0)]
    seen = {}

    def script(i, m, dest):
        if i % 5 == 3:                                       # an object moves: SetData -> in-place scene update + refit on the main stream
            mo = sc.mesh_objects.copy()
            mo[0]["localToWorldMatrix"] = moves[(i // 5) % 3]
            m._meshObjectBuffer.SetData(mo)
            m._meshObjectBVHBuffer.SetData(scenes.build_object_bvh(*scenes.mesh_bounds(mo, sc.vertices, sc.indices)))
        if i % 7 == 2:                                       # the host looks at _target (a synchronising read of a slab slot)
            seen.setdefault("target", []).append(m._target.GetPixels())
        if i % 9 == 4:                                       # ... writes the destination itself
            dest.SetPixels(np.full((sc.height, sc.width, 4), 0.25, np.float32))
        if i % 11 == 6:                                      # ... restarts the accumulation
            m._currentSample = 0

    got, final, c, infos = run_stream(gpu_ctx, sc, 36, 2, 0, script=script)
    t1 = seen.pop("target")
    ref, rfinal, rc, _ = run_stream(gpu_ctx, sc, 36, 0, 1, script=script)
    t0 = seen.pop("target")
    for i in range(36):
        assert bits_equal(got[i], ref[i]), i
    for a, b in zip(final, rfinal):
        assert bits_equal(a, b)
    assert len(t0) == len(t1) and all(bits_equal(a, b) for a, b in zip(t0, t1))
    assert c["rays"] == rc["rays"] and c["watchdog_trips"] == 0
    wide = [i for i, inf in enumerate(infos) if inf["overlapped"] == 0]
    assert 0 in wide and 3 in wide and 8 in wide and len(wide) < 24, wide     # scene changes widen the dependency, undisturbed frames do not


def test_small_batches_and_a_second_camera(gpu_ctx):
    """Submissions of 3 frames (three dispatches + blends, then one readback) overlap like single frames; launches of more than eight
    frames, and a second RayTraceMaster rendering into another texture in between, take the main stream."""
    sc = scenes.mixed_test_scene(168, 96)
    got, final, c, infos = run_stream(gpu_ctx, sc, 14, 2, 0, group=3)
    ref, rfinal, rc, _ = run_stream(gpu_ctx, sc, 14, 0, 1, group=3)
    assert all(bits_equal(a, b) for a, b in zip(got, ref)) and all(bits_equal(a, b) for a, b in zip(final, rfinal))
    assert c["launches"] == 14 and rc["launches"] == 42 and c["rays"] == rc["rays"]
    assert all(i["n_frames"] == 3 and i["trace_stream"] in (1, 2) for i in infos) and all(b == a + 3 or b == 0 for a, b in zip([i["slab_base"] for i in infos], [i["slab_base"] for i in infos][1:]))
    big, bfinal, bc, binfos = run_stream(gpu_ctx, sc, 4, 2, 0, group=12)
    rbig, rbfinal, rbc, _ = run_stream(gpu_ctx, sc, 4, 0, 1, group=12)
    assert all(bits_equal(a, b) for a, b in zip(big, rbig)) and all(i["trace_stream"] == 0 and i["n_frames"] == 12 for i in binfos)
    # two cameras alternating: every submission changes the Result texture of the batch
    sc2 = copy.copy(sc)
    sc2.seed = sc.seed + 3.0
    out = {}
    for overlap, fpl in ((2, 0), (0, 1)):
        gpu_ctx.set_option("overlap_launches", overlap)
        gpu_ctx.set_option("frames_per_launch", fpl)
        try:
            a, b = RayTraceMaster(gpu_ctx, sc), RayTraceMaster(gpu_ctx, sc2)
            da, db = RenderTexture(gpu_ctx, sc.width, sc.height), RenderTexture(gpu_ctx, sc.width, sc.height)
            frames = []
            for i in range(6):
                a.OnRenderImage(da)
                ta = da.ReadBegin("RGBA8_SRGB")
                b.OnRenderImage(db)
                tb = db.ReadBegin("RGBA8_SRGB")
                frames += [da.ReadEnd(ta), db.ReadEnd(tb)]
            frames += [a._converged.GetPixels(), b._converged.GetPixels()]
            out[overlap] = frames
            a.OnDisable(); b.OnDisable(); da.Release(); db.Release()
        finally:
            gpu_ctx.set_option("frames_per_launch", 0)
            gpu_ctx.set_option("overlap_launches", 1)
    assert all(bits_equal(x, y) for x, y in zip(out[2], out[0]))
    assert np.array_equal(out[2][-4], host_io.encode_srgb8(out[2][-2]))     # the last present of camera a IS its running mean, encoded


def test_auto_overlaps_only_while_no_readback_is_in_flight(gpu_ctx):
    sc = scenes.mixed_test_scene(168, 96)
    gpu_ctx.set_option("kernel_mode", 3)
    m = RayTraceMaster(gpu_ctx, sc)
    dest = RenderTexture(gpu_ctx, sc.width, sc.height)
    streams = []
    for i in range(4):                                       # submitted frame by frame, never read: overlapped
        m.OnRenderImage(dest)
        gpu_ctx.flush()
        streams.append(gpu_ctx.launch_info()["trace_stream"])
    t = dest.ReadBegin("RGBA8_SRGB")
    m.OnRenderImage(dest)
    gpu_ctx.flush()
    streams.append(gpu_ctx.launch_info()["trace_stream"])   # a ticket is in flight: the context's own stream
    img = dest.ReadEnd(t)
    m.OnRenderImage(dest)
    gpu_ctx.flush()
    streams.append(gpu_ctx.launch_info()["trace_stream"])
    assert streams[:4] in ([1, 2, 1, 2], [2, 1, 2, 1]) and streams[4] == 0 and streams[5] in (1, 2), streams
    conv = m._converged.GetPixels()
    m.OnDisable(); dest.Release()
    gpu_ctx.set_option("overlap_launches", 0)
    try:
        m = RayTraceMaster(gpu_ctx, sc)
        for i in range(6):
            m.OnRenderImage()
            if i == 3:
                want4 = host_io.encode_srgb8(m._converged.GetPixels())
        assert bits_equal(conv, m._converged.GetPixels()) and np.array_equal(img, want4)
        m.OnDisable()
    finally:
        gpu_ctx.set_option("overlap_launches", 1)
