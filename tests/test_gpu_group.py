"""GPU: urt_group_* — one host thread drives N ranks through the C ABI (include/urt.h "device groups").  The 1-GPU box
hosts the ranks on one card (the device list repeats ordinal 0); strip dispatch, local accumulation, pack kernels, the peer
copies to rank 0 and the de-interleave all run for real.  Whatever rank 0 holds after a gather must be bit-identical to
the same frames rendered by a single context."""
import numpy as np
import pytest

from unityraytracer_amd import DeviceGroup, RayTraceMaster, RenderTexture, UrtError, scenes

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def single_context_frames(ctx, sc, n):
    ctx.set_option("kernel_mode", 3)
    m = RayTraceMaster(ctx, sc)
    out = []
    for _ in range(n):
        m.OnRenderImage()
        out.append(m._converged.GetPixels())
    m.OnDisable()
    return out


@pytest.mark.parametrize("ranks,fpl", [(2, 0), (3, 0), (4, 1), (3, 5)])
def test_group_gather_equals_single_context(gpu_ctx, ranks, fpl):
    sc = scenes.mixed_test_scene(176, 120)                 # 15 group rows: ragged over 2, 3 and 4 ranks
    n = 7
    ref = single_context_frames(gpu_ctx, sc, n)
    with DeviceGroup([0] * ranks) as g:
        assert g.size == ranks
        g.set_option("frames_per_launch", fpl)
        m = RayTraceMaster(g, sc)                          # the reference's driver, unchanged, on a group
        full = RenderTexture(g, sc.width, sc.height)
        peeks = {}
        for i in range(n):
            m.OnRenderImage()
            g.gather(m._converged, full)                   # ONE exchange per frame
            if i in (2, n - 1):
                peeks[i] = full.GetPixels()                # rank 0's full image after frame i
        c = g.counters()
        assert c["dispatches"] == n and c["watchdog_trips"] == 0
        if fpl != 1:
            assert c["launches"] < n                       # the ranks really batched frames under a gather-every-frame protocol
        for i, img in peeks.items():
            assert bits_equal(img, ref[i]), (ranks, fpl, i)
        full.Release()
        m.OnDisable()


def test_group_counts_rays_once_and_rejects_foreign_objects(gpu_ctx):
    sc = scenes.config1(96, 64)
    gpu_ctx.reset_counters()
    single_context_frames(gpu_ctx, sc, 2)
    want = gpu_ctx.counters()["rays"]
    with DeviceGroup([0, 0]) as g:
        m = RayTraceMaster(g, sc)
        for _ in range(2):
            m.OnRenderImage()
        assert g.counters()["rays"] == want                # every pixel is traced by exactly one rank
        m.OnDisable()
        # an object created on ONE rank's context behind the group's back breaks the shared handle numbering: reported, not ignored
        import ctypes as C
        raw = g._raw
        h = C.c_uint64()
        assert raw.urt_buffer_create(C.c_void_p(raw.urt_group_context(g._h, 1)), 4, 12, C.byref(h)) == 0
        with pytest.raises(UrtError) as e:
            RenderTexture(g, 8, 8)
        assert e.value.code == 2


@pytest.mark.parametrize("fpl", [0, 1])
def test_group_present_after_gather_is_ordered(gpu_ctx, fpl):
    """gather(_converged -> full) followed by the present Blit(full, destination) (RM:819), a larger image gathered while
    gathers are still queued (the staging buffers grow), SetPixels into a gather target: every call sees the gathers before it
    in program order.  (Round 2 forwarded these calls past the queued gathers: the present showed a stale image.)"""
    from unityraytracer_amd import Graphics
    sc = scenes.mixed_test_scene(176, 120)
    n = 6
    ref = single_context_frames(gpu_ctx, sc, n)
    with DeviceGroup([0, 0, 0]) as g:
        g.set_option("frames_per_launch", fpl)
        m = RayTraceMaster(g, sc)
        full = RenderTexture(g, sc.width, sc.height)
        dest = RenderTexture(g, sc.width, sc.height)
        peeks = {}
        for i in range(n):
            m.OnRenderImage()
            g.gather(m._converged, full)
            Graphics.Blit(full, dest)                      # the present of the gathered frame
            if i == 3:
                peeks[i] = dest.GetPixels()
        assert bits_equal(peeks[3], ref[3]) and bits_equal(dest.GetPixels(), ref[n - 1]), fpl
        if fpl != 1:
            assert g.counters()["launches"] < n            # the presents did not break the ranks' batching
        # a second, larger scene on the same group while gathers of the first are queued: staging is re-allocated safely
        sc2 = scenes.mixed_test_scene(264, 168)
        ref2 = single_context_frames(gpu_ctx, sc2, 2)
        m.OnRenderImage()
        g.gather(m._converged, full)                       # queued (frames are deferred when fpl != 1)
        m2 = RayTraceMaster(g, sc2)
        full2 = RenderTexture(g, sc2.width, sc2.height)
        for _ in range(2):
            m2.OnRenderImage()
            g.gather(m2._converged, full2)
        assert bits_equal(full2.GetPixels(), ref2[1])
        # SetPixels into a gather target after a queued gather wins over the gather
        m2.OnRenderImage()
        g.gather(m2._converged, full2)
        flat = np.full((sc2.height, sc2.width, 4), 0.5, np.float32)
        full2.SetPixels(flat)
        assert bits_equal(full2.GetPixels(), flat)
        full.Release(); dest.Release(); full2.Release()
        m.OnDisable(); m2.OnDisable()


@pytest.mark.parametrize("fpl", [0, 1])
def test_group_blit_of_a_gather_source_keeps_program_order(gpu_ctx, fpl):
    """gather(_converged -> full), then Blit(_converged, snap), then two more frames: `snap` must hold the mean after the frame the
    blit followed — a blit that reads a gather's SOURCE is ordered by the ranks' own deferred operations and must not be queued
    behind the late unpack, where it would run after frames dispatched later (group.cpp urt_group_blit)."""
    from unityraytracer_amd import Graphics
    sc = scenes.mixed_test_scene(176, 120)
    n = 5
    ref = single_context_frames(gpu_ctx, sc, n)
    with DeviceGroup([0, 0, 0]) as g:
        g.set_option("frames_per_launch", fpl)
        m = RayTraceMaster(g, sc)
        full = RenderTexture(g, sc.width, sc.height)
        snap = RenderTexture(g, sc.width, sc.height)
        for i in range(n):
            m.OnRenderImage()
            g.gather(m._converged, full)
            if i == 2:
                Graphics.Blit(m._converged, snap)          # every rank copies ITS strips of the mean after frame 2
        g.gather(snap, full)                               # bring the snapshot's strips together
        assert bits_equal(full.GetPixels(), ref[2]), fpl
        full.Release(); snap.Release()
        m.OnDisable()


# ---- ragged strip sets, ranks that own no strip, a scene that changes, the other kernel modes ----------------------------------------
NINE = ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere", "hit_ground", "hit_sky")


def single_context_run(ctx, sc, n, mode=3, count=False):
    """the running mean after each of n frames on one context, and its counters"""
    try:
        ctx.set_option("kernel_mode", mode)
        ctx.set_option("count_stats", 1 if count else 0)
        ctx.reset_counters()
        m = RayTraceMaster(ctx, sc)
        out = []
        for _ in range(n):
            m.OnRenderImage()
            out.append(m._converged.GetPixels())
        c = ctx.counters()
        m.OnDisable()
        return out, c
    finally:
        ctx.set_option("kernel_mode", 3)
        ctx.set_option("count_stats", 0)


@pytest.mark.parametrize("fpl", [0, 1])
@pytest.mark.parametrize("w,h,ranks", [(52, 44, 2), (52, 44, 3), (52, 44, 5), (52, 44, 8), (9, 7, 2), (9, 7, 3)])
def test_group_with_ragged_strips_and_idle_ranks(gpu_ctx, w, h, ranks, fpl):
    """52x44 is 6 group rows, the last of 4 pixel rows: over 5 ranks rank 0 owns two strips and the others one, over 8 ranks two own none;
    9x7 is one group row, so every rank but the first is idle.  The staging is sized by rank 0 (csrc/group.cpp urt_group_gather) and an
    idle rank packs and unpacks nothing.  Image and device counters equal a single context's."""
    sc = scenes.mixed_test_scene(w, h)
    n = 5
    ref, rc = single_context_run(gpu_ctx, sc, n, count=True)
    with DeviceGroup([0] * ranks) as g:
        g.set_option("frames_per_launch", fpl)
        g.set_option("count_stats", 1)
        g.reset_counters()
        m = RayTraceMaster(g, sc)
        full = RenderTexture(g, w, h)
        peeks = {}
        for i in range(n):
            m.OnRenderImage()
            g.gather(m._converged, full)
            if i in (2, 4):
                peeks[i] = full.GetPixels()
        c = g.counters()
        full.Release()
        m.OnDisable()
    for i, img in peeks.items():
        assert bits_equal(img, ref[i]), (w, h, ranks, fpl, i)
    assert c["watchdog_trips"] == 0 and c["dispatches"] == n
    assert {k: c[k] for k in NINE} == {k: rc[k] for k in NINE}, (w, h, ranks, fpl)


def drive_changing_scene(m, after_frame, read):
    """3 frames; one mesh's localToWorldMatrix changes; 2 frames; the blob's vertices change through ranged SetData; 2 frames; the camera
    moves; 2 frames.  after_frame() follows every frame, read() returns the image after every step."""
    sc = m.scene
    out = []

    def frames(k):
        for _ in range(k):
            m.OnRenderImage()
            after_frame()
        out.append(read())

    frames(3)
    m.MoveObjects(mesh_edits={1: scenes.trs(translate=(2.0, 1.3, -0.5), scale=1.1, yaw_deg=15.0)})     # the matrix refit (csrc/refit.hip)
    frames(2)
    lo, hi = m.vertex_span(0)
    v = np.array(np.asarray(sc.vertices, np.float32).reshape(-1, 3)[lo: hi + 1])
    v[:, 1] = v[:, 1] * np.float32(0.75) + np.float32(0.1) * np.sin(v[:, 0] * np.float32(3.0))
    m.DeformMeshes({0: v})                                        # _vertexBuffer.SetData(v, 0, lo, len(v)): the in-place refit of the deformed mesh
    frames(2)
    c2w, invp = scenes.camera_matrices(sc.width, sc.height, position=(0.6, 1.4, -9.0), yaw_deg=6.0, pitch_deg=-3.0)
    m.MoveCamera(c2w, invp)
    frames(2)
    return out


def edit_stats(lib, ctx_handle):
    """(MeshObjects refitted after a matrix change, preparations done in place, deformed MeshObjects refitted in place, MeshObjects whose
    normals were re-gathered, full preparations forced) of one context since its creation: urt_debug_refit_stats, urt_debug_deform_stats"""
    import ctypes as C
    a, b, d = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)()
    assert lib.urt_debug_refit_stats(ctx_handle, C.byref(a), C.byref(b)) == 0
    assert lib.urt_debug_deform_stats(ctx_handle, d) == 0
    return a.value, b.value, int(d[0]), int(d[1]), int(d[3])


@pytest.mark.parametrize("fpl", [0, 1])
def test_group_follows_a_changing_scene(gpu_ctx, fpl):
    """The same host sequence on a group of 3 and on one context: matrix edit, ranged vertex edit (urt_group_buffer_set_data_range),
    camera move — every rank refits and re-binds as the single context does; the gathered mean is bit-equal after every step."""
    import copy
    sc = scenes.mixed_test_scene(52, 44)
    before = edit_stats(gpu_ctx.lib, gpu_ctx._h)
    m1 = RayTraceMaster(gpu_ctx, copy.deepcopy(sc))
    ref = drive_changing_scene(m1, lambda: None, lambda: m1._converged.GetPixels())
    m1.OnDisable()
    single = tuple(b - a for a, b in zip(before, edit_stats(gpu_ctx.lib, gpu_ctx._h)))
    assert single[0] >= 1 and single[2] >= 1, single             # the matrix refit and the in-place update of the deformed mesh both ran
    assert not bits_equal(ref[0], ref[1]) and not bits_equal(ref[1], ref[2]) and not bits_equal(ref[2], ref[3])     # every edit shows
    with DeviceGroup([0, 0, 0]) as g:
        g.set_option("frames_per_launch", fpl)
        m = RayTraceMaster(g, copy.deepcopy(sc))
        full = RenderTexture(g, sc.width, sc.height)
        got = drive_changing_scene(m, lambda: g.gather(m._converged, full), lambda: full.GetPixels())
        assert g.counters()["watchdog_trips"] == 0
        import ctypes as C
        for r in range(g.size):                                   # every rank took the same refit paths as the single context
            assert edit_stats(g._raw, C.c_void_p(g._raw.urt_group_context(g._h, r))) == single, (r, single)
        full.Release()
        m.OnDisable()
    for step, (a, b) in enumerate(zip(got, ref)):
        assert bits_equal(a, b), (fpl, "after step", step)


@pytest.mark.parametrize("mode", [0, 2, 5])
def test_group_in_other_kernel_modes(gpu_ctx, mode):
    """(mode 3 runs everywhere above; the strip dispatch of modes 1 and 4 is held by tests/test_gpu_frame_shapes.py)"""
    sc = scenes.mixed_test_scene(52, 44)
    n = 3
    ref, _ = single_context_run(gpu_ctx, sc, n, mode=mode)
    with DeviceGroup([0, 0, 0]) as g:
        g.set_option("kernel_mode", mode)
        m = RayTraceMaster(g, sc)
        full = RenderTexture(g, sc.width, sc.height)
        for i in range(n):
            m.OnRenderImage()
            g.gather(m._converged, full)
            assert bits_equal(full.GetPixels(), ref[i]), (mode, i)
        assert g.counters()["watchdog_trips"] == 0
        full.Release()
        m.OnDisable()
