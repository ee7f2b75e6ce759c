"""GPU: the resampling step (include/urt.h urt_select_pixels, urt_blend_samples, urt_resample_below) — bit for bit against the numpy
restatements of tests/resample_ref.py: the ordered compaction on both sides of every wave, workgroup and chunk boundary, the capacity
and count-only forms, the sparse blend with skipped pixels and against urt_blit_add_history, the one-call form against the three calls,
RayTraceMaster.ResampleDisocclusions end to end, ordering with deferred frames, and every argument error against sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

from reproject_ref import blit_add_history_ref
from resample_ref import blend_samples_ref, select_pixels_ref
from unityraytracer_amd import Context, RayTraceMaster, UrtError, scenes
from unityraytracer_amd.unity_api import SELECT_CHUNK, ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

F = np.float32
NAN, INF = float("nan"), float("inf")


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, ref, what):
    bad = u32(got) != u32(ref)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} texels differ, first at {np.argwhere(bad)[0]}"


def count_image(w, h, x, rng):
    c = rng.uniform(-9, 9, (h, w, 4)).astype(F)                     # .yzw are junk: only .x counts
    c[..., 0] = np.asarray(x, F).reshape(h, w)
    return c


def device(ctx):
    return torch.device("cuda", ctx.device)


# ---- 1. select ---------------------------------------------------------------------------------------------------------------------------
# one wave, one workgroup round, one chunk (SELECT_CHUNK texels per workgroup) and two chunks, each with the last texel before, on and
# after the boundary; 257 x 131 spans 17 chunks with rows that end inside a wave
SIZES = [(1, 1), (63, 1), (64, 1), (1, 65), (255, 1), (256, 1), (257, 1),
         (23, 89), (64, 32), (3, 683), (63, 65), (64, 64), (17, 241), (257, 131)]


def test_sizes_sit_on_the_chunk_boundaries():
    assert SELECT_CHUNK == 2048
    assert [w * h for w, h in SIZES[7:13]] == [SELECT_CHUNK - 1, SELECT_CHUNK, SELECT_CHUNK + 1,
                                               2 * SELECT_CHUNK - 1, 2 * SELECT_CHUNK, 2 * SELECT_CHUNK + 1]
    assert 257 * 131 > 16 * SELECT_CHUNK


def masks(w, h, rng):
    n = w * h
    first, last = np.ones(n, F), np.ones(n, F)
    first[0], last[-1] = 0.0, 0.0
    special = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, 4.5, 5.0, 100.0, NAN, INF, -INF, -1.0, -0.0], F), n)
    return [("none", np.full(n, 3.0, F), 1.0), ("all", np.zeros(n, F), 1.0), ("first", first, 1.0), ("last", last, 1.0),
            ("half", (rng.random(n) < 0.5).astype(F), 1.0), ("special_1", special, 1.0), ("special_4.5", special, 4.5)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_matches_reference(gpu_ctx, size):
    w, h = size
    rng = np.random.default_rng(1000 * w + h)
    with Context(gpu_ctx.device) as ctx:
        tex = RenderTexture(ctx, w, h)
        for name, x, below in masks(w, h, rng):
            img = count_image(w, h, x, rng)
            tex.SetPixels(img)
            ref = select_pixels_ref(img, below)
            got = ctx.select_pixels(tex, below)
            assert got.dtype == torch.int32 and got.device == device(ctx) and tuple(got.shape) == (len(ref), 2), (name, got.shape, len(ref))
            assert np.array_equal(got.cpu().numpy(), ref), name
            assert tex.GetPixels().tobytes() == img.tobytes(), name                  # the count texture is only read
        tex.Release()


# ---- 2. capacity -------------------------------------------------------------------------------------------------------------------------
def test_capacity_prefix_tail_and_count_only(gpu_ctx):
    w, h = 257, 131
    rng = np.random.default_rng(2)
    img = count_image(w, h, (rng.random(w * h) < 0.4).astype(F), rng)
    ref = select_pixels_ref(img, 1.0)
    n = len(ref)
    assert n > 4 * SELECT_CHUNK
    with Context(gpu_ctx.device) as ctx:
        tex = RenderTexture(ctx, w, h)
        tex.SetPixels(img)
        out = C.c_int(-1)
        ctx.check(ctx.lib.urt_select_pixels(ctx._h, tex.handle, 1.0, None, 0, C.byref(out)))      # count only
        assert out.value == n
        for cap in (n // 2, 1, n, n + 100):
            buf = torch.full((n + 200, 2), -77, dtype=torch.int32, device=device(ctx))
            torch.cuda.synchronize()
            out = C.c_int(-1)
            ctx.check(ctx.lib.urt_select_pixels(ctx._h, tex.handle, 1.0, C.c_void_p(buf.data_ptr()), cap, C.byref(out)))
            got = buf.cpu().numpy()
            k = min(cap, n)
            assert out.value == n, cap                                                # the total, whatever fits
            assert np.array_equal(got[:k], ref[:k]), cap
            assert (got[k:] == -77).all(), cap                                        # nothing beyond the capacity (or the list) is touched
        tex.Release()


# ---- 3. blend ----------------------------------------------------------------------------------------------------------------------------
BW, BH = 37, 23
OUTSIDE = np.array([[-1, 0], [BW, 0], [0, BH], [0, -1], [BW + 5, BH + 5], [2**31 - 1, 2**31 - 1], [-2**31, 3], [3, -2**31]], np.int32)


def blend_case(n, rng):
    """n list entries: distinct pixels in shuffled order, every ninth entry replaced by a pixel outside the image."""
    flat = rng.permutation(BW * BH)[:n]
    xy = np.stack([flat % BW, flat // BW], axis=1).astype(np.int32)
    for k, i in enumerate(range(4, n, 9)):
        xy[i] = OUTSIDE[k % len(OUTSIDE)]
    samples = rng.uniform(0, 4, (n, 4)).astype(F)
    dst = rng.uniform(0, 4, (BH, BW, 4)).astype(F)
    cnt = count_image(BW, BH, rng.choice(np.array([0.0, 0.25, 1.0, 5.5, 7.0, 7.5, 8.0, 63.0, 1e30, NAN, INF, -INF, -1.0, -0.0], F), BW * BH), rng)
    return xy, samples, dst, cnt


@pytest.mark.parametrize("n", [0, 1, 63, 64, 257])
def test_blend_matches_reference(gpu_ctx, n):
    rng = np.random.default_rng(30 + n)
    with Context(gpu_ctx.device) as ctx:
        dst, cnt = RenderTexture(ctx, BW, BH), RenderTexture(ctx, BW, BH)
        for weight in (1.0, 2.0, 0.5):
            for mh in (0.0, 1.0, 8.0):
                xy, samples, d, c = blend_case(n, rng)
                dst.SetPixels(d); cnt.SetPixels(c)
                ctx.blend_samples(torch.from_numpy(xy).to(device(ctx)), torch.from_numpy(samples).to(device(ctx)), dst, cnt, weight, mh)
                rd, rc = blend_samples_ref(xy, samples, d, c, weight, mh)
                what = f"n={n} weight={weight} mh={mh}"
                assert_bits(dst.GetPixels(), rd, what + " dst")                       # the skipped and the unlisted texels included
                assert_bits(cnt.GetPixels(), rc, what + " count")
                if n >= 63:
                    assert (u32(rd) != u32(d)).any(), what
        dst.Release(); cnt.Release()


@pytest.mark.parametrize("mh", [0.0, 8.0])
def test_whole_frame_blend_of_weight_one_is_blit_add_history(gpu_ctx, mh):
    rng = np.random.default_rng(40)
    X, Y = np.meshgrid(np.arange(BW, dtype=np.int32), np.arange(BH, dtype=np.int32))
    xy = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)                            # natural order
    _, _, d, c = blend_case(0, rng)
    s = rng.uniform(0, 4, (BH, BW, 4)).astype(F)
    with Context(gpu_ctx.device) as ctx:
        src, dst, cnt, dst2, cnt2 = (RenderTexture(ctx, BW, BH) for _ in range(5))
        src.SetPixels(s); dst.SetPixels(d); cnt.SetPixels(c); dst2.SetPixels(d); cnt2.SetPixels(c)
        ctx.blit_add_history(src, dst, cnt, mh)
        ctx.blend_samples(torch.from_numpy(xy).to(device(ctx)), torch.from_numpy(s.reshape(-1, 4)).to(device(ctx)), dst2, cnt2, 1.0, mh)
        a, an, b, bn = dst.GetPixels(), cnt.GetPixels(), dst2.GetPixels(), cnt2.GetPixels()
        for t in (src, dst, cnt, dst2, cnt2):
            t.Release()
    assert_bits(b, a, "dst")
    assert_bits(bn, an, "count")
    rd, rn = blit_add_history_ref(s, d, c, mh)
    assert_bits(a, rd, "dst vs reference")
    assert_bits(an, rn, "count vs reference")


# ---- 4. the one-call form ----------------------------------------------------------------------------------------------------------------
def moved_master(ctx, w=96, h=64, max_history=None):
    """The input of tests/test_gpu_radiance_query.py::test_resample_pixels_of_a_disocclusion_mask: four frames, then a 3 degree yaw."""
    sc = scenes.mixed_test_scene(w, h)
    m = RayTraceMaster(ctx, sc)
    m.numRays = 2
    m.EnableTemporalAccumulation(**({} if max_history is None else {"max_history": max_history}))
    for _ in range(4):
        m.OnRenderImage()
    m.MoveCamera(*scenes.camera_matrices(w, h, position=(0.6, 1.0, -10.0), yaw_deg=3.0))
    return m


@pytest.mark.parametrize("below,weight,mh", [(1.0, 1.0, 64.0), (4.5, 2.0, 8.0), (0.0, 1.0, 0.0)])
def test_resample_below_equals_the_three_calls(gpu_ctx, below, weight, mh):
    w, h = 96, 64
    with Context(gpu_ctx.device) as ctx:
        m = moved_master(ctx, w, h)
        conv0, cnt0 = m._converged.GetPixels(), m._tcount.GetPixels()
        m._bind_for_queries()
        m.InitRenderTexture()
        m.RayTraceShader.SetTexture(0, "Result", m._target)
        n = ctx.resample_below(m._converged, m._tcount, below, m.numRays, m.numBounces, weight, mh)
        one = (m._converged.GetPixels(), m._tcount.GetPixels())
        m._converged.SetPixels(conv0); m._tcount.SetPixels(cnt0)
        xy = ctx.select_pixels(m._tcount, below)
        samples = ctx.radiance_query_pixels(xy, m.numRays, m.numBounces)
        ctx.blend_samples(xy, samples, m._converged, m._tcount, weight, mh)
        three = (m._converged.GetPixels(), m._tcount.GetPixels())
        m.OnDisable()
    ref_xy = select_pixels_ref(cnt0, below)
    assert n == len(xy) == len(ref_xy) and np.array_equal(xy.cpu().numpy(), ref_xy)
    assert n == {1.0: n, 4.5: w * h, 0.0: 0}[below] and (below != 1.0 or 0 < n < w * h // 2)
    assert_bits(one[0], three[0], "converged")
    assert_bits(one[1], three[1], "count")
    rd, rc = blend_samples_ref(ref_xy, samples.cpu().numpy(), conv0, cnt0, weight, mh)
    assert_bits(one[0], rd, "converged vs reference")
    assert_bits(one[1], rc, "count vs reference")
    if n == 0:
        assert one[0].tobytes() == conv0.tobytes() and one[1].tobytes() == cnt0.tobytes()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
def test_resample_disocclusions_end_to_end(gpu_ctx):
    w, h = 96, 64
    with Context(gpu_ctx.device) as ctx:
        m = moved_master(ctx, w, h)
        conv0, cnt0 = m._converged.GetPixels(), m._tcount.GetPixels()
        zero = cnt0[..., 0] == 0
        c0 = ctx.counters()
        n = m.ResampleDisocclusions()
        c1 = ctx.counters()
        conv1, cnt1 = m._converged.GetPixels(), m._tcount.GetPixels()
        ys, xs = np.nonzero(zero)
        xy = np.stack([xs, ys], axis=1).astype(np.int32)
        fresh = ctx.radiance_query_pixels(xy, m.numRays, m.numBounces)               # the uniforms ResampleDisocclusions bound are still bound
        m.OnDisable()
    assert n == int(zero.sum()) and 0 < n < w * h // 2
    assert c1 == c0 and c1["launches"] == c0["launches"]
    assert (cnt1[zero] == np.array([1, 0, 0, 0], F)).all()
    assert np.array_equal(u32(conv1[zero]), u32(fresh))
    assert (fresh[:, :3] > 0).any() and (fresh[:, 3] == 1).all()
    assert conv1[~zero].tobytes() == conv0[~zero].tobytes() and cnt1[~zero].tobytes() == cnt0[~zero].tobytes()


def test_resample_disocclusions_needs_temporal_accumulation(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(32, 24))
        m.OnRenderImage()
        with pytest.raises(UrtError):
            m.ResampleDisocclusions()
        m.EnableTemporalAccumulation()
        with pytest.raises(UrtError):                                                # enabled, but nothing accumulated yet
            m.ResampleDisocclusions()
        m.OnRenderImage()
        assert m.ResampleDisocclusions() == 0                                        # every pixel has one frame
        assert m.ResampleDisocclusions(below=1.5) == 32 * 24
        assert (m._tcount.GetPixels()[..., 0] == 2).all()
        m.OnDisable()


# ---- 6. deferred work --------------------------------------------------------------------------------------------------------------------
def test_select_and_blend_are_ordered_with_deferred_frames(gpu_ctx):
    w, h = 64, 48
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(w, h))
        m.EnableTemporalAccumulation(max_history=0.0)
        for _ in range(3):
            m.OnRenderImage()                                                        # deferred: nothing has run yet
        none = ctx.select_pixels(m._tcount, 3.0)                                     # sees the three frames' counts
        everything = ctx.select_pixels(m._tcount, 3.5)
        conv0, cnt0 = m._converged.GetPixels(), m._tcount.GetPixels()
        assert ctx.launch_info()["n_frames"] == 3                                    # the frames were one deferred batch
        assert len(none) == 0 and (cnt0[..., 0] == 3).all()
        assert np.array_equal(everything.cpu().numpy(), select_pixels_ref(cnt0, 3.5)) and len(everything) == w * h
        flat = rng.permutation(w * h)[:700]
        xy = np.stack([flat % w, flat // w], axis=1).astype(np.int32)
        samples = rng.uniform(0, 4, (700, 4)).astype(F)
        ctx.blend_samples(torch.from_numpy(xy).to(device(ctx)), torch.from_numpy(samples).to(device(ctx)), m._converged, m._tcount, 2.0, 0.0)
        m.OnRenderImage()                                                            # deferred behind the blend: blends on top of it
        conv1, cnt1, frame = m._converged.GetPixels(), m._tcount.GetPixels(), m._target.GetPixels()
        m.OnDisable()
    rd, rc = blend_samples_ref(xy, samples, conv0, cnt0, 2.0, 0.0)
    rd, rc = blit_add_history_ref(frame, rd, rc, 0.0)
    assert_bits(conv1, rd, "converged")
    assert_bits(cnt1, rc, "count")
    assert sorted(set(cnt1[..., 0].reshape(-1).tolist())) == [4.0, 6.0]


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(gpu_ctx):
    w, h = 16, 8
    rng = np.random.default_rng(7)
    with Context(gpu_ctx.device) as ctx:
        lib, hd, dev = ctx.lib, ctx._h, device(ctx)
        sh = ComputeShader(ctx)
        dst, cnt, sky, small, result = (RenderTexture(ctx, w, h), RenderTexture(ctx, w, h), RenderTexture(ctx, w, h), RenderTexture(ctx, 8, 8),
                                        RenderTexture(ctx, w, h))
        snap = {}
        for name, t in (("dst", dst), ("cnt", cnt), ("sky", sky), ("result", result)):
            snap[name] = rng.uniform(0, 0.5, (h, w, 4)).astype(F)                    # counts below 1: a call that ran would select and blend
            t.SetPixels(snap[name])
        small.SetPixels(np.zeros((8, 8, 4), F))
        sh.SetTexture(0, "_SkyboxTexture", sky)
        gone = RenderTexture(ctx, w, h)
        gone_h = gone.handle
        gone.Release()
        pixels = torch.full((w * h, 2), -77, dtype=torch.int32, device=dev)
        xy = torch.zeros((4, 2), dtype=torch.int32, device=dev)
        xy[:, 0] = torch.arange(4)
        samples = torch.full((4, 4), 9.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pp, xp, sp = C.c_void_p(pixels.data_ptr()), C.c_void_p(xy.data_ptr()), C.c_void_p(samples.data_ptr())
        out = C.c_int(-5)
        ARG, HANDLE, UNBOUND = 1, 2, 5

        def unchanged(what):
            ctx.synchronize()
            assert out.value == -5, what
            assert (pixels.cpu().numpy() == -77).all(), what
            for name, t in (("dst", dst), ("cnt", cnt), ("sky", sky), ("result", result)):
                assert t.GetPixels().tobytes() == snap[name].tobytes(), (what, name)

        select = [("below NaN", ARG, (cnt.handle, NAN, pp, 8, C.byref(out))), ("capacity < 0", ARG, (cnt.handle, 1.0, pp, -1, C.byref(out))),
                  ("NULL list", ARG, (cnt.handle, 1.0, None, 8, C.byref(out))), ("NULL out_n", ARG, (cnt.handle, 1.0, pp, 8, None)),
                  ("misaligned list", ARG, (cnt.handle, 1.0, C.c_void_p(pixels.data_ptr() + 4), 8, C.byref(out))),
                  ("count 0", HANDLE, (0, 1.0, pp, 8, C.byref(out))), ("count unknown", HANDLE, (gone_h, 1.0, pp, 8, C.byref(out)))]
        for what, code, a in select:
            assert lib.urt_select_pixels(hd, *a) == code, what
            unchanged("select: " + what)

        d, c = dst.handle, cnt.handle
        blend = [("n < 0", ARG, (xp, sp, -1, 1.0, d, c, 0.0)), ("NULL pixels", ARG, (None, sp, 4, 1.0, d, c, 0.0)),
                 ("NULL samples", ARG, (xp, None, 4, 1.0, d, c, 0.0)), ("weight 0", ARG, (xp, sp, 4, 0.0, d, c, 0.0)),
                 ("weight < 0", ARG, (xp, sp, 4, -1.0, d, c, 0.0)), ("weight NaN", ARG, (xp, sp, 4, NAN, d, c, 0.0)),
                 ("weight inf", ARG, (xp, sp, 4, INF, d, c, 0.0)), ("max_history NaN", ARG, (xp, sp, 4, 1.0, d, c, NAN)),
                 ("max_history < 0", ARG, (xp, sp, 4, 1.0, d, c, -1.0)), ("max_history 0.5", ARG, (xp, sp, 4, 1.0, d, c, 0.5)),
                 ("dst == count", ARG, (xp, sp, 4, 1.0, d, d, 0.0)), ("sizes differ", ARG, (xp, sp, 4, 1.0, d, small.handle, 0.0)),
                 ("dst is the sky", ARG, (xp, sp, 4, 1.0, sky.handle, c, 0.0)), ("count is the sky", ARG, (xp, sp, 4, 1.0, d, sky.handle, 0.0)),
                 ("dst 0", HANDLE, (xp, sp, 4, 1.0, 0, c, 0.0)), ("count unknown", HANDLE, (xp, sp, 4, 1.0, d, gone_h, 0.0)),
                 ("n == 0, weight 0", ARG, (None, None, 0, 0.0, d, c, 0.0))]
        for what, code, a in blend:
            assert lib.urt_blend_samples(hd, *a) == code, what
            unchanged("blend: " + what)
        assert lib.urt_blend_samples(hd, None, None, 0, 1.0, d, c, 0.0) == 0         # n == 0: fine, and nothing happens
        unchanged("blend: n == 0")

        ok = (d, c, 1.0, 1, 2, 1.0, 0.0, C.byref(out))

        def resample(**ch):
            a = dict(zip(("dst", "count", "below", "samples", "bounces", "weight", "max_history", "out_n"), ok))
            a.update(ch)
            return lib.urt_resample_below(hd, *a.values())

        assert resample() == UNBOUND                                                 # no Result texture, no camera
        unchanged("resample: nothing bound")
        sh.SetTexture(0, "Result", result)
        assert resample() == UNBOUND                                                 # still no camera matrices
        unchanged("resample: no camera")
        c2w, invp = scenes.camera_matrices(w, h)
        sh.SetMatrix("_CameraToWorld", c2w)
        sh.SetMatrix("_CameraInverseProjection", invp)
        cases = [("below NaN", ARG, dict(below=NAN)), ("samples 0", ARG, dict(samples=0)), ("samples 4097", ARG, dict(samples=4097)),
                 ("bounces -1", ARG, dict(bounces=-1)), ("bounces 65", ARG, dict(bounces=65)), ("weight 0", ARG, dict(weight=0.0)),
                 ("weight NaN", ARG, dict(weight=NAN)), ("max_history 0.5", ARG, dict(max_history=0.5)), ("max_history NaN", ARG, dict(max_history=NAN)),
                 ("dst == count", ARG, dict(count=d)), ("dst is the sky", ARG, dict(dst=sky.handle)), ("count 0", HANDLE, dict(count=0)),
                 ("dst unknown", HANDLE, dict(dst=gone_h))]
        for what, code, ch in cases:
            assert resample(**ch) == code, what
            unchanged("resample: " + what)
        sh.SetTexture(0, "Result", small)
        assert resample() == ARG                                                     # dst and count are not of the Result texture's size
        unchanged("resample: size of Result")
        sh.SetTexture(0, "Result", result)
        assert resample(below=0.0) == 0 and out.value == 0                           # and a valid call that selects nothing
        out.value = -5
        unchanged("resample: nothing selected")
        for t in (dst, cnt, sky, small, result):
            t.Release()
