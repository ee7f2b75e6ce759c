"""GPU: bloom (include/urt.h urt_bloom, RayTraceMaster.EnableBloom) — every comparison bit for bit against the numpy restatement
(tests/bloom_ref.py): ragged sizes that are odd at every level and cross the 16 x 16 tiles of the levels 0..2, every parameter's corner,
in place, the exposure state read on the device, the pyramid's scratch reused at other sizes, ordering with deferred frames and with the
tone mapping, the error contract against sentinel fills, counters and resources."""
import ctypes as C
import functools

import numpy as np
import pytest

from bloom_ref import FLAG_ONLY, bloom_ref, level_sizes
from tonemap_ref import auto_exposure_ref, tonemap_ref
from unityraytracer_amd import Context, RayTraceMaster, _lib, live_resources, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
SPECIALS = np.array([NAN, INF, -INF, -1.0, -3e38, 0.0, -0.0, 1e-40, -1e-40, 1e-45, 3e38, 65504.0, 70000.0], F)
ALPHA_PAYLOADS = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], U)


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def assert_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    bad = g != r
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[0]}"


def assert_bloomed(got, ref, what):
    """The header's contract: a NaN where the reference holds one (payload unspecified), every other word equal."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: the NaNs are elsewhere"
    assert_bits(np.where(nan, F(0), got), np.where(nan, F(0), ref), what)


@functools.lru_cache(maxsize=None)
def image(w, h, seed=0):
    """Radiance log-uniform over 2^-20 .. 2^12; about 1 % of the colour channels, and the first texels as far as they fit, hold a value
    that is no radiance; alpha holds NaN payloads, -0, infinities and a denormal.  Cached and never written."""
    rng = np.random.default_rng(1000 * w + h + seed)
    px = np.exp2(rng.uniform(-20, 12, (h, w, 4))).astype(F)
    odd = rng.uniform(size=(h, w, 3)) < 0.01
    px[..., :3] = np.where(odd, rng.choice(SPECIALS, (h, w, 3)), px[..., :3])
    flat = px.reshape(-1, 4)
    for k, s in enumerate(SPECIALS[:max(0, min(SPECIALS.size, flat.shape[0] - 2))]):
        flat[k, k % 3] = s
    px[..., 3] = np.resize(ALPHA_PAYLOADS, w * h).view(F).reshape(h, w)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def reference(w, h, exposure=None, seed=0, **params):
    out = bloom_ref(image(w, h, seed), exposure, **params)[0]
    out.setflags(write=False)
    return out


def make_state(ctx, exposure=0.0):
    """A urt_ExposureState on the context's device with the given exposure."""
    import torch
    raw = np.zeros(260, U)
    raw[0] = F(exposure).view(U)
    t = torch.from_numpy(raw.view(np.int32)).to(torch.device("cuda", ctx.device))
    torch.cuda.synchronize(t.device)
    return t


class Pair:
    """src and dst of one size on a context, released at the end."""
    def __init__(self, ctx, w, h, img=None):
        self.src, self.dst = RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
        if img is not None:
            self.src.SetPixels(img)

    def __enter__(self):
        return self.src, self.dst

    def __exit__(self, *exc):
        self.src.Release()
        self.dst.Release()


# ---- 1. every shape and depth --------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (16, 16), (17, 33), (33, 17), (70, 38), (130, 66)]


@pytest.mark.parametrize("levels", [1, 2, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_matches_reference_bit_for_bit(gpu_ctx, shape, levels):
    w, h = shape
    with Pair(gpu_ctx, w, h, image(w, h)) as (src, dst):
        gpu_ctx.bloom(src, dst, levels=levels, threshold=0.5, intensity=0.75)
        assert_bloomed(dst.GetPixels(), reference(w, h, levels=levels, threshold=0.5, intensity=0.75), f"{shape} levels={levels}")
        assert_bits(src.GetPixels(), image(w, h), "src is only read")


def test_the_headers_closed_forms(gpu_ctx):
    w, h = 64, 128
    const = np.full((h, w, 4), 4.0, F)
    img = np.ascontiguousarray(image(w, h)[..., :])
    with Pair(gpu_ctx, w, h, const) as (src, dst):
        gpu_ctx.bloom(src, dst, intensity=1.0, flags=FLAG_ONLY)                   # dst = b
        got = dst.GetPixels()
        assert (got[..., :3] == F(3.0)).all() and (got[..., 3] == F(4.0)).all()   # a constant 4.0 blooms to exactly 3.0
        outs = []
        for flip in (None, 0, 1):                                                 # every level even: mirroring the input mirrors the bloom
            src.SetPixels(img if flip is None else np.ascontiguousarray(np.flip(img, flip)))
            gpu_ctx.bloom(src, dst, intensity=1.0, flags=FLAG_ONLY, levels=5)
            got = dst.GetPixels()[..., :3]
            outs.append(got if flip is None else np.flip(got, flip))
        assert_bits(outs[1], outs[0], "mirrored in y")
        assert_bits(outs[2], outs[0], "mirrored in x")
        assert np.isfinite(outs[0]).all() and (outs[0] > 0).any()


# ---- 2. every parameter's corner -----------------------------------------------------------------------------------------------------
CORNERS = {
    "defaults": {},
    "knee_0": {"soft_knee": 0.0}, "knee_1": {"soft_knee": 1.0},
    "threshold_0": {"threshold": 0.0}, "threshold_0_knee_0": {"threshold": 0.0, "soft_knee": 0.0}, "threshold_max": {"threshold": 65504.0},
    "scatter_0": {"scatter": 0.0}, "scatter_1": {"scatter": 1.0},
    "clamp_small": {"clamp": 0.03125, "threshold": 0.001}, "clamp_tiny": {"clamp": 1e-30, "threshold": 0.0},
    "intensity_large": {"intensity": 3e38}, "only": {"flags": FLAG_ONLY, "intensity": 1.0},
}


@pytest.mark.parametrize("corner", sorted(CORNERS))
def test_parameter_corners(gpu_ctx, corner):
    w, h = 70, 38
    with Pair(gpu_ctx, w, h, image(w, h)) as (src, dst):
        gpu_ctx.bloom(src, dst, **CORNERS[corner])
        assert_bloomed(dst.GetPixels(), reference(w, h, **CORNERS[corner]), corner)


def test_intensity_zero_and_below_threshold_leave_the_image(gpu_ctx):
    """src.c + b.c * 0: the bits of src, except that -0 + 0 is +0 and that a NaN keeps no payload — the header's arithmetic, which the
    reference restates; on an image without those two, dst == src in bits."""
    w, h = 70, 38
    img = image(w, h)
    clean = np.ascontiguousarray(np.where(np.isnan(img) | (bits(img) == 0x80000000), F(0.5), img))
    clean[..., 3] = img[..., 3]
    dim = np.ascontiguousarray(np.exp2(np.random.default_rng(5).uniform(-20, -1.1, (h, w, 4))).astype(F))    # below t - k = 0.5
    with Pair(gpu_ctx, w, h, img) as (src, dst):
        gpu_ctx.bloom(src, dst, intensity=0.0)
        assert_bloomed(dst.GetPixels(), reference(w, h, intensity=0.0), "intensity 0 vs reference")
        src.SetPixels(clean)
        gpu_ctx.bloom(src, dst, intensity=0.0)
        assert_bits(dst.GetPixels(), clean, "intensity 0")
        src.SetPixels(dim)
        gpu_ctx.bloom(src, dst)
        assert_bits(dst.GetPixels(), dim, "below the threshold")
        gpu_ctx.bloom(src, dst, flags=FLAG_ONLY)
        got = dst.GetPixels()
        assert (bits(got[..., :3]) == 0).all() and np.array_equal(bits(got[..., 3]), bits(dim[..., 3]))     # b == 0


def test_nan_and_inf_images_give_a_finite_bloom(gpu_ctx):
    w, h = 33, 17
    with Pair(gpu_ctx, w, h) as (src, dst):
        for v in (NAN, INF, -INF):
            img = np.full((h, w, 4), v, F)
            src.SetPixels(img)
            gpu_ctx.bloom(src, dst, flags=FLAG_ONLY, intensity=1.0, levels=16)
            got = dst.GetPixels()
            assert np.isfinite(got[..., :3]).all()
            assert_bits(got, bloom_ref(img, flags=FLAG_ONLY, intensity=1.0, levels=16)[0], f"all {v}")


# ---- 3. in place, alpha, the state -----------------------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place_and_alpha_is_copied(gpu_ctx):
    w, h = 130, 66
    img = image(w, h)
    with Pair(gpu_ctx, w, h, img) as (src, dst):
        for kw in ({}, {"flags": FLAG_ONLY, "levels": 3}):
            src.SetPixels(img)
            gpu_ctx.bloom(src, dst, **kw)
            out = dst.GetPixels()
            gpu_ctx.bloom(src, src, **kw)
            assert_bits(src.GetPixels(), out, f"in place {kw}")
            assert_bloomed(out, reference(w, h, **kw), f"out of place {kw}")
            assert_bits(out[..., 3], img[..., 3], "alpha")


def test_the_state_is_read_on_the_device(gpu_ctx):
    w, h = 70, 38
    ctx = gpu_ctx
    img = image(w, h)
    with Pair(ctx, w, h, img) as (src, dst):
        state = make_state(ctx)
        ctx.auto_exposure(src, state, key=0.5)
        ctx.bloom(src, dst, state, threshold=2.0, clamp=64.0)                    # no download, no synchronisation in between
        got = dst.GetPixels()
        e = ctx.exposure_state(state)["exposure"]                                 # downloaded afterwards, for the reference
        assert F(e).view(U) == F(auto_exposure_ref(img, key=0.5)["exposure"]).view(U) and e != 1.0
        assert_bloomed(got, reference(w, h, exposure=e, threshold=2.0, clamp=64.0), "metered state")
        plain = reference(w, h, threshold=2.0, clamp=64.0)
        assert not np.array_equal(bits(got), bits(plain))
        for s in (0.0, -0.0, NAN, INF, -INF, -4.0, 2.0 ** -70, 2.0 ** -61, 2.0 ** 61, 1e-40):
            ctx.bloom(src, dst, make_state(ctx, s), threshold=2.0, clamp=64.0)
            assert_bloomed(dst.GetPixels(), plain, f"state exposure {s} is e = 1")
        for s in (2.0 ** -60, 2.0 ** 60, 0.37):
            kw = {"threshold": 65504.0 if s < 1 else 2.0, "clamp": 64.0, "soft_knee": 1.0}
            ctx.bloom(src, dst, make_state(ctx, s), **kw)
            assert_bloomed(dst.GetPixels(), reference(w, h, exposure=s, **kw), f"state exposure {s}")


# ---- 4. the scratch, back-to-back calls, deferred frames ---------------------------------------------------------------------------------
def test_the_pyramid_scratch_is_reused_across_sizes(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        for k, (w, h) in enumerate([(130, 66), (3, 5), (130, 66), (17, 33), (70, 38)]):
            with Pair(ctx, w, h, image(w, h, seed=k % 2)) as (src, dst):
                held = live_resources()["device_bytes"]
                ctx.bloom(src, dst, levels=16, threshold=0.25)
                grown = live_resources()["device_bytes"] - held
                assert grown == (16 * sum(a * b for a, b in level_sizes(w, h, 16)) if k == 0 else 0)    # sum_l w_l * h_l float4, once
                assert_bloomed(dst.GetPixels(), reference(w, h, seed=k % 2, levels=16, threshold=0.25), f"call {k} at {w} x {h}")


def test_two_calls_back_to_back(gpu_ctx):
    w, h = 70, 38
    ctx = gpu_ctx
    with Pair(ctx, w, h, image(w, h)) as (src, dst), Pair(ctx, 33, 17, image(33, 17)) as (src2, dst2):
        ctx.bloom(src, dst, scatter=0.25)
        ctx.bloom(src2, dst2, levels=2)                                           # the same pyramid scratch, no synchronisation in between
        ctx.bloom(dst, dst, threshold=0.125)                                      # and a bloom of the first result, in place
        once = reference(w, h, scatter=0.25)
        assert_bloomed(dst2.GetPixels(), reference(33, 17, levels=2), "second call")
        assert_bloomed(dst.GetPixels(), bloom_ref(once, threshold=0.125)[0], "third call on the first's result")


def test_bloom_sees_deferred_frames_and_an_error_submits_nothing(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
        out = RenderTexture(ctx, 48, 32)
        for _ in range(3):
            m.OnRenderImage()                                                     # deferred: three dispatches and their urt_blit_add into _converged
        bad = _lib.BloomParams(1.0, 0.5, 65504.0, 0.7, 0.2, 0, 0)                 # levels 0
        assert ctx.lib.urt_bloom(ctx._h, m._converged.handle, out.handle, C.byref(bad), None) == 1
        ctx.bloom(m._converged, out, threshold=0.125)
        got = out.GetPixels()
        assert ctx.launch_info()["n_frames"] == 3                                 # one deferred batch when the valid call came
        conv = m._converged.GetPixels()
        ref, b = bloom_ref(conv, threshold=0.125)
        assert_bloomed(got, ref, "after deferred frames")
        assert (b > 0).any() and (conv[..., :3] > 0).any()
        out.Release()
        m.OnDisable()


# ---- 5. RayTraceMaster ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metered", [False, True], ids=["plain", "auto_exposure"])
def test_master_bloom_then_tonemap(gpu_ctx, metered):
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
        for _ in range(3):
            m.OnRenderImage()
        if metered:
            m.EnableAutoExposure(key=0.25)
        before = m.ToneMap().GetPixels()                                          # today's bytes
        conv = m._converged.GetPixels()
        e = auto_exposure_ref(conv, key=0.25)["exposure"] if metered else None
        assert_bits(before, tonemap_ref(conv, state_exposure=e), "without bloom")
        held = live_resources()
        m.EnableBloom(threshold=0.25, scatter=0.5, intensity=0.5)
        assert live_resources() == held and m._tonemapped is not None           # EnableBloom creates nothing
        out = m.ToneMap()
        assert out is m._tonemapped
        bloomed, b = bloom_ref(conv, e, threshold=0.25, scatter=0.5, intensity=0.5)
        assert (b > 0).any()
        assert_bits(out.GetPixels(), tonemap_ref(bloomed, state_exposure=e), "bloom, then tone map")
        assert not np.array_equal(bits(out.GetPixels()), bits(before))
        assert_bits(m._converged.GetPixels(), conv, "_converged is never modified")
        dest = RenderTexture(ctx, 48, 32)
        assert m.ToneMap(destination=dest, operator="reinhard") is dest
        assert_bits(dest.GetPixels(), tonemap_ref(bloomed, op=1, state_exposure=e), "into a destination")
        m.DisableBloom()
        assert_bits(m.ToneMap().GetPixels(), before, "DisableBloom restores today's bytes")
        with pytest.raises(ValueError):
            m.EnableBloom(levels=17)
        assert m._bloom is None
        dest.Release()
        m.OnDisable()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
ARG, HANDLE = 1, 2
BLOOM_OK = {"threshold": 1.0, "soft_knee": 0.5, "clamp": 65504.0, "scatter": 0.7, "intensity": 0.2, "levels": 6, "flags": 0}
# name -> (expected code, call changes: src / dst / state, params changes)
BLOOM_ERRORS = {
    "threshold_negative": (ARG, {}, {"threshold": -1e-6}), "threshold_large": (ARG, {}, {"threshold": 65536.0}),
    "threshold_nan": (ARG, {}, {"threshold": NAN}), "threshold_inf": (ARG, {}, {"threshold": INF}),
    "knee_negative": (ARG, {}, {"soft_knee": -0.5}), "knee_above_1": (ARG, {}, {"soft_knee": 1.5}), "knee_nan": (ARG, {}, {"soft_knee": NAN}),
    "scatter_negative": (ARG, {}, {"scatter": -0.5}), "scatter_above_1": (ARG, {}, {"scatter": 2.0}), "scatter_nan": (ARG, {}, {"scatter": NAN}),
    "clamp_zero": (ARG, {}, {"clamp": 0.0}), "clamp_negative": (ARG, {}, {"clamp": -1.0}), "clamp_large": (ARG, {}, {"clamp": 65536.0}),
    "clamp_nan": (ARG, {}, {"clamp": NAN}),
    "intensity_negative": (ARG, {}, {"intensity": -0.2}), "intensity_nan": (ARG, {}, {"intensity": NAN}), "intensity_inf": (ARG, {}, {"intensity": INF}),
    "levels_zero": (ARG, {}, {"levels": 0}), "levels_17": (ARG, {}, {"levels": 17}), "levels_negative": (ARG, {}, {"levels": -3}),
    "flags_unknown_bit": (ARG, {}, {"flags": 2}), "flags_high_bit": (ARG, {}, {"flags": -2147483648}),
    "state_misaligned_4": (ARG, {"state": "+4"}, {}), "state_misaligned_8": (ARG, {"state": "+8"}, {}),
    "dst_size": (ARG, {"dst": "odd"}, {}), "src_size": (ARG, {"src": "odd"}, {}),
    "dst_is_sky": (ARG, {"dst": "sky"}, {}),
    "src_zero": (HANDLE, {"src": 0}, {}), "dst_zero": (HANDLE, {"dst": 0}, {}), "src_unknown": (HANDLE, {"src": 987654}, {}),
    "dst_unknown": (HANDLE, {"dst": 987654}, {}), "dst_released": (HANDLE, {"dst": "gone"}, {}),
}
SENTINEL = 0xC0FFEE42


@pytest.fixture(scope="module")
def error_rig(gpu_ctx):
    W, H = 16, 8
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        tex = {n: RenderTexture(ctx, W, H) for n in ("src", "dst", "sky")}
        tex["odd"] = RenderTexture(ctx, 5, 5)
        snap = {}
        for n, t in tex.items():
            snap[n] = rng.uniform(0.1, 4, (t.height, t.width, 4)).astype(F)
            t.SetPixels(snap[n])
        import torch
        state = torch.from_numpy(np.full(260, SENTINEL, U).view(np.int32)).to(torch.device("cuda", ctx.device))
        torch.cuda.synchronize(state.device)
        gone = RenderTexture(ctx, W, H)
        gone_h = gone.handle
        gone.Release()
        sh = ComputeShader(ctx)
        sh.SetTexture(0, "_SkyboxTexture", tex["sky"])
        for t in tex.values():
            t.GetPixels()                                                        # (whatever a readback keeps is held from here on)
        yield ctx, tex, snap, gone_h, state, live_resources()["device_bytes"]
        sh.SetTexture(0, "_SkyboxTexture", None)
        for t in tex.values():
            t.Release()


def error_call(rig, changes, params):
    ctx, tex, _, gone_h, state, _ = rig
    d = {"src": tex["src"].handle, "dst": tex["dst"].handle, "state": state.data_ptr()}
    for n, v in changes.items():
        d[n] = gone_h if v == "gone" else state.data_ptr() + int(v) if isinstance(v, str) and v.startswith("+") else tex[v].handle if isinstance(v, str) else v
    p = None if params == "null" else C.byref(_lib.BloomParams(*({**BLOOM_OK, **params}[k] for k in BLOOM_OK)))
    return ctx.lib.urt_bloom(ctx._h, d["src"], d["dst"], p, C.c_void_p(d["state"]))


@pytest.mark.parametrize("case", sorted(BLOOM_ERRORS))
def test_errors_write_nothing_and_allocate_nothing(error_rig, case):
    code, changes, params = BLOOM_ERRORS[case]
    ctx, tex, snap, _, state, held = error_rig
    assert error_call(error_rig, changes, params) == code
    ctx.synchronize()
    for n, t in tex.items():
        assert t.GetPixels().tobytes() == snap[n].tobytes(), n
    assert (state.cpu().numpy().view(U) == SENTINEL).all()
    assert live_resources()["device_bytes"] == held                              # no pyramid: the checks come before the scratch


def test_valid_calls_after_the_errors_do_write(error_rig):
    ctx, tex, snap, _, state, held = error_rig
    assert ctx.lib.urt_bloom(None, 1, 2, None, None) == ARG
    assert error_call(error_rig, {}, "null") == 0                                # params == NULL: the defaults; the sentinel exposure is negative: e = 1
    assert_bits(tex["dst"].GetPixels(), bloom_ref(snap["src"])[0], "defaults")
    assert live_resources()["device_bytes"] - held == 16 * sum(a * b for a, b in level_sizes(16, 8))
    assert error_call(error_rig, {"state": 0}, {"levels": 16, "flags": 1}) == 0  # no state
    assert_bits(tex["dst"].GetPixels(), bloom_ref(snap["src"], levels=16, flags=1)[0], "no state")
    assert error_call(error_rig, {"src": "sky"}, {"threshold": 0.5}) == 0        # the sky may be read
    assert_bits(tex["dst"].GetPixels(), bloom_ref(snap["sky"], threshold=0.5)[0], "from the sky")
    for n in ("src", "sky", "odd"):
        assert tex[n].GetPixels().tobytes() == snap[n].tobytes(), n              # the inputs are only read
    assert (state.cpu().numpy().view(U) == SENTINEL).all()                       # and so is the state


# ---- 7. counters and resources ------------------------------------------------------------------------------------------------------------
def test_counters_are_left_alone_and_everything_is_given_back(gpu_ctx):
    def run():
        with Context(gpu_ctx.device) as ctx:
            ctx.set_option("count_stats", 1)
            m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
            m.EnableAutoExposure()
            m.EnableBloom()
            m.OnRenderImage()
            ctx.synchronize()
            c0 = ctx.counters()
            m.ToneMap()
            ctx.bloom(m._converged, m._tonemapped, m._exposureState, levels=16)
            ctx.synchronize()
            assert ctx.counters() == c0
            m.OnDisable()
    run()
    before = live_resources()
    run()
    assert live_resources() == before
