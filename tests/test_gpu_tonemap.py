"""GPU: auto-exposure and tone mapping (include/urt.h urt_auto_exposure / urt_tonemap, RayTraceMaster.ToneMap) — every comparison bit for
bit against the numpy restatement (tests/tonemap_ref.py): the histogram, the resolved exposure and the three operators at ragged sizes
and at one size the capped grid has to stride over, the state carried from call to call, ordering with deferred frames and with the
formatted readback, the error contract against sentinel fills, counters and resources."""
import ctypes as C

import numpy as np
import pytest

from tonemap_ref import (ACES, BINS, F, FRESH, LINEAR, REINHARD, U, auto_exposure_ref, luminance, luminance_bin, texel_with_luminance,
                         tonemap_ref)
from unityraytracer_amd import Context, RayTraceMaster, UrtError, _lib, host_io, live_resources, scenes
from unityraytracer_amd.unity_api import EXPOSURE_MAX_BLOCKS, ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

OPS = {"linear": LINEAR, "reinhard": REINHARD, "aces": ACES}
NAN, INF = float("nan"), float("inf")
SPECIALS = np.array([0.0, -0.0, -1.0, -1e-40, NAN, INF, -INF, 1e-40, 1e-45, 3e38, 65504.0, 70000.0], F)


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def assert_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    bad = g != r
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[0]}"


def assert_state(got, ref, what):
    assert np.array_equal(got["hist"], ref["hist"]), f"{what}: hist differs in bins {np.nonzero(got['hist'] != ref['hist'])[0][:8]}"
    assert (got["counted"], got["skipped"]) == (ref["counted"], ref["skipped"]), what
    assert F(got["target"]).view(U) == F(ref["target"]).view(U), (what, got["target"], ref["target"])
    assert F(got["exposure"]).view(U) == F(ref["exposure"]).view(U), (what, got["exposure"], ref["exposure"])


def make_state(ctx, s=FRESH, fill=None):
    """A urt_ExposureState on the context's device holding s (or `fill` in every word)."""
    import torch
    raw = np.zeros(4 + BINS, U) if fill is None else np.full(4 + BINS, fill, U)
    if fill is None:
        raw[0], raw[1] = F(s["exposure"]).view(U), F(s["target"]).view(U)
        raw[2], raw[3], raw[4:] = s["counted"], s["skipped"], s["hist"]
    t = torch.from_numpy(raw.view(np.int32)).to(torch.device("cuda", ctx.device))
    torch.cuda.synchronize(t.device)
    return t


def special_texels():
    """Every special value in every channel position of an otherwise ordinary texel."""
    px = np.tile(np.array([0.25, 0.5, 0.75, 1.0], F), (SPECIALS.size * 4, 1))
    for k, s in enumerate(SPECIALS):
        for c in range(4):
            px[4 * k + c, c] = s
    return px


def edge_texels():
    """Luminances at the first float of every bin and one ulp below it."""
    return np.stack([texel_with_luminance(((380 + k) << 21) - d) for k in range(1, BINS) for d in (0, 1)])


def image(w, h, content, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    n = w * h
    if content == "constant":
        px = np.tile(np.array([0.5, 0.5, 0.5, 1.0], F), (n, 1))                     # every texel in one bin
    else:                                                                          # log-uniform over 2^-40 .. 2^40: both clamps
        stops = 4 if content == "midrange" else 40                                 # ("midrange": targets inside [min_exposure, max_exposure])
        px = np.exp2(rng.uniform(-stops, stops, (n, 4))).astype(F)
        px[:, 3] = rng.uniform(0, 1, n).astype(F)
        if content == "mixed":                                                     # the specials and the bin edges first, as far as they fit
            head = np.concatenate([special_texels(), edge_texels()])[:n]
            px[:head.shape[0]] = head
    return px.reshape(h, w, 4)


def count_image(w, h, seed=0):
    """A count texture with zeros, negatives, NaN, denormals and ordinary counts in .x; the other channels are not read."""
    rng = np.random.default_rng(77 * w + h + seed)
    c = rng.uniform(-3, 3, (h, w, 4)).astype(F)
    x = rng.choice(np.array([0.0, -0.0, -2.0, NAN, 1e-45, 1.0, 7.0, INF, -INF], F), (h, w))
    c[..., 0] = x
    return c


SIZES = [(1, 1), (63, 1), (64, 1), (65, 3), (257, 5)]                                # ragged wave and block tails
LARGE = (1920, 1080)


# ---- 1. the histogram, the resolve and the operators at every size ---------------------------------------------------------------------
@pytest.mark.parametrize("content", ["mixed", "constant", "loguniform"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_small_images_match_reference_bit_for_bit(gpu_ctx, size, content):
    w, h = size
    ctx = gpu_ctx
    img, cnt = image(w, h, content), count_image(w, h)
    src, count, dst = RenderTexture(ctx, w, h), RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
    try:
        src.SetPixels(img)
        count.SetPixels(cnt)
        for with_count in (False, True):
            for params in ({"low_permille": 0, "high_permille": 1000}, {"key": 0.5, "min_exposure": 0.25, "max_exposure": 2.0},
                           {"low_permille": 499, "high_permille": 501}, {}):
                state = make_state(ctx)
                ctx.auto_exposure(src, state, count if with_count else None, **params)
                ref = auto_exposure_ref(img, cnt if with_count else None, **params)
                got = ctx.exposure_state(state)
                assert_state(got, ref, f"{size} {content} count={with_count} {params}")
                assert got["counted"] + got["skipped"] == w * h
        # the operators, with the state of the last metering and without one, into dst and in place
        for name, op in OPS.items():
            for st in (None, state):
                for white, exposure in ((4.0, 1.0), (0.01, 3.0), (65504.0, 0.125)):
                    kw = {"op": name, "white": white, "exposure": exposure}
                    ref_img = tonemap_ref(img, exposure, white, op, state_exposure=None if st is None else ref["exposure"])
                    ctx.tonemap(src, dst, st, **kw)
                    assert_bits(dst.GetPixels(), ref_img, f"{size} {content} {kw} state={st is not None}")
                    assert_bits(src.GetPixels(), img, "src is only read")
                    ctx.tonemap(src, src, st, **kw)
                    assert_bits(src.GetPixels(), ref_img, f"{size} {content} {kw} state={st is not None} in place")
                    src.SetPixels(img)
    finally:
        for t in (src, count, dst):
            t.Release()


@pytest.mark.parametrize("content", ["mixed", "constant"])
def test_an_image_the_capped_grid_strides_over(gpu_ctx, content):
    """1920 x 1080 = 2 073 600 texels: more than twice (7.9 times) the 1024 x 256 = 262 144 lanes the histogram launches at most
    (csrc/tonemap.h kExposureMaxBlocks), so every lane takes a full unrolled trip of four texels and a second, ragged one."""
    w, h = LARGE
    assert w * h > 2 * 256 * EXPOSURE_MAX_BLOCKS and (w * h) % (256 * EXPOSURE_MAX_BLOCKS) != 0
    ctx = gpu_ctx
    img, cnt = image(w, h, content), count_image(w, h)
    src, count, dst = RenderTexture(ctx, w, h), RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
    try:
        src.SetPixels(img)
        count.SetPixels(cnt)
        state = make_state(ctx)
        ctx.auto_exposure(src, state, count)
        assert_state(ctx.exposure_state(state), auto_exposure_ref(img, cnt), f"{content} with count")
        ctx.auto_exposure(src, state)                                              # overwrites hist, counted and skipped
        ref = auto_exposure_ref(img)
        got = ctx.exposure_state(state)
        assert_state(got, ref, content)
        if content == "constant":
            assert got["hist"][luminance_bin(luminance(img[0, 0]))[0]] == w * h and got["skipped"] == 0
        ctx.tonemap(src, dst, state)
        ref_img = tonemap_ref(img, state_exposure=ref["exposure"])
        assert_bits(dst.GetPixels(), ref_img, content)
        ctx.tonemap(src, src, state)
        assert_bits(src.GetPixels(), ref_img, content + " in place")
    finally:
        for t in (src, count, dst):
            t.Release()


# ---- 2. the state from call to call -----------------------------------------------------------------------------------------------------
def test_state_snaps_then_follows_and_survives_an_empty_window(gpu_ctx):
    w, h = 65, 3
    ctx = gpu_ctx
    a, b = image(w, h, "midrange", 1), image(w, h, "midrange", 2) * F(1.0 / 16.0)
    nothing = np.zeros((h, w, 4), F)
    nothing[..., 0] = NAN
    src = RenderTexture(ctx, w, h)
    try:
        state = make_state(ctx)
        src.SetPixels(a)
        ctx.auto_exposure(src, state, rate=0.25)                                   # a fresh state snaps whatever the rate
        s1 = ctx.exposure_state(state)
        r1 = auto_exposure_ref(a, rate=0.25)
        assert_state(s1, r1, "first call")
        assert s1["exposure"] == s1["target"] > 0
        src.SetPixels(b)
        ctx.auto_exposure(src, state, rate=0.25)                                   # a quarter of the way
        s2 = ctx.exposure_state(state)
        r2 = auto_exposure_ref(b, state=r1, rate=0.25)
        assert_state(s2, r2, "second call")
        assert F(s2["exposure"]) == F(s1["exposure"]) + (F(s2["target"]) - F(s1["exposure"])) * F(0.25)
        assert s2["target"] != s1["target"] and s2["exposure"] not in (s1["exposure"], s2["target"])
        src.SetPixels(nothing)
        ctx.auto_exposure(src, state, rate=0.25)                                   # all skipped: M == 0
        s3 = ctx.exposure_state(state)
        assert_state(s3, auto_exposure_ref(nothing, state=r2, rate=0.25), "empty window")
        assert (s3["exposure"], s3["target"], s3["counted"], s3["skipped"]) == (s2["exposure"], s2["target"], 0, w * h)
        assert not s3["hist"].any()
        ctx.auto_exposure(src, state, low_permille=0, high_permille=1)             # counted texels, but a window that floors to nothing
        src.SetPixels(b)
        ctx.auto_exposure(src, state, low_permille=0, high_permille=1)
        s4 = ctx.exposure_state(state)
        assert (s4["exposure"], s4["target"]) == (s2["exposure"], s2["target"]) and s4["counted"] == w * h
        ctx.auto_exposure(src, state, rate=1.0)                                    # rate >= 1 snaps
        s5 = ctx.exposure_state(state)
        assert s5["exposure"] == s5["target"] == s2["target"]
    finally:
        src.Release()


@pytest.mark.parametrize("op", sorted(OPS))
def test_an_unusable_state_exposure_falls_back_and_alpha_is_copied(gpu_ctx, op):
    w, h = 65, 3
    ctx = gpu_ctx
    img = image(w, h, "mixed")
    payloads = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], U)
    img[..., 3] = np.resize(payloads, w * h).view(F).reshape(h, w)               # alpha: NaN payloads, -0, infinities, a denormal
    src, dst = RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
    try:
        src.SetPixels(img)
        plain = tonemap_ref(img, 0.5, 4.0, OPS[op])
        for s in (0.0, -0.0, -2.0, NAN, INF, -INF):
            state = make_state(ctx, {**FRESH, "exposure": s})
            ctx.tonemap(src, dst, state, op=op, exposure=0.5)
            assert_bits(dst.GetPixels(), plain, f"{op} state exposure {s}")
        state = make_state(ctx, {**FRESH, "exposure": 1e-40})                      # a denormal is finite and > 0: used
        ctx.tonemap(src, dst, state, op=op, exposure=0.5)
        assert_bits(dst.GetPixels(), tonemap_ref(img, 0.5, 4.0, OPS[op], state_exposure=1e-40), f"{op} denormal state exposure")
        assert_bits(dst.GetPixels()[..., 3], img[..., 3], "alpha")
    finally:
        src.Release()
        dst.Release()


# ---- 3. observers of deferred frames ---------------------------------------------------------------------------------------------------
def deferred_run(device, synchronise):
    with Context(device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
        out = RenderTexture(ctx, 48, 32)
        state = make_state(ctx)
        for _ in range(3):
            m.OnRenderImage()                                                # deferred: three dispatches and their urt_blit_add into _converged
            if synchronise:
                ctx.synchronize()
        ctx.auto_exposure(m._converged, state)
        if synchronise:
            ctx.synchronize()
        ctx.tonemap(m._converged, out, state)
        if synchronise:
            ctx.synchronize()
        res = (out.GetPixels(), ctx.exposure_state(state), m._converged.GetPixels(), ctx.launch_info()["n_frames"])
        out.Release()
        m.OnDisable()
    return res


def test_metering_and_tone_mapping_see_deferred_frames(gpu_ctx):
    a = deferred_run(gpu_ctx.device, False)
    b = deferred_run(gpu_ctx.device, True)
    assert a[3] == 3, a[3]                                                   # the frames were one deferred batch when urt_auto_exposure came
    assert_bits(a[2], b[2], "converged")
    assert_state(a[1], b[1], "state")
    assert_bits(a[0], b[0], "tone-mapped")
    ref = auto_exposure_ref(a[2])
    assert_state(a[1], ref, "state vs reference")
    assert_bits(a[0], tonemap_ref(a[2], state_exposure=ref["exposure"]), "tone-mapped vs reference")
    assert a[1]["counted"] > 0.9 * 48 * 32


@pytest.mark.parametrize("temporal", [False, True], ids=["mean", "temporal"])
def test_master_tonemap_then_formatted_readback(gpu_ctx, temporal):
    with Context(gpu_ctx.device) as ctx:
        def master():
            m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
            if temporal:
                m.EnableTemporalAccumulation()
            for _ in range(3):
                m.OnRenderImage()
            return m
        twin = master()                                                      # the same frames without any ToneMap
        twin.OnRenderImage()
        twin_frame, twin_conv = twin._target.GetPixels(), twin._converged.GetPixels()
        twin.OnDisable()
        m = master()
        with pytest.raises(ValueError):
            m.ToneMap(destination=m._converged)
        # without auto-exposure: params' exposure alone
        out = m.ToneMap(operator="reinhard", exposure=2.0, white=3.0)
        ticket = out.ReadBegin("RGBA8_SRGB")                                 # no flush, no synchronise in between
        got8 = out.ReadEnd(ticket)
        conv = m._converged.GetPixels()
        assert out is m._tonemapped and (out.width, out.height) == (48, 32)
        assert np.array_equal(got8, host_io.encode_srgb8(tonemap_ref(conv, 2.0, 3.0, REINHARD)))
        # with auto-exposure: metered on the device, never downloaded
        m.EnableAutoExposure(key=0.25, low_permille=50)
        dest = RenderTexture(ctx, 48, 32)
        assert m.ToneMap(destination=dest) is dest
        ticket = dest.ReadBegin("RGBA8_SRGB")
        got8 = dest.ReadEnd(ticket)
        ref = auto_exposure_ref(conv, m._tcount.GetPixels() if temporal else None, key=0.25, low_permille=50)
        assert_state(ctx.exposure_state(m._exposureState), ref, "ToneMap's metering")
        ref_img = tonemap_ref(conv, state_exposure=ref["exposure"])
        assert np.array_equal(got8, host_io.encode_srgb8(ref_img))
        assert_bits(dest.GetPixels(), ref_img, "ToneMap")
        assert 0 < ref["exposure"] and len(np.unique(got8[..., :3])) > 32     # an image, not a clipped or black frame
        assert_bits(m._converged.GetPixels(), conv, "_converged is never modified")
        m.DisableAutoExposure()
        assert m._exposure is None and m._exposureState is None
        assert_bits(m.ToneMap(operator="linear").GetPixels(), tonemap_ref(conv, op=LINEAR), "after DisableAutoExposure")
        # the next frame is what it would have been
        m.OnRenderImage()
        assert_bits(m._target.GetPixels(), twin_frame, "the frame after ToneMap")
        assert_bits(m._converged.GetPixels(), twin_conv, "the accumulation after ToneMap")
        dest.Release()
        m.OnDisable()
        assert m._tonemapped is None


def test_tonemap_needs_a_frame(gpu_ctx):
    m = RayTraceMaster(gpu_ctx, scenes.mixed_test_scene(16, 8))
    with pytest.raises(UrtError):
        m.ToneMap()
    m.OnDisable()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
ARG, HANDLE = 1, 2
EXPOSURE_OK = {"key": 0.18, "min_exposure": 1.0 / 64.0, "max_exposure": 64.0, "rate": 1.0, "low_permille": 100, "high_permille": 950}
TONEMAP_OK = {"exposure": 1.0, "white": 4.0, "op": 2, "flags": 0}
# name -> (expected code, call changes: src / count / dst / state, params changes)
EXPOSURE_ERRORS = {
    "state_null": (ARG, {"state": 0}, {}),
    "state_misaligned_4": (ARG, {"state": "+4"}, {}),
    "state_misaligned_8": (ARG, {"state": "+8"}, {}),
    "key_nan": (ARG, {}, {"key": NAN}), "key_zero": (ARG, {}, {"key": 0.0}), "key_negative": (ARG, {}, {"key": -0.18}),
    "key_inf": (ARG, {}, {"key": INF}),
    "min_zero": (ARG, {}, {"min_exposure": 0.0}), "min_nan": (ARG, {}, {"min_exposure": NAN}), "min_inf": (ARG, {}, {"min_exposure": INF}),
    "max_inf": (ARG, {}, {"max_exposure": INF}), "max_nan": (ARG, {}, {"max_exposure": NAN}), "max_negative": (ARG, {}, {"max_exposure": -1.0}),
    "min_above_max": (ARG, {}, {"min_exposure": 2.0, "max_exposure": 1.0}),
    "rate_nan": (ARG, {}, {"rate": NAN}), "rate_zero": (ARG, {}, {"rate": 0.0}), "rate_negative": (ARG, {}, {"rate": -0.5}),
    "low_negative": (ARG, {}, {"low_permille": -1}), "low_equals_high": (ARG, {}, {"low_permille": 500, "high_permille": 500}),
    "low_above_high": (ARG, {}, {"low_permille": 600, "high_permille": 500}), "high_above_1000": (ARG, {}, {"high_permille": 1001}),
    "count_size": (ARG, {"count": "odd"}, {}),
    "too_many_texels": (ARG, {"src": "huge", "count": 0}, {}),
    "src_zero": (HANDLE, {"src": 0}, {}), "src_unknown": (HANDLE, {"src": 987654}, {}), "src_released": (HANDLE, {"src": "gone"}, {}),
    "count_unknown": (HANDLE, {"count": 987654}, {}),
}
TONEMAP_ERRORS = {
    "op_unknown": (ARG, {}, {"op": 3}), "op_negative": (ARG, {}, {"op": -1}),
    "flags_nonzero": (ARG, {}, {"flags": 1}),
    "exposure_nan": (ARG, {}, {"exposure": NAN}), "exposure_zero": (ARG, {}, {"exposure": 0.0}), "exposure_negative": (ARG, {}, {"exposure": -1.0}),
    "exposure_inf": (ARG, {}, {"exposure": INF}),
    "white_small": (ARG, {}, {"white": 0.009}), "white_large": (ARG, {}, {"white": 65536.0}), "white_nan": (ARG, {}, {"white": NAN}),
    "state_misaligned_4": (ARG, {"state": "+4"}, {}), "state_misaligned_8": (ARG, {"state": "+8"}, {}),
    "dst_size": (ARG, {"dst": "odd"}, {}), "src_size": (ARG, {"src": "odd"}, {}),
    "dst_is_sky": (ARG, {"dst": "sky"}, {}),
    "src_zero": (HANDLE, {"src": 0}, {}), "dst_zero": (HANDLE, {"dst": 0}, {}), "dst_unknown": (HANDLE, {"dst": 987654}, {}),
    "dst_released": (HANDLE, {"dst": "gone"}, {}),
}
SENTINEL = 0xC0FFEE42


@pytest.fixture(scope="module")
def error_rig(gpu_ctx):
    import torch
    W, H = 16, 8
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        tex = {n: RenderTexture(ctx, W, H) for n in ("src", "count", "dst", "sky")}
        tex["odd"] = RenderTexture(ctx, 5, 5)
        snap = {}
        for n, t in tex.items():
            snap[n] = rng.uniform(0.1, 2, (t.height, t.width, 4)).astype(F)
            t.SetPixels(snap[n])
        state = make_state(ctx, fill=SENTINEL)
        small = torch.zeros(64, dtype=torch.int32, device=state.device)
        torch.cuda.synchronize(state.device)
        tex["huge"] = RenderTexture(ctx, 65536, 32768, external_ptr=small.data_ptr())   # 2^31 texels on paper: refused before it is touched
        gone = RenderTexture(ctx, W, H)
        gone_h = gone.handle
        gone.Release()
        sh = ComputeShader(ctx)
        sh.SetTexture(0, "_SkyboxTexture", tex["sky"])
        yield ctx, tex, snap, gone_h, state
        sh.SetTexture(0, "_SkyboxTexture", None)
        for t in tex.values():
            t.Release()


def error_call(rig, which, changes, params):
    ctx, tex, _, gone_h, state = rig
    d = {"src": tex["src"].handle, "count": tex["count"].handle, "dst": tex["dst"].handle, "state": state.data_ptr()}
    for n, v in changes.items():
        d[n] = gone_h if v == "gone" else state.data_ptr() + int(v) if isinstance(v, str) and v.startswith("+") else tex[v].handle if isinstance(v, str) else v
    sp = C.c_void_p(d["state"])
    if which == "exposure":
        p = None if params == "null" else C.byref(_lib.ExposureParams(*({**EXPOSURE_OK, **params}[k] for k in EXPOSURE_OK)))
        return ctx.lib.urt_auto_exposure(ctx._h, d["src"], d["count"], p, sp)
    p = None if params == "null" else C.byref(_lib.TonemapParams(*({**TONEMAP_OK, **params}[k] for k in TONEMAP_OK)))
    return ctx.lib.urt_tonemap(ctx._h, d["src"], d["dst"], p, sp)


def assert_untouched(rig):
    ctx, tex, snap, _, state = rig
    ctx.synchronize()
    for n, t in tex.items():
        if n != "huge":
            assert t.GetPixels().tobytes() == snap[n].tobytes(), n
    assert (state.cpu().numpy().view(U) == SENTINEL).all()


@pytest.mark.parametrize("case", sorted(EXPOSURE_ERRORS))
def test_auto_exposure_errors_write_nothing(error_rig, case):
    code, changes, params = EXPOSURE_ERRORS[case]
    assert error_call(error_rig, "exposure", changes, params) == code
    assert_untouched(error_rig)


@pytest.mark.parametrize("case", sorted(TONEMAP_ERRORS))
def test_tonemap_errors_write_nothing(error_rig, case):
    code, changes, params = TONEMAP_ERRORS[case]
    assert error_call(error_rig, "tonemap", changes, params) == code
    assert_untouched(error_rig)


def test_valid_calls_after_the_errors_do_write(error_rig):
    ctx, tex, snap, _, state = error_rig
    assert ctx.lib.urt_auto_exposure(None, 1, 0, None, None) == ARG and ctx.lib.urt_tonemap(None, 1, 2, None, None) == ARG
    try:
        assert error_call(error_rig, "exposure", {}, "null") == 0                # params == NULL: the defaults; the sentinel exposure is negative
        by_null = ctx.exposure_state(state)
        assert_state(by_null, auto_exposure_ref(snap["src"], snap["count"]), "defaults")
        assert error_call(error_rig, "exposure", {"count": 0}, {}) == 0          # no count texture
        assert_state(ctx.exposure_state(state), auto_exposure_ref(snap["src"], state=by_null), "no count")
        assert error_call(error_rig, "tonemap", {}, "null") == 0
        assert_bits(tex["dst"].GetPixels(), tonemap_ref(snap["src"], state_exposure=by_null["exposure"]), "defaults")
        assert error_call(error_rig, "tonemap", {"state": 0}, {}) == 0           # no state
        assert_bits(tex["dst"].GetPixels(), tonemap_ref(snap["src"]), "no state")
        assert error_call(error_rig, "tonemap", {"src": "sky", "dst": "dst"}, {"op": 0}) == 0   # the sky may be read
        assert_bits(tex["dst"].GetPixels(), tonemap_ref(snap["sky"], op=LINEAR, state_exposure=by_null["exposure"]), "from the sky")
        for n in ("src", "count", "sky", "odd"):
            assert tex[n].GetPixels().tobytes() == snap[n].tobytes(), n          # the inputs are only read
    finally:
        tex["dst"].SetPixels(snap["dst"])
        state.fill_(int(np.array([SENTINEL], U).view(np.int32)[0]))
        import torch
        torch.cuda.synchronize(state.device)


def test_wrappers_refuse_a_state_that_is_not_device_memory(gpu_ctx):
    import torch
    ctx = gpu_ctx
    src = RenderTexture(ctx, 4, 4)
    try:
        good = torch.zeros(600, dtype=torch.int32, device=torch.device("cuda", ctx.device))
        ctx.auto_exposure(src, good[4:])                                         # 16 bytes in: aligned, long enough
        for bad, exc in ((np.zeros(260, np.int32), TypeError), (torch.zeros(260, dtype=torch.int32), ValueError),
                         (good[:259], ValueError), (good[1:], ValueError), (good[::2], ValueError), (None, TypeError)):
            with pytest.raises(exc):
                ctx.auto_exposure(src, bad)
            if bad is not None:
                with pytest.raises(exc):
                    ctx.tonemap(src, src, bad)
            with pytest.raises(exc):
                ctx.exposure_state(bad)
    finally:
        src.Release()


# ---- 5. counters and resources ------------------------------------------------------------------------------------------------------------
def test_counters_are_left_alone_and_everything_is_given_back(gpu_ctx):
    def run():
        with Context(gpu_ctx.device) as ctx:
            ctx.set_option("count_stats", 1)
            m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
            m.EnableAutoExposure()
            m.OnRenderImage()
            ctx.synchronize()
            c0 = ctx.counters()
            m.ToneMap()
            ctx.auto_exposure(m._converged, m._exposureState, rate=0.5)
            ctx.tonemap(m._converged, m._tonemapped, m._exposureState, op="reinhard")
            ctx.synchronize()
            assert ctx.counters() == c0
            m.OnDisable()
    run()
    before = live_resources()
    run()
    assert live_resources() == before                                        # a destroyed context leaves the tally where it was
