"""GPU: guide-driven upsampling (include/urt.h urt_upsample, RayTraceMaster.Upscale) — bit for bit against the numpy restatement
(tests/upsample_ref.py) on synthetic guides at every size class and on a real scene, ordering with deferred frames, the error contract,
the master's opt-in method with and without hole filling, and the quality relation DESIGN.md §22 records."""
import ctypes as C

import numpy as np
import pytest

from upsample_ref import SKY_FROM_ALBEDO, WIDE_FALLBACK, bilinear_resize_ref, synthetic_case, upsample_ref
from unityraytracer_amd import Context, RayTraceMaster, UrtError, _lib, live_resources, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

F = np.float32
LOW = ("low_color", "low_count", "low_hit", "low_normal", "low_id")
FULL_IN = ("hit", "normal", "id", "albedo")
NAMES = LOW + FULL_IN + ("color", "count")


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, ref, what):
    g, r = u32(got), u32(ref)
    bad = g != r
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} texels differ, first at {np.argwhere(bad)[0]}: {got[tuple(np.argwhere(bad)[0][:2])]} " \
                          f"vs {ref[tuple(np.argwhere(bad)[0][:2])]}"


def ref_of(c, low_count, albedo, flags, **kw):
    return upsample_ref(c["low_color"], c["low_hit"], c["low_normal"], c["low_id"], c["hit"], c["normal"], c["id"],
                        low_count=c["low_count"] if low_count else None, albedo=c["albedo"] if albedo else None, flags=flags, **kw)


# ---- 1. synthetic guides, every option, outputs in external memory with a guard band ---------------------------------------------------
PAIRS = [(1, 1, 1, 1), (1, 1, 5, 3), (3, 2, 7, 5), (5, 3, 10, 6), (8, 8, 17, 17), (13, 9, 37, 33), (16, 16, 16, 16), (20, 12, 10, 6)]
GUARD = 3                                                                    # rows of the output's width before and after it


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_synthetic_guides_match_reference_bit_for_bit(gpu_ctx, pair):
    import torch
    w, h, W, H = pair
    ctx = gpu_ctx
    dev = torch.device("cuda", ctx.device)
    c = synthetic_case(w, h, W, H, seed=100 * w + H)
    tex = {n: RenderTexture(ctx, *((w, h) if n in LOW else (W, H))) for n in LOW + FULL_IN}
    for n, t in tex.items():
        t.SetPixels(c[n])
    pattern = torch.from_numpy(np.random.default_rng(7).uniform(-9, -1, (2, H + 2 * GUARD, W, 4)).astype(F)).to(dev)
    ext = pattern.clone()
    torch.cuda.synchronize(dev)
    out = [RenderTexture(ctx, W, H, external_ptr=ext[k, GUARD].data_ptr()) for k in range(2)]
    seen_stage2 = seen_none = 0
    try:
        for low_count in (True, False):
            for albedo in (True, False):
                for flags in (0, WIDE_FALLBACK, SKY_FROM_ALBEDO, WIDE_FALLBACK | SKY_FROM_ALBEDO):
                    ref = ref_of(c, low_count, albedo, flags, count_scale=0.375)
                    seen_stage2 += int(ref["stage2"].sum())
                    seen_none += int((~ref["result"]).sum())
                    for count in (True, False):
                        ext.copy_(pattern)
                        torch.cuda.synchronize(dev)
                        ctx.upsample(tex["low_color"], tex["low_hit"], tex["low_normal"], tex["low_id"], tex["hit"], tex["normal"], tex["id"],
                                     out[0], out[1] if count else None, low_count=tex["low_count"] if low_count else None,
                                     albedo=tex["albedo"] if albedo else None, count_scale=0.375, wide_fallback=bool(flags & WIDE_FALLBACK),
                                     sky_from_albedo=bool(flags & SKY_FROM_ALBEDO))
                        ctx.synchronize()
                        got, keep = ext.cpu().numpy(), pattern.cpu().numpy()
                        what = f"{pair} low_count={low_count} albedo={albedo} flags={flags} count={count}"
                        assert_bits(got[0, GUARD:GUARD + H], ref["color"], what + " color")
                        assert_bits(got[1, GUARD:GUARD + H], ref["count"] if count else keep[1, GUARD:GUARD + H], what + " count")
                        for k in range(2):                               # nothing outside the W x H texels
                            assert got[k, :GUARD].tobytes() == keep[k, :GUARD].tobytes(), what + " guard below"
                            assert got[k, GUARD + H:].tobytes() == keep[k, GUARD + H:].tobytes(), what + " guard above"
        # other thresholds, the default count_scale
        for nt, pt in ((-1.0, 1e3), (0.99, 0.001), (0.5, 0.2)):
            ref = ref_of(c, True, True, WIDE_FALLBACK, normal_threshold=nt, plane_threshold=pt)
            ctx.upsample(tex["low_color"], tex["low_hit"], tex["low_normal"], tex["low_id"], tex["hit"], tex["normal"], tex["id"], out[0], out[1],
                         low_count=tex["low_count"], albedo=tex["albedo"], normal_threshold=nt, plane_threshold=pt)
            ctx.synchronize()
            got = ext.cpu().numpy()
            assert_bits(got[0, GUARD:GUARD + H], ref["color"], f"{pair} nt={nt} pt={pt} color")
            assert_bits(got[1, GUARD:GUARD + H], ref["count"], f"{pair} nt={nt} pt={pt} count")
    finally:
        for t in list(tex.values()) + out:
            t.Release()
    if w >= 4 and h >= 4 and W * H >= w * h:                                 # the cases do reach the fallback and the pixels nothing serves
        assert seen_stage2 > 0 and seen_none > 0, (seen_stage2, seen_none)


# ---- 2. a real scene --------------------------------------------------------------------------------------------------------------------
def rendered_case(ctx, frames=6, low=(24, 16), full=(48, 32)):
    """The mixed scene traced on the low grid with temporal accumulation, and render_aov's guides on both grids: (master, low guide
    textures (hit, normal, albedo, id), full guide textures)."""
    m = RayTraceMaster(ctx, scenes.mixed_test_scene(*low))
    m.EnableTemporalAccumulation()
    for _ in range(frames):
        m.OnRenderImage()
    low_t = m.RenderFeatureBuffers()
    full_t = [RenderTexture(ctx, *full) for _ in range(4)]
    ctx.render_aov(*full_t)
    return m, low_t, full_t


def test_real_scene_matches_reference_bit_for_bit(gpu_ctx):
    W, H = 48, 32
    with Context(gpu_ctx.device) as ctx:
        m, low_t, full_t = rendered_case(ctx)
        color, count = RenderTexture(ctx, W, H), RenderTexture(ctx, W, H)
        ctx.upsample(m._converged, low_t[0], low_t[1], low_t[3], full_t[0], full_t[1], full_t[3], color, count, low_count=m._tcount,
                     albedo=full_t[2], sky_from_albedo=True)
        got_c, got_n = color.GetPixels(), count.GetPixels()
        low_color, low_count = m._converged.GetPixels(), m._tcount.GetPixels()
        lo = [t.GetPixels() for t in low_t]
        fu = [t.GetPixels() for t in full_t]
        for t in full_t + [color, count]:
            t.Release()
        m.OnDisable()
    ref = upsample_ref(low_color, lo[0], lo[1], lo[3], fu[0], fu[1], fu[3], low_count=low_count, albedo=fu[2],
                       flags=WIDE_FALLBACK | SKY_FROM_ALBEDO)
    assert_bits(got_c, ref["color"], "color")
    assert_bits(got_n, ref["count"], "count")
    assert (low_count[..., 0] == 6).all()
    assert ref["result"].mean() > 0.9 and ref["sky"].any() and ref["surface"].any()
    assert (got_n[ref["result"]][:, 0] == 6).all()                           # a mean of equal counts
    zero = got_n[..., 0] == 0
    assert not ref["any_tap"][zero].any()                                    # a count of 0: the restatement finds no valid tap at all
    assert (zero == ~ref["result"]).all()
    sky = ref["sky"] & ref["result"]
    assert got_c[sky][:, :3].tobytes() == fu[2][sky][:, :3].tobytes()        # the exact sky


# ---- 3. an observer of deferred frames ------------------------------------------------------------------------------------------------
def deferred_run(device, synchronise):
    W, H = 48, 32
    with Context(device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(24, 16))
        low_t = m.RenderFeatureBuffers()
        full_t = [RenderTexture(ctx, W, H) for _ in range(4)]
        ctx.render_aov(*full_t)
        color, count = RenderTexture(ctx, W, H), RenderTexture(ctx, W, H)
        for _ in range(3):
            m.OnRenderImage()                                                # deferred: three dispatches and their blends into _converged
        if synchronise:
            ctx.synchronize()
        ctx.upsample(m._converged, low_t[0], low_t[1], low_t[3], full_t[0], full_t[1], full_t[3], color, count)
        out = (color.GetPixels(), count.GetPixels(), m._converged.GetPixels(), ctx.launch_info()["n_frames"])
        for t in full_t + [color, count]:
            t.Release()
        m.OnDisable()
    return out


def test_upsample_sees_deferred_frames(gpu_ctx):
    a = deferred_run(gpu_ctx.device, False)
    b = deferred_run(gpu_ctx.device, True)
    assert a[3] == 3, a[3]                                                   # the frames were one deferred batch when urt_upsample came
    assert_bits(a[2], b[2], "converged")
    assert_bits(a[0], b[0], "color")
    assert_bits(a[1], b[1], "count")
    assert (a[1][..., 0] > 0).mean() > 0.9 and (a[0][..., :3] > 0).any()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# name -> (expected code, image changes, params or "null" or None for the defaults' struct)
ERROR_CASES = {
    "images_null": (1, None, {}),
    "flags_unknown_bit": (1, {}, {"flags": 4}),
    "flags_negative": (1, {}, {"flags": -1}),
    "normal_threshold_nan": (1, {}, {"nt": NAN}),
    "plane_threshold_nan": (1, {}, {"pt": NAN}),
    "count_scale_zero": (1, {}, {"cs": 0.0}),
    "count_scale_negative": (1, {}, {"cs": -2.0}),
    "count_scale_inf": (1, {}, {"cs": INF}),
    "count_scale_nan": (1, {}, {"cs": NAN}),
    "low_hit_size": (1, {"low_hit": "odd"}, {}),
    "low_count_size": (1, {"low_count": "odd"}, {}),
    "low_id_has_the_full_size": (1, {"low_id": "=id"}, {}),
    "normal_size": (1, {"normal": "odd"}, {}),
    "albedo_size": (1, {"albedo": "odd"}, {}),
    "color_has_the_low_size": (1, {"color": "=low_color"}, {}),
    "count_size": (1, {"count": "odd"}, {}),
    "color_is_hit": (1, {"color": "=hit"}, {}),
    "color_is_albedo": (1, {"color": "=albedo"}, {}),
    "count_is_id": (1, {"count": "=id"}, {}),
    "count_is_color": (1, {"count": "=color"}, {}),
    "color_is_sky": (1, {"color": "sky"}, {}),
    "count_is_sky": (1, {"count": "sky"}, {}),
    "low_color_zero": (2, {"low_color": 0}, {}),
    "low_hit_zero": (2, {"low_hit": 0}, {}),
    "low_normal_zero": (2, {"low_normal": 0}, {}),
    "low_id_zero": (2, {"low_id": 0}, {}),
    "hit_zero": (2, {"hit": 0}, {}),
    "normal_zero": (2, {"normal": 0}, {}),
    "id_zero": (2, {"id": 0}, {}),
    "color_zero": (2, {"color": 0}, {}),
    "low_color_unknown": (2, {"low_color": 987654}, {}),
    "low_count_unknown": (2, {"low_count": 987654}, {}),
    "albedo_unknown": (2, {"albedo": 987654}, {}),
    "count_unknown": (2, {"count": 987654}, {}),
    "color_released": (2, {"color": "gone"}, {}),
}


@pytest.fixture(scope="module")
def error_rig(gpu_ctx):
    w, h, W, H = 6, 4, 16, 8
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        tex = {n: RenderTexture(ctx, *((w, h) if n in LOW else (W, H))) for n in NAMES}
        tex["odd"], tex["sky"] = RenderTexture(ctx, 5, 5), RenderTexture(ctx, W, H)
        snap = {}
        for n, t in tex.items():
            snap[n] = rng.uniform(-2, 2, (t.height, t.width, 4)).astype(F)
            t.SetPixels(snap[n])
        gone = RenderTexture(ctx, W, H)
        gone_h = gone.handle
        gone.Release()
        sh = ComputeShader(ctx)
        sh.SetTexture(0, "_SkyboxTexture", tex["sky"])
        yield ctx, tex, snap, gone_h
        sh.SetTexture(0, "_SkyboxTexture", None)
        for t in tex.values():
            t.Release()


def error_call(rig, changes, params):
    ctx, tex, _, gone_h = rig
    if changes is None:
        images = None
    else:
        d = {n: tex[n].handle for n in NAMES}
        for n, v in changes.items():
            d[n] = gone_h if v == "gone" else tex[v[1:]].handle if isinstance(v, str) and v.startswith("=") else tex[v].handle if isinstance(v, str) else v
        images = C.byref(_lib.UpsampleImages(*(d[n] for n in NAMES)))
    p = None if params == "null" else C.byref(_lib.UpsampleParams(params.get("nt", 0.9), params.get("pt", 0.02), params.get("cs", 1.0),
                                                                  params.get("flags", 1)))
    return ctx.lib.urt_upsample(ctx._h, images, p)


@pytest.mark.parametrize("case", sorted(ERROR_CASES))
def test_errors_write_nothing(error_rig, case):
    code, changes, params = ERROR_CASES[case]
    ctx, tex, snap, _ = error_rig
    assert error_call(error_rig, changes, params) == code
    ctx.synchronize()
    for n, t in tex.items():
        assert t.GetPixels().tobytes() == snap[n].tobytes(), n


def test_valid_calls_after_the_errors_do_write(error_rig):
    ctx, tex, snap, _ = error_rig
    assert ctx.lib.urt_upsample(None, None, None) == 1
    assert error_call(error_rig, {}, "null") == 0                            # params == NULL: the defaults
    by_null = (tex["color"].GetPixels(), tex["count"].GetPixels())
    assert by_null[0].tobytes() != snap["color"].tobytes() and by_null[1].tobytes() != snap["count"].tobytes()
    tex["color"].SetPixels(snap["color"]); tex["count"].SetPixels(snap["count"])
    d = _lib.UPSAMPLE_DEFAULTS
    assert error_call(error_rig, {}, {"nt": d["normal_threshold"], "pt": d["plane_threshold"], "cs": d["count_scale"], "flags": d["flags"]}) == 0
    assert tex["color"].GetPixels().tobytes() == by_null[0].tobytes() and tex["count"].GetPixels().tobytes() == by_null[1].tobytes()
    assert error_call(error_rig, {"low_count": 0, "albedo": 0, "count": 0}, {"flags": 3}) == 0      # every optional image left out
    for n in NAMES[:-2]:
        assert tex[n].GetPixels().tobytes() == snap[n].tobytes(), n          # the inputs are only read
    tex["color"].SetPixels(snap["color"]); tex["count"].SetPixels(snap["count"])


def test_counters_and_the_scene_are_left_alone(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        m, low_t, full_t = rendered_case(ctx, frames=2)
        color = RenderTexture(ctx, 48, 32)
        ctx.synchronize()
        c0 = ctx.counters()
        ctx.upsample(m._converged, low_t[0], low_t[1], low_t[3], full_t[0], full_t[1], full_t[3], color)
        ctx.synchronize()
        assert ctx.counters() == c0
        for t in full_t + [color]:
            t.Release()
        m.OnDisable()


# ---- 5. RayTraceMaster.Upscale ---------------------------------------------------------------------------------------------------------
def upscale_master(ctx, temporal):
    m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
    m.numRays = 2
    if temporal:
        m.EnableTemporalAccumulation()
    for _ in range(4):
        m.OnRenderImage()
    return m


@pytest.mark.parametrize("temporal", [False, True], ids=["mean", "temporal"])
@pytest.mark.parametrize("size", [(96, 64), (100, 70)], ids=lambda s: "%dx%d" % s)
def test_master_upscale(gpu_ctx, size, temporal):
    W, H = size
    below = 1.0
    with Context(gpu_ctx.device) as ctx:
        twin = upscale_master(ctx, temporal)                                 # the same frames without any Upscale
        twin.OnRenderImage()
        twin_frame, twin_conv = twin._target.GetPixels(), twin._converged.GetPixels()
        twin.OnDisable()
        m = upscale_master(ctx, temporal)
        with pytest.raises(ValueError):
            m.Upscale(W, H, destination=m._target)                           # not W x H
        # without hole filling: Context.upsample by hand with the same inputs, and the restatement
        out = m.Upscale(W, H)
        assert out is m._upscaled and (out.width, out.height) == (W, H) and m.upscaleFilled == 0
        got_c, got_n = out.GetPixels(), m._upcount.GetPixels()
        low_hit, low_normal, _, low_id = m._uplow
        hit, normal, albedo, ids = m._upaov
        counts = {"low_count": m._tcount} if temporal else {"count_scale": 4.0 * (48 * 32) / (W * H)}
        mine, mine_n, result = RenderTexture(ctx, W, H), RenderTexture(ctx, W, H), RenderTexture(ctx, W, H)
        ctx.upsample(m._converged, low_hit, low_normal, low_id, hit, normal, ids, mine, mine_n, albedo=albedo, sky_from_albedo=True, **counts)
        assert_bits(got_c, mine.GetPixels(), "Upscale vs Context.upsample: color")
        assert_bits(got_n, mine_n.GetPixels(), "Upscale vs Context.upsample: count")
        ref = upsample_ref(m._converged.GetPixels(), low_hit.GetPixels(), low_normal.GetPixels(), low_id.GetPixels(), hit.GetPixels(),
                           normal.GetPixels(), ids.GetPixels(), low_count=m._tcount.GetPixels() if temporal else None, albedo=albedo.GetPixels(),
                           count_scale=counts.get("count_scale", 1.0), flags=WIDE_FALLBACK | SKY_FROM_ALBEDO)
        assert_bits(got_c, ref["color"], "Upscale vs reference: color")
        assert_bits(got_n, ref["count"], "Upscale vs reference: count")
        assert ref["result"].mean() > 0.9
        # with hole filling: select, trace and blend by hand under the same uniforms
        dest = RenderTexture(ctx, W, H)
        assert m.Upscale(W, H, destination=dest, fill_holes=True, below=below) is dest
        fill_c, fill_n = dest.GetPixels(), m._upcount.GetPixels()
        assert (fill_n[..., 0] >= below).all()
        m.RayTraceShader.SetTexture(0, "Result", result)
        xy = ctx.select_pixels(mine_n, below)
        samples = ctx.radiance_query_pixels(xy, m.numRays, m.numBounces)
        ctx.blend_samples(xy, samples, mine, mine_n, 1.0, 0.0)
        assert m.upscaleFilled == len(xy) and len(xy) >= int((~ref["result"]).sum())
        assert_bits(fill_c, mine.GetPixels(), "filled color")
        assert_bits(fill_n, mine_n.GetPixels(), "filled count")
        sel = np.zeros((H, W), bool)
        xy_h = xy.cpu().numpy()
        sel[xy_h[:, 1], xy_h[:, 0]] = True
        assert fill_c[~sel].tobytes() == got_c[~sel].tobytes() and fill_n[~sel].tobytes() == got_n[~sel].tobytes()
        if temporal or size == (96, 64):                                     # counts of 4 (or 4 * 1/4): only the holes are below 1
            assert (sel == ~ref["result"]).all()
            assert np.array_equal(u32(fill_c[sel]), u32(samples.cpu().numpy()))
        # the next frame is the low-size frame it would have been: Result was rebound, nothing of the accumulation moved
        m.OnRenderImage()
        assert_bits(m._target.GetPixels(), twin_frame, "the frame after Upscale")
        assert_bits(m._converged.GetPixels(), twin_conv, "the accumulation after Upscale")
        for t in (mine, mine_n, result, dest):
            t.Release()
        m.OnDisable()
        assert m._upaov is None and m._upcount is None and m._upscaled is None and m._uptarget is None


def test_upscale_needs_a_frame_and_gives_everything_back(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        def run(first):
            m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
            if first:
                with pytest.raises(UrtError):
                    m.Upscale(96, 64)                                        # before the first frame
            m.OnRenderImage()
            m.Upscale(96, 64, fill_holes=True)
            m.Upscale(100, 70, fill_holes=True, below=0.5)                   # another size: the textures are re-created
            m.OnRenderImage()
            ctx.synchronize()
            m.OnDisable()
        run(True)                                                            # grows the context's own scratch to what the sequence needs
        before = live_resources()
        run(False)
        assert live_resources() == before                                    # OnDisable leaves the tally where it was before the master


# ---- 6. quality --------------------------------------------------------------------------------------------------------------------------
def edge_mask(ids, normal, radius=2):
    """Pixels within `radius` texels (Chebyshev) of a change of object id or kind between 4-neighbours."""
    key = ids.view(np.int32)[..., 0].astype(np.int64) * 8 + normal[..., 3].astype(np.int64)
    edge = np.zeros(key.shape, bool)
    dx = key[:, 1:] != key[:, :-1]
    dy = key[1:, :] != key[:-1, :]
    edge[:, 1:] |= dx; edge[:, :-1] |= dx
    edge[1:, :] |= dy; edge[:-1, :] |= dy
    out = edge.copy()
    H, W = edge.shape
    for oy in range(-(radius - 1), radius):
        for ox in range(-(radius - 1), radius):
            ys, xs = np.nonzero(edge)
            out[np.clip(ys + oy, 0, H - 1), np.clip(xs + ox, 0, W - 1)] = True
    return out


def test_quality_at_edges_beats_a_plain_bilinear_resize(gpu_ctx):
    """Mixed scene, 48 x 32 traced for 16 frames, against 96 x 64 traced for 64: over the pixels within 2 texels of an id or kind change
    the guided result has the lower RMSE.  Measured on one MI355X at the starting thresholds 0.9 / 0.02: guided 0.3076,
    plain bilinear 0.3858 over 739 pixels; one texel off the change 0.1103 against 0.2268.  With guides through the pixel centres
    instead of the centres of the frames' samples (RayTraceMaster._sample_centre_projection) the relation fails, 0.3947 against 0.3785."""
    W, H = 96, 64
    with Context(gpu_ctx.device) as ctx:
        truth_m = RayTraceMaster(ctx, scenes.mixed_test_scene(W, H), frame_seed=0xBEEF)
        for _ in range(64):
            truth_m.OnRenderImage()
        truth = truth_m._converged.GetPixels()[..., :3].astype(np.float64)
        truth_m.OnDisable()
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(48, 32))
        for _ in range(16):
            m.OnRenderImage()
        guided = m.Upscale(W, H).GetPixels()
        count = m._upcount.GetPixels()[..., 0]
        low = m._converged.GetPixels()
        ids, normal = m._upaov[3].GetPixels(), m._upaov[1].GetPixels()
        filled = m.Upscale(W, H, fill_holes=True).GetPixels()
        n_filled = m.upscaleFilled
        m.OnDisable()
    plain = bilinear_resize_ref(low, W, H)[..., :3]
    mask = edge_mask(ids, normal, 2)
    rmse = lambda a: float(np.sqrt(((a[..., :3].astype(np.float64) - truth)[mask] ** 2).mean()))  # noqa: E731
    g, p, f = rmse(guided), rmse(plain), rmse(filled)
    ring = mask & ~edge_mask(ids, normal, 1)                                 # without the pixels on either side of the change itself
    rmse_ring = lambda a: float(np.sqrt(((a[..., :3].astype(np.float64) - truth)[ring] ** 2).mean()))  # noqa: E731
    print(f"upsample quality one texel off the change ({int(ring.sum())} pixels): RMSE guided {rmse_ring(guided):.4e}, "
          f"plain bilinear {rmse_ring(plain):.4e}")
    print(f"upsample quality at edges ({int(mask.sum())} of {W * H} pixels): RMSE guided {g:.4e}, plain bilinear {p:.4e}, "
          f"guided + fill_holes {f:.4e}; holes {int((count == 0).sum())}, filled {n_filled}")
    assert 0.05 < mask.mean() < 0.6
    assert g < p, (g, p)
