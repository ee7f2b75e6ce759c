"""GPU: depth of field (include/urt.h urt_depth_of_field, RayTraceMaster.EnableDepthOfField) — every comparison bit for bit against the
numpy restatement (tests/dof_ref.py), which loops over all 33 x 33 taps and knows no tiles: ragged sizes across the 16 x 16 tiles at three
radii, the images built against the kernels' tile-reach bound, the closed forms, URT_DOF_FLAG_COC, the parameters' corners, the scratch
reused at other sizes, ordering with deferred frames and with bloom and tone mapping, the error contract against sentinel fills,
counters and resources, and ToneMap with the effect on and off."""
import ctypes as C
import functools

import numpy as np
import pytest

import dof_cases as cases
from bloom_ref import bloom_ref
from dof_cases import F, INF, NAN, U, assert_bits, bits
from dof_ref import FLAG_COC, coc_ref, dof_ref
from tonemap_ref import tonemap_ref
from unityraytracer_amd import Context, RayTraceMaster, _lib, live_resources, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

RANDOM = {"focus_distance": 4.0, "scale": 6.0}


@functools.lru_cache(maxsize=None)
def reference(w, h, seed=0, **params):
    out = dof_ref(cases.image(w, h, seed), cases.hit_image(w, h, seed), **params)
    out.setflags(write=False)
    return out


class Trio:
    """src, hit and dst of one size on a context, released at the end."""
    def __init__(self, ctx, w, h, src=None, hit=None):
        self.tex = tuple(RenderTexture(ctx, w, h) for _ in range(3))
        if src is not None:
            self.tex[0].SetPixels(src)
        if hit is not None:
            self.tex[1].SetPixels(hit)

    def __enter__(self):
        return self.tex

    def __exit__(self, *exc):
        for t in self.tex:
            t.Release()


def run(ctx, src_px, hit_px, **params):
    h, w = src_px.shape[:2]
    with Trio(ctx, w, h, src_px, hit_px) as (src, hit, dst):
        ctx.depth_of_field(src, hit, dst, **params)
        return dst.GetPixels()


# ---- 1. every shape and radius -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 9), (9, 1), (3, 5), (16, 16), (17, 33), (33, 17), (70, 38), (130, 66)]


@pytest.mark.parametrize("max_radius", [0.5, 3.0, 16.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_matches_reference_bit_for_bit(gpu_ctx, shape, max_radius):
    w, h = shape
    with Trio(gpu_ctx, w, h, cases.image(w, h), cases.hit_image(w, h)) as (src, hit, dst):
        dst.SetPixels(np.full((h, w, 4), NAN, F))
        gpu_ctx.depth_of_field(src, hit, dst, max_radius=max_radius, **RANDOM)
        assert_bits(dst.GetPixels(), reference(w, h, max_radius=max_radius, **RANDOM), f"{shape} max_radius={max_radius}")
        assert_bits(src.GetPixels(), cases.image(w, h), "src is only read")
        assert_bits(hit.GetPixels(), cases.hit_image(w, h), "hit is only read")


# ---- 2. the reach shortcut -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", sorted(cases.REACH_PLANES))
@pytest.mark.parametrize("position", sorted(cases.REACH_POSITIONS))
def test_one_wide_pixel_reaches_every_tile_it_covers(gpu_ctx, position, plane):
    src, hit, ref = cases.reach_case(position, plane)
    assert_bits(run(gpu_ctx, src, hit, **cases.REACH_PARAMS), ref, f"{position} {plane}")


def test_the_reach_is_not_rounded_down_and_an_in_focus_tile_sees_its_blurred_neighbours(gpu_ctx):
    src, hit, params, ref = cases.rounding_case()
    assert_bits(run(gpu_ctx, src, hit, **params), ref, "a = 15.5 + 2^-20")
    src, hit, ref = cases.in_focus_tile_case()
    got = run(gpu_ctx, src, hit, **cases.REACH_PARAMS)
    assert_bits(got, ref, "one in-focus tile")
    assert_bits(got[16:32, 16:32], src[16:32, 16:32], "the in-focus tile lies in front of the sky and stays sharp")


# ---- 3. the closed forms ----------------------------------------------------------------------------------------------------------------
def test_the_headers_closed_forms(gpu_ctx):
    w, h = 70, 38
    src, hit = cases.image(w, h), cases.hit_image(w, h)
    zero = {"focus_distance": 2.0 ** -10, "scale": 0.0, "max_radius": 16.0}      # (s / z stays finite at the denormal depth)
    got = run(gpu_ctx, src, hit, **zero)
    assert_bits(got, dof_ref(src, hit, **zero), "scale 0 vs reference")
    assert np.array_equal(got[~np.isnan(src)], src[~np.isnan(src)])              # src by value; a -0 colour of a lens pixel comes out +0
    differ = bits(got) != bits(src)
    assert differ.any() and (bits(src)[differ] == 0x80000000).all() and (bits(got)[differ] == 0).all()
    const = np.full((h, w, 4), 4.0, F)
    for params in ({}, {"scale": 1e30, "max_radius": 16.0}, {"focus_distance": 0.3, "max_radius": 0.5}):
        assert_bits(run(gpu_ctx, const, hit, **params), const, f"a constant 4.0 {params}")
    src, hit, params = cases.depth_step()
    got = run(gpu_ctx, src, hit, **params)
    half = src.shape[1] // 2
    assert_bits(got, dof_ref(src, hit, **params), "depth step")
    assert_bits(got[:, :half], src[:, :half], "the sharp foreground")
    assert np.isfinite(got).all() and not np.array_equal(got[:, half:], src[:, half:])


def test_pass_through_pixels_are_never_taps(gpu_ctx):
    w, h = 33, 17
    src, hit = np.array(cases.image(w, h)), cases.hit_image(w, h)
    params = {"max_radius": 16.0, **RANDOM}
    lens = coc_ref(src, hit, **params)[2]
    with Trio(gpu_ctx, w, h, src, hit) as (s, z, d):
        gpu_ctx.depth_of_field(s, z, d, **params)
        out = d.GetPixels()
        assert_bits(out[~lens], src[~lens], "pass-through pixels are copied")
        changed = src.copy()
        changed[~lens, :3] = np.where(np.isfinite(src[~lens, :3]) & (np.abs(src[~lens, :3]) <= 2.0 ** 100), F(NAN), F(3e38))
        s.SetPixels(changed)
        gpu_ctx.depth_of_field(s, z, d, **params)
        again = d.GetPixels()
        assert_bits(again[lens], out[lens], "lens pixels after the pass-through colours changed")
        assert_bits(again[~lens], changed[~lens], "pass-through pixels are copied")


# ---- 4. URT_DOF_FLAG_COC ---------------------------------------------------------------------------------------------------------------
def test_the_coc_flag_shows_the_blur_radius(gpu_ctx):
    w, h = 70, 38
    src, hit = cases.image(w, h), cases.hit_image(w, h)
    for params in ({"max_radius": 16.0, **RANDOM}, {"scale": 5.0, "max_radius": 3.0}, {"scale": 2.5, "max_radius": 16.0}):
        got = run(gpu_ctx, src, hit, flags=_lib.URT_DOF_FLAG_COC, **params)
        a, z, lens = coc_ref(src, hit, **params)
        assert_bits(got, dof_ref(src, hit, flags=FLAG_COC, **params), f"coc {params}")
        assert_bits(got[..., :3], np.repeat(a[..., None], 3, axis=2), "a_p in the three channels")
        assert_bits(got[..., 3], src[..., 3], "alpha")
        assert (bits(got[~lens][:, :3]) == 0).all() and (~lens).any()          # zeros at the pass-through pixels
        sky = lens & np.isinf(z)
        assert sky.any() and (got[sky][:, 0] == F(min(params["scale"], params["max_radius"]))).all()    # min(K, Rmax), exactly
        assert (got[lens][:, 0] >= 0.5).all() and (got[lens][:, 0] <= params["max_radius"]).all()


# ---- 5. the parameters' corners -----------------------------------------------------------------------------------------------------------
CORNERS = {
    "defaults": {},
    "scale_0": {"scale": 0.0}, "scale_0_wide": {"scale": 0.0, "max_radius": 16.0},
    "scale_large": {"scale": 3e38, "max_radius": 5.0}, "scale_large_wide": {"scale": 1e30, "max_radius": 16.0},
    "focus_smallest_normal": {"focus_distance": 1.17549435e-38, "max_radius": 4.0},
    "focus_huge": {"focus_distance": 3e38, "scale": 7.0, "max_radius": 7.0},
    "radius_half": {"max_radius": 0.5, "scale": 100.0},
}


@pytest.mark.parametrize("corner", sorted(CORNERS))
def test_parameter_corners(gpu_ctx, corner):
    w, h = 70, 38
    assert_bits(run(gpu_ctx, cases.image(w, h), cases.hit_image(w, h), **CORNERS[corner]), reference(w, h, **CORNERS[corner]), corner)


def test_params_null_means_the_defaults(gpu_ctx):
    w, h = 33, 17
    with Trio(gpu_ctx, w, h, cases.image(w, h), cases.hit_image(w, h)) as (src, hit, dst):
        assert gpu_ctx.lib.urt_depth_of_field(gpu_ctx._h, src.handle, hit.handle, dst.handle, None) == 0
        assert_bits(dst.GetPixels(), reference(w, h), "params == NULL")


# ---- 6. the scratch, back-to-back calls, deferred frames ---------------------------------------------------------------------------------
def test_the_scratch_is_reused_across_sizes(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        for k, (w, h) in enumerate([(130, 66), (3, 5), (130, 66), (17, 33), (70, 38)]):
            with Trio(ctx, w, h, cases.image(w, h, seed=k % 2), cases.hit_image(w, h, seed=k % 2)) as (src, hit, dst):
                held = live_resources()["device_bytes"]
                ctx.depth_of_field(src, hit, dst, max_radius=16.0, **RANDOM)
                grown = live_resources()["device_bytes"] - held
                assert grown == (4 * (2 * w * h + ((w + 15) // 16) * ((h + 15) // 16)) if k == 0 else 0)   # {a, z} and the tile table, once
                assert_bits(dst.GetPixels(), reference(w, h, seed=k % 2, max_radius=16.0, **RANDOM), f"call {k} at {w} x {h}")


def test_calls_back_to_back_share_the_scratch_in_order(gpu_ctx):
    ctx = gpu_ctx
    with Trio(ctx, 70, 38, cases.image(70, 38), cases.hit_image(70, 38)) as (src, hit, dst), \
            Trio(ctx, 33, 17, cases.image(33, 17), cases.hit_image(33, 17)) as (src2, hit2, dst2):
        ctx.depth_of_field(src, hit, dst, max_radius=16.0, **RANDOM)
        ctx.depth_of_field(src2, hit2, dst2, max_radius=3.0, **RANDOM)           # the same scratch, no synchronisation in between
        ctx.depth_of_field(dst, hit, src, scale=2.0)                             # and the first result, blurred again
        assert_bits(dst2.GetPixels(), reference(33, 17, max_radius=3.0, **RANDOM), "second call")
        once = reference(70, 38, max_radius=16.0, **RANDOM)
        assert_bits(dst.GetPixels(), once, "first call")
        assert_bits(src.GetPixels(), dof_ref(once, cases.hit_image(70, 38), scale=2.0), "third call on the first's result")


def test_deferred_frames_are_seen_and_bloom_and_tonemap_follow_in_place(gpu_ctx):
    w, h = 48, 32
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(w, h))
        hit, out = RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
        hit.SetPixels(cases.hit_image(w, h))
        for _ in range(3):
            m.OnRenderImage()                                                     # deferred: three dispatches and their urt_blit_add into _converged
        bad = _lib.DofParams(10.0, 8.0, 17.0, 0)                                  # max_radius 17
        assert ctx.lib.urt_depth_of_field(ctx._h, m._converged.handle, hit.handle, out.handle, C.byref(bad)) == 1
        params = {"focus_distance": 3.0, "scale": 5.0, "max_radius": 6.0}
        ctx.depth_of_field(m._converged, hit, out, **params)
        got = out.GetPixels()
        assert ctx.launch_info()["n_frames"] == 3                                 # one deferred batch when the valid call came
        conv = m._converged.GetPixels()
        assert (conv[..., :3] > 0).any()
        blurred = dof_ref(conv, cases.hit_image(w, h), **params)
        assert_bits(got, blurred, "after deferred frames")
        assert not np.array_equal(bits(got), bits(conv))
        ctx.bloom(out, out, threshold=0.125)
        ctx.tonemap(out, out)
        bloomed, b = bloom_ref(blurred, threshold=0.125)
        assert (b > 0).any() and not np.isnan(bloomed).any()
        assert_bits(out.GetPixels(), tonemap_ref(bloomed), "depth of field, bloom, tone mapping: the three references composed")
        for t in (hit, out):
            t.Release()
        m.OnDisable()


# ---- 7. RayTraceMaster ------------------------------------------------------------------------------------------------------------------
def sample_centre_hit(m, w, h):
    """urt_render_aov's hit target through the centres of the frames' samples: _CameraInverseProjection with the uv moved by half a pixel
    (its last column plus the first over w plus the second over h), the host's matrix bound again afterwards."""
    p = np.array(m.scene.camera_inverse_projection, dtype=F).reshape(16).copy()
    p[12:16] += p[0:4] * F(1.0 / w) + p[4:8] * F(1.0 / h)
    tex = RenderTexture(m.ctx, w, h)
    m.RayTraceShader.SetMatrix("_CameraInverseProjection", p)
    m.ctx.render_aov(hit=tex)
    m.RayTraceShader.SetMatrix("_CameraInverseProjection", m.scene.camera_inverse_projection)
    px = tex.GetPixels()
    tex.Release()
    return px


@pytest.mark.parametrize("bloom", [False, True], ids=["plain", "bloom"])
def test_master_tonemap_with_depth_of_field(gpu_ctx, bloom):
    w, h = 32, 24
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        m = RayTraceMaster(ctx, scenes.mixed_test_scene(w, h))
        for _ in range(3):
            m.OnRenderImage()
        if bloom:
            m.EnableBloom(threshold=0.25, intensity=0.5)
        before = m.ToneMap().GetPixels()                                          # today's bytes
        conv = m._converged.GetPixels()
        centre = np.array(m.RenderFeatureBuffers()[0].GetPixels())               # the pixel-centre guide, under the host's matrix
        today = bloom_ref(conv, threshold=0.25, intensity=0.5)[0] if bloom else conv
        assert_bits(before, tonemap_ref(today), "without depth of field")
        hit = sample_centre_hit(m, w, h)
        z = hit[..., 3]
        assert np.isinf(z).any() and (np.isfinite(z) & (z > 0)).sum() > 50      # sky and surfaces
        params = {"focus_distance": float(np.median(z[np.isfinite(z)])), "scale": 5.0, "max_radius": 6.0}
        held, counters = live_resources(), ctx.counters()
        m.EnableDepthOfField(**params)
        assert live_resources() == held and m._dofHit is None                    # EnableDepthOfField creates nothing
        out = m.ToneMap()
        assert out is m._tonemapped and (m._dofHit.width, m._dofHit.height) == (w, h)
        assert_bits(m._dofHit.GetPixels(), hit, "the owned guide")
        blurred = dof_ref(conv, hit, **params)
        assert not np.array_equal(bits(blurred), bits(conv))
        staged = bloom_ref(blurred, threshold=0.25, intensity=0.5)[0] if bloom else blurred
        assert_bits(out.GetPixels(), tonemap_ref(staged), "render_aov, depth of field, (bloom,) tone mapping composed")
        assert not np.array_equal(bits(out.GetPixels()), bits(before))
        assert_bits(m._converged.GetPixels(), conv, "_converged is never modified")
        assert ctx.counters() == counters
        probe = RenderTexture(ctx, w, h)                                          # the host's matrix is bound again
        ctx.render_aov(hit=probe)
        assert_bits(probe.GetPixels(), centre, "the camera after ToneMap")
        dest, guide = RenderTexture(ctx, w, h), m._dofHit
        m.EnableDepthOfField(focus_distance=params["focus_distance"] * 2.0, scale=3.0)      # a focus pull: no ray of the image is traced
        assert m.ToneMap(destination=dest, operator="reinhard") is dest and m._dofHit is guide
        pulled = dof_ref(conv, hit, focus_distance=params["focus_distance"] * 2.0, scale=3.0)
        staged = bloom_ref(pulled, threshold=0.25, intensity=0.5)[0] if bloom else pulled
        assert_bits(dest.GetPixels(), tonemap_ref(staged, op=1), "into a destination")
        assert_bits(m._converged.GetPixels(), conv, "_converged is never modified")
        m.DisableDepthOfField()
        assert_bits(m.ToneMap().GetPixels(), before, "DisableDepthOfField restores today's bytes")
        with pytest.raises(ValueError):
            m.EnableDepthOfField(max_radius=17.0)
        assert m._dof is None
        for t in (probe, dest):
            t.Release()
        m.OnDisable()
        assert m._dofHit is None


def test_everything_is_given_back(gpu_ctx):
    def once():
        with Context(gpu_ctx.device) as ctx:
            m = RayTraceMaster(ctx, scenes.mixed_test_scene(32, 24))
            m.EnableDepthOfField()
            m.OnRenderImage()
            m.ToneMap()
            m.OnDisable()
    once()
    before = live_resources()
    once()
    assert live_resources() == before


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------------
ARG, HANDLE = 1, 2
DOF_OK = {"focus_distance": 10.0, "scale": 8.0, "max_radius": 8.0, "flags": 0}
# name -> (expected code, call changes: src / hit / dst, params changes)
DOF_ERRORS = {
    "focus_zero": (ARG, {}, {"focus_distance": 0.0}), "focus_negative": (ARG, {}, {"focus_distance": -10.0}),
    "focus_nan": (ARG, {}, {"focus_distance": NAN}), "focus_inf": (ARG, {}, {"focus_distance": INF}),
    "scale_negative": (ARG, {}, {"scale": -1e-6}), "scale_nan": (ARG, {}, {"scale": NAN}), "scale_inf": (ARG, {}, {"scale": INF}),
    "radius_below_half": (ARG, {}, {"max_radius": 0.49}), "radius_zero": (ARG, {}, {"max_radius": 0.0}),
    "radius_above_16": (ARG, {}, {"max_radius": 16.001}), "radius_nan": (ARG, {}, {"max_radius": NAN}), "radius_inf": (ARG, {}, {"max_radius": INF}),
    "flags_unknown_bit": (ARG, {}, {"flags": 2}), "flags_high_bit": (ARG, {}, {"flags": -2147483648}),
    "flags_unknown_bit_with_coc": (ARG, {}, {"flags": 3}),
    "dst_size": (ARG, {"dst": "odd"}, {}), "src_size": (ARG, {"src": "odd"}, {}), "hit_size": (ARG, {"hit": "odd"}, {}),
    "dst_is_src": (ARG, {"dst": "src"}, {}), "dst_is_hit": (ARG, {"dst": "hit"}, {}),
    "dst_is_src_with_coc": (ARG, {"dst": "src"}, {"flags": 1}),
    "dst_is_sky": (ARG, {"dst": "sky"}, {}),
    "src_zero": (HANDLE, {"src": 0}, {}), "hit_zero": (HANDLE, {"hit": 0}, {}), "dst_zero": (HANDLE, {"dst": 0}, {}),
    "src_unknown": (HANDLE, {"src": 987654}, {}), "hit_unknown": (HANDLE, {"hit": 987654}, {}), "dst_unknown": (HANDLE, {"dst": 987654}, {}),
    "dst_released": (HANDLE, {"dst": "gone"}, {}),
    "ctx_null": (ARG, {"ctx": None}, {}),
}
SENTINEL = 0xC0FFEE42


@pytest.fixture(scope="module")
def error_rig(gpu_ctx):
    W, H = 16, 8
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        tex = {n: RenderTexture(ctx, W, H) for n in ("src", "hit", "dst", "sky")}
        tex["odd"] = RenderTexture(ctx, 5, 5)
        snap = {}
        for n, t in tex.items():
            snap[n] = rng.uniform(0.1, 4, (t.height, t.width, 4)).astype(F)
            if n == "dst":
                snap[n] = np.full((H, W, 4), SENTINEL, U).view(F)
            t.SetPixels(snap[n])
        gone = RenderTexture(ctx, W, H)
        gone_h = gone.handle
        gone.Release()
        sh = ComputeShader(ctx)
        sh.SetTexture(0, "_SkyboxTexture", tex["sky"])
        for t in tex.values():
            t.GetPixels()                                                        # (whatever a readback keeps is held from here on)
        yield ctx, tex, snap, gone_h, live_resources()["device_bytes"]
        sh.SetTexture(0, "_SkyboxTexture", None)
        for t in tex.values():
            t.Release()


def error_call(rig, changes, params):
    ctx, tex, _, gone_h, _ = rig
    d = {"ctx": ctx._h, **{n: tex[n].handle for n in ("src", "hit", "dst")}}
    for n, v in changes.items():
        d[n] = gone_h if v == "gone" else tex[v].handle if isinstance(v, str) else v
    p = None if params == "null" else C.byref(_lib.DofParams(*({**DOF_OK, **params}[k] for k in DOF_OK)))
    return ctx.lib.urt_depth_of_field(d["ctx"], d["src"], d["hit"], d["dst"], p)


@pytest.mark.parametrize("case", sorted(DOF_ERRORS))
def test_errors_write_nothing_and_allocate_nothing(error_rig, case):
    code, changes, params = DOF_ERRORS[case]
    ctx, tex, snap, _, held = error_rig
    counters = ctx.counters()
    assert error_call(error_rig, changes, params) == code
    ctx.synchronize()
    for n, t in tex.items():
        assert t.GetPixels().tobytes() == snap[n].tobytes(), n
    assert live_resources()["device_bytes"] == held                              # no scratch: the checks come before it
    assert ctx.counters() == counters


def test_valid_calls_after_the_errors_do_write(error_rig):
    ctx, tex, snap, _, held = error_rig
    counters = ctx.counters()
    assert error_call(error_rig, {}, "null") == 0                                # params == NULL: the defaults
    assert_bits(tex["dst"].GetPixels(), dof_ref(snap["src"], snap["hit"]), "defaults")
    assert live_resources()["device_bytes"] - held == 4 * (2 * 16 * 8 + 1)
    assert error_call(error_rig, {"hit": "src"}, {"flags": 1, "max_radius": 16.0}) == 0   # src may stand in for hit: both are only read
    assert_bits(tex["dst"].GetPixels(), dof_ref(snap["src"], snap["src"], flags=1, max_radius=16.0), "hit == src")
    assert error_call(error_rig, {"src": "sky"}, {"focus_distance": 1.0}) == 0   # the sky may be read
    assert_bits(tex["dst"].GetPixels(), dof_ref(snap["sky"], snap["hit"], focus_distance=1.0), "from the sky")
    for n in ("src", "hit", "sky", "odd"):
        assert tex[n].GetPixels().tobytes() == snap[n].tobytes(), n              # the inputs are only read
    assert ctx.counters() == counters


# the height limit of the 16-row tiles (65535 rows of workgroups): textures of their own, 16 MB each
TALLEST = 16 * 65535


def test_textures_taller_than_the_grid_are_refused_and_the_tallest_are_served(gpu_ctx):
    """1 x 1048561 is an error like the others: nothing written, nothing allocated, counters unchanged.  1 x 1048560 is served: in focus
    everywhere (scale 0) every pixel has its own tap alone, w = 4, and (4 c) / 4 = c, so dst is src in bits on positive finite colours —
    a closed form that needs no restatement at this size."""
    rng = np.random.default_rng(8)
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        for height, code in ((TALLEST + 1, ARG), (TALLEST, 0)):
            src_px = np.exp2(rng.uniform(-6, 6, (height, 1, 4))).astype(F)
            hit_px = np.exp2(rng.uniform(-2, 6, (height, 1, 4))).astype(F)
            sentinel = np.full((height, 1, 4), SENTINEL, U).view(F)
            with Trio(ctx, 1, height, src_px, hit_px) as (src, hit, dst):
                dst.SetPixels(sentinel)
                for t in (src, hit, dst):
                    t.GetPixels()                                                # (whatever a readback keeps is held from here on)
                held, counters = live_resources()["device_bytes"], ctx.counters()
                p = _lib.DofParams(4.0, 0.0, 16.0, 0)
                assert ctx.lib.urt_depth_of_field(ctx._h, src.handle, hit.handle, dst.handle, C.byref(p)) == code
                ctx.synchronize()
                grown = live_resources()["device_bytes"] - held
                assert ctx.counters() == counters
                assert src.GetPixels().tobytes() == src_px.tobytes() and hit.GetPixels().tobytes() == hit_px.tobytes()
                if code:
                    assert dst.GetPixels().tobytes() == sentinel.tobytes() and grown == 0
                else:
                    assert_bits(dst.GetPixels(), src_px, "1 x 1048560, in focus")
                    assert grown == 4 * (2 * height + 65535)

