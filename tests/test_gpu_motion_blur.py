"""GPU: motion blur (include/urt.h urt_motion_blur, RayTraceMaster.EnableMotionBlur) — every comparison covers all pixels and all four
channels, bit for bit, against the numpy restatement (tests/motion_blur_ref.py), which knows no workgroups: ragged sizes across the
16 x 16 tiles at three radii, pans, clamped motion, the tie rules, depth order, sky, vectors and colours and depths that are none,
colours at the 2^100 bound, URT_MOTION_BLUR_FLAG_VELOCITY, external textures, the scratch regrown, the error contract against sentinel
fills, and ToneMap with the effect on after an edit and off again on a still view."""
import ctypes as C
import functools

import numpy as np
import pytest

import motion_blur_cases as cases
from motion_blur_cases import F, INF, NAN, U, assert_bits, bits
from motion_blur_ref import FLAG_VELOCITY, motion_blur_ref, velocity_ref
from unityraytracer_amd import Context, RayTraceMaster, _lib, live_resources, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu


class Quad:
    """src, motion, hit and dst of one size on a context, released at the end."""
    def __init__(self, ctx, w, h, src=None, motion=None, hit=None):
        self.tex = tuple(RenderTexture(ctx, w, h) for _ in range(4))
        for t, px in zip(self.tex, (src, motion, hit)):
            if px is not None:
                t.SetPixels(px)

    def __enter__(self):
        return self.tex

    def __exit__(self, *exc):
        for t in self.tex:
            t.Release()


def run(ctx, src_px, motion_px, hit_px, **params):
    h, w = src_px.shape[:2]
    with Quad(ctx, w, h, src_px, motion_px, hit_px) as (src, motion, hit, dst):
        dst.SetPixels(np.full((h, w, 4), NAN, F))
        ctx.motion_blur(src, motion, hit, dst, **params)
        out = dst.GetPixels()
        assert_bits(src.GetPixels(), src_px, "src is only read")
        assert_bits(motion.GetPixels(), motion_px, "motion is only read")
        assert_bits(hit.GetPixels(), hit_px, "hit is only read")
        return out


# ---- 1. every shape and radius, random vectors on images that mix in everything that is no colour, no depth and no vector -----------
SHAPES = [(1, 1), (1, 40), (40, 1), (16, 16), (17, 16), (33, 31), (48, 48), (70, 50)]


@functools.lru_cache(maxsize=None)
def random_reference(w, h, max_radius, flags=0):
    out = motion_blur_ref(cases.image(w, h), cases.random_motion(w, h), cases.hit_image(w, h), shutter=1.0, max_radius=max_radius, flags=flags)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("max_radius", [0.5, 4.0, 16.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_matches_reference_bit_for_bit(gpu_ctx, shape, max_radius):
    w, h = shape
    got = run(gpu_ctx, cases.image(w, h), cases.random_motion(w, h), cases.hit_image(w, h), shutter=1.0, max_radius=max_radius)
    assert_bits(got, random_reference(w, h, max_radius), f"{shape} max_radius={max_radius}")
    got = run(gpu_ctx, cases.image(w, h), cases.random_motion(w, h), cases.hit_image(w, h), shutter=1.0, max_radius=max_radius,
              flags=_lib.URT_MOTION_BLUR_FLAG_VELOCITY)
    assert_bits(got, random_reference(w, h, max_radius, FLAG_VELOCITY), f"{shape} max_radius={max_radius} velocity")


# ---- 2. the named cases --------------------------------------------------------------------------------------------------------------
def _pan(mx, my, w=70, h=50, **params):
    return lambda: (cases.image(w, h), cases.pan(w, h, mx, my), cases.hit_image(w, h), params)


def _invalid_vectors():
    w, h = 33, 31
    mo = np.array(cases.pan(w, h, 9.0, 5.0))
    mo[::2, :, 2] = 0.0                                                          # not valid
    mo[1::4, :, 2] = NAN
    mo[:, 5, 0], mo[:, 9, 1], mo[:, 13, 0], mo[:, 17, 1] = NAN, INF, -INF, 3e38  # (3e38: the first sum overflows, v ends as 0)
    return cases.clean_image(w, h, seed=12), cases.frozen(mo), cases.flat_hit(w, h), {"shutter": 1.0}


def _odd_depths():
    w, h = 33, 31
    z = np.full((h, w), 2.0, F)
    z[3, :], z[9, :], z[:, 20], z[15, 3:9], z[20:, 25:] = NAN, 0.0, -1.0, -0.0, INF
    z[25, 4] = 1e-40
    return cases.clean_image(w, h, seed=13), cases.pan(w, h, -11.0, 14.0), cases.hit_of(z), {"shutter": 1.0}


CASES = {
    "all_still": _pan(0.0, 0.0),
    "shutter_closed": lambda: (cases.image(70, 50), cases.random_motion(70, 50), cases.hit_image(70, 50), {"shutter": 0.0}),
    "pan_x": _pan(12.0, 0.0, shutter=1.0), "pan_y": _pan(0.0, -9.0, shutter=1.0), "pan_diagonal": _pan(7.0, 7.0, shutter=1.0),
    "pan_repeated_k": _pan(3.2, -1.7, shutter=1.0), "pan_default_shutter": _pan(-25.0, 6.0),
    "pan_below_half_a_pixel": _pan(0.9, 0.0),
    "above_radius_0.5": _pan(100.0, 40.0, shutter=1.0, max_radius=0.5), "above_radius_4": _pan(100.0, 40.0, shutter=1.0, max_radius=4.0),
    "above_radius_16": _pan(100.0, 40.0, shutter=1.0, max_radius=16.0), "above_radius_16_axis": _pan(-1000.0, 0.0, shutter=1.0),
    "one_fast_pixel": lambda: (*cases.one_fast_pixel(), {"shutter": 1.0}),
    "equal_m_in_one_tile": lambda: (*cases.equal_m_in_one_tile(), {"shutter": 1.0}),
    "equal_m_in_two_tiles": lambda: (*cases.equal_m_in_two_tiles(), {"shutter": 1.0}),
    "moving_foreground": lambda: (*cases.moving_disc_over_still()[:3], {"shutter": 1.0}),
    "still_foreground": lambda: (*cases.still_disc_over_pan()[:3], {"shutter": 1.0}),
    "moving_disc": lambda: (*cases.moving_disc()[:3], {"shutter": 1.0}),
    "sky_beside_surface": lambda: (*cases.sky_beside_surface(), {"shutter": 1.0}),
    "invalid_vectors": _invalid_vectors,
    "odd_depths": _odd_depths,
    "odd_colours": lambda: (*cases.odd_colours_beside_moving(), {"shutter": 1.0}),
    "colours_at_2_100": lambda: (*cases.bright_pan(), {"shutter": 1.0}),
}


@pytest.mark.parametrize("flags", [0, FLAG_VELOCITY], ids=["image", "velocity"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_named_cases_match_reference_bit_for_bit(gpu_ctx, case, flags):
    src, motion, hit, params = CASES[case]()
    ref = motion_blur_ref(src, motion, hit, flags=flags, **params)
    got = run(gpu_ctx, src, motion, hit, flags=flags, **params)
    assert_bits(got, ref, case)
    if flags:
        return
    moving = velocity_ref(src, motion, hit, **params)[4]
    assert_bits(got[~moving], src[~moving], "pass-through pixels are copied")
    assert np.isfinite(got[moving][:, :3]).all(), "a moving pixel never takes a colour that is none, and no sum overflows"
    if case in ("all_still", "shutter_closed", "pan_below_half_a_pixel"):
        assert_bits(got, src, "nothing moves half a pixel: a copy")
    elif case == "one_fast_pixel":
        assert_bits(got[:, :16], src[:, :16], "two tiles away")
        assert_bits(got[:, 64:], src[:, 64:], "two tiles away")
        assert not np.array_equal(bits(got[16:32, 48:64]), bits(src[16:32, 48:64]))
    elif case == "still_foreground":
        inside = cases.still_disc_over_pan()[3]
        assert_bits(got[inside], src[inside], "the still disc stays sharp")
    elif case == "colours_at_2_100":
        assert (np.abs(got[..., :3]) <= 2.0 ** 100 * (1 + 2.0 ** -16)).all() and not np.array_equal(bits(got), bits(src))
    else:
        assert not np.array_equal(bits(got), bits(src))


def test_params_null_means_the_defaults(gpu_ctx):
    w, h = 33, 31
    src, motion, hit = cases.image(w, h), cases.pan(w, h, 20.0, -8.0), cases.hit_image(w, h)
    with Quad(gpu_ctx, w, h, src, motion, hit) as (s, m, z, d):
        assert gpu_ctx.lib.urt_motion_blur(gpu_ctx._h, s.handle, m.handle, z.handle, d.handle, None) == 0
        assert_bits(d.GetPixels(), motion_blur_ref(src, motion, hit), "params == NULL")
        assert gpu_ctx.lib.urt_motion_blur(gpu_ctx._h, s.handle, s.handle, s.handle, d.handle, None) == 0   # the inputs may be one another
        assert_bits(d.GetPixels(), motion_blur_ref(src, src, src), "src as motion and hit")


# ---- 3. external textures, the scratch -------------------------------------------------------------------------------------------------
GUARD = 3                                                                    # rows of the output's width before and after it


def test_external_textures_and_nothing_outside_them(gpu_ctx):
    import torch
    w, h = 33, 31
    ctx, dev = gpu_ctx, torch.device("cuda", gpu_ctx.device)
    src, motion, hit = cases.image(w, h), cases.random_motion(w, h), cases.hit_image(w, h)
    filled = np.random.default_rng(7).uniform(-9, -1, (4, h + 2 * GUARD, w, 4)).astype(F)
    for k, px in enumerate((src, motion, hit)):
        filled[k, GUARD:GUARD + h] = px
    pattern = torch.from_numpy(filled).to(dev)
    ext = pattern.clone()
    torch.cuda.synchronize(dev)
    tex = [RenderTexture(ctx, w, h, external_ptr=ext[k, GUARD].data_ptr()) for k in range(4)]
    try:
        for flags in (0, FLAG_VELOCITY):
            ctx.motion_blur(*tex, shutter=1.0, flags=flags)
            ctx.synchronize()
            got, keep = ext.cpu().numpy(), pattern.cpu().numpy()
            assert_bits(got[3, GUARD:GUARD + h], motion_blur_ref(src, motion, hit, shutter=1.0, flags=flags), f"external dst flags={flags}")
            assert got[:3].tobytes() == keep[:3].tobytes(), "the inputs and their guards"
            assert got[3, :GUARD].tobytes() == keep[3, :GUARD].tobytes() and got[3, GUARD + h:].tobytes() == keep[3, GUARD + h:].tobytes()
    finally:
        for t in tex:
            t.Release()


def scratch_bytes(w, h):
    return 4 * (4 * ((w + 15) // 16) * ((h + 15) // 16) + 2 * w * h)             # csrc/motion_blur.h motion_blur_scratch_floats


def test_the_scratch_grows_once_and_is_reused_across_sizes(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        largest = 0
        for k, (w, h) in enumerate([(17, 16), (70, 50), (1, 40), (70, 50), (33, 31)]):
            with Quad(ctx, w, h, cases.image(w, h), cases.random_motion(w, h), cases.hit_image(w, h)) as (src, motion, hit, dst):
                held = live_resources()["device_bytes"]
                ctx.motion_blur(src, motion, hit, dst, shutter=1.0)
                grown = live_resources()["device_bytes"] - held
                assert grown == max(scratch_bytes(w, h) - largest, 0), (k, w, h)                 # the old scratch is given back when it grows
                largest = max(largest, scratch_bytes(w, h))
                assert_bits(dst.GetPixels(), random_reference(w, h, 16.0), f"call {k} at {w} x {h}")


def test_calls_back_to_back_share_the_scratch_in_order(gpu_ctx):
    ctx = gpu_ctx
    a = (cases.image(70, 50), cases.random_motion(70, 50), cases.hit_image(70, 50))
    b = (cases.image(33, 31), cases.random_motion(33, 31), cases.hit_image(33, 31))
    with Quad(ctx, 70, 50, *a) as (src, motion, hit, dst), Quad(ctx, 33, 31, *b) as (src2, motion2, hit2, dst2):
        ctx.motion_blur(src, motion, hit, dst, shutter=1.0)
        ctx.motion_blur(src2, motion2, hit2, dst2, shutter=1.0, max_radius=4.0)   # the same scratch, no synchronisation in between
        ctx.motion_blur(dst, motion, hit, src, shutter=0.5)                       # and the first result, streaked again
        assert_bits(dst2.GetPixels(), random_reference(33, 31, 4.0), "second call")
        once = random_reference(70, 50, 16.0)
        assert_bits(dst.GetPixels(), once, "first call")
        assert_bits(src.GetPixels(), motion_blur_ref(once, a[1], a[2], shutter=0.5), "third call on the first's result")


# ---- 4. RayTraceMaster ------------------------------------------------------------------------------------------------------------------
def sample_centre_hit(m, w, h):
    """urt_render_aov's hit target through the centres of the frames' samples (RayTraceMaster._sample_centre_projection restated), the
    host's matrix bound again afterwards; -> a texture the caller releases."""
    p = np.array(m.scene.camera_inverse_projection, dtype=F).reshape(16).copy()
    p[12:16] += p[0:4] * F(1.0 / w) + p[4:8] * F(1.0 / h)
    tex = RenderTexture(m.ctx, w, h)
    m.RayTraceShader.SetMatrix("_CameraInverseProjection", p)
    m.ctx.render_aov(hit=tex)
    m.RayTraceShader.SetMatrix("_CameraInverseProjection", m.scene.camera_inverse_projection)
    return tex


@pytest.mark.parametrize("stages", ["plain", "dof_bloom"])
def test_master_streaks_the_frame_after_an_edit_and_not_the_still_view(gpu_ctx, stages):
    w, h = 64, 48
    sc = scenes.mixed_test_scene(w, h)
    dof = {"focus_distance": 6.0, "scale": 3.0, "max_radius": 4.0}
    bloom = {"threshold": 0.25, "intensity": 0.5}
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, sc)
        with pytest.raises(ValueError):
            m.EnableMotionBlur()                                                  # no temporal accumulation, no motion vectors
        m.EnableTemporalAccumulation()
        held = live_resources()
        m.EnableMotionBlur(shutter=1.0)
        assert live_resources() == held and m._mbMotion is None                   # EnableMotionBlur creates nothing
        if stages == "dof_bloom":
            m.EnableDepthOfField(**dof)
            m.EnableBloom(**bloom)
        for _ in range(4):
            m.OnRenderImage()
        mine = [RenderTexture(ctx, w, h) for _ in range(5)]
        color, count, motion, tmp, out = mine

        def chain(streak):
            """The presented frame assembled from Context calls -> pixels."""
            hit = sample_centre_hit(m, w, h)
            source = m._converged
            if stages == "dof_bloom":
                ctx.depth_of_field(source, hit, tmp if streak else out, **dof)
                source = tmp if streak else out
            if streak:
                ctx.motion_blur(source, motion, hit, out, shutter=1.0)
                source = out
            if stages == "dof_bloom":
                ctx.bloom(source, out, None, **bloom)
                source = out
            ctx.tonemap(source, out, None, op="aces", exposure=1.0, white=4.0)
            px = out.GetPixels()
            hit.Release()
            return px

        assert_bits(m.ToneMap().GetPixels(), chain(False), "before any edit: no streak")
        # the edit: one sphere moves to the right; the reprojection of the edit is repeated by hand, motion image included
        prev_m = scenes.world_to_clip(sc.camera_to_world, sc.camera_inverse_projection)
        k = 0                                                                     # the large sphere near the camera
        m.MoveObjects(None, {k: (sc.spheres[k]["position"] + np.array([1.2, 0.0, 0.0], F), sc.spheres[k]["radius"])})
        assert m._mbAge == 0 and (m._mbMotion.width, m._mbMotion.height) == (w, h)
        ctx.reproject(*m._tspare, *m._taov[0], *m._taov[1], color, count, prev_m, motion=motion, mesh_motion=m._tmotion[0],
                      sphere_motion=m._tmotion[1], moved_max_history=m._moved_max_history, **m._temporal)
        assert_bits(m._converged.GetPixels(), color.GetPixels(), "the reprojected history")
        vectors = motion.GetPixels()
        assert_bits(m._mbMotion.GetPixels(), vectors, "the motion image this master owns")
        valid = vectors[..., 2] > 0
        assert valid.any() and np.hypot(vectors[..., 0], vectors[..., 1])[valid].max() > 2.0   # the sphere moved by pixels
        m.OnRenderImage()
        assert m._mbAge == 1
        conv = m._converged.GetPixels()
        streaked = m.ToneMap().GetPixels()
        assert_bits(streaked, chain(True), "the frame after the edit: the chain with the streak")
        assert not np.array_equal(bits(streaked), bits(chain(False)))
        assert_bits(m._converged.GetPixels(), conv, "_converged is never modified")
        # a second frame without an edit: the motion is two frames old, the view is still
        m.OnRenderImage()
        assert m._mbAge == 2
        assert_bits(m.ToneMap().GetPixels(), chain(False), "a still view presents unblurred")
        # an edit again, then the stage off
        m.MoveObjects(None, {k: (sc.spheres[k]["position"] - np.array([1.2, 0.0, 0.0], F), sc.spheres[k]["radius"])})
        m.OnRenderImage()
        motion.SetPixels(m._mbMotion.GetPixels())
        assert_bits(m.ToneMap().GetPixels(), chain(True), "the second edit")
        m.DisableMotionBlur()
        assert_bits(m.ToneMap().GetPixels(), chain(False), "DisableMotionBlur")
        for t in mine:
            t.Release()
        m.OnDisable()
        assert m._mbMotion is None and m._mbStage is None and m._dofHit is None


def test_everything_is_given_back(gpu_ctx):
    def once():
        with Context(gpu_ctx.device) as ctx:
            sc = scenes.mixed_test_scene(32, 24)
            m = RayTraceMaster(ctx, sc)
            m.EnableTemporalAccumulation()
            m.EnableMotionBlur()
            m.EnableDepthOfField()
            m.OnRenderImage()
            m.MoveObjects(None, {0: (sc.spheres[0]["position"] + F(0.2), sc.spheres[0]["radius"])})
            m.OnRenderImage()
            m.ToneMap()
            m.OnDisable()
    once()
    before = live_resources()
    once()
    assert live_resources() == before


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
ARG, HANDLE = 1, 2
MB_OK = {"shutter": 0.5, "max_radius": 16.0, "flags": 0, "reserved": 0}
# name -> (expected code, call changes: src / motion / hit / dst, params changes)
MB_ERRORS = {
    "shutter_negative": (ARG, {}, {"shutter": -1e-6}), "shutter_above_1": (ARG, {}, {"shutter": 1.0001}),
    "shutter_nan": (ARG, {}, {"shutter": NAN}), "shutter_inf": (ARG, {}, {"shutter": INF}), "shutter_minus_inf": (ARG, {}, {"shutter": -INF}),
    "radius_below_half": (ARG, {}, {"max_radius": 0.49}), "radius_zero": (ARG, {}, {"max_radius": 0.0}),
    "radius_above_16": (ARG, {}, {"max_radius": 16.001}), "radius_nan": (ARG, {}, {"max_radius": NAN}), "radius_inf": (ARG, {}, {"max_radius": INF}),
    "flags_unknown_bit": (ARG, {}, {"flags": 2}), "flags_high_bit": (ARG, {}, {"flags": -2147483648}),
    "flags_unknown_bit_with_velocity": (ARG, {}, {"flags": 3}),
    "reserved_set": (ARG, {}, {"reserved": 1}), "reserved_negative": (ARG, {}, {"reserved": -1}),
    "dst_size": (ARG, {"dst": "odd"}, {}), "src_size": (ARG, {"src": "odd"}, {}), "motion_size": (ARG, {"motion": "odd"}, {}),
    "hit_size": (ARG, {"hit": "odd"}, {}),
    "dst_is_src": (ARG, {"dst": "src"}, {}), "dst_is_motion": (ARG, {"dst": "motion"}, {}), "dst_is_hit": (ARG, {"dst": "hit"}, {}),
    "dst_is_src_with_velocity": (ARG, {"dst": "src"}, {"flags": 1}),
    "dst_is_sky": (ARG, {"dst": "sky"}, {}),
    "src_zero": (HANDLE, {"src": 0}, {}), "motion_zero": (HANDLE, {"motion": 0}, {}), "hit_zero": (HANDLE, {"hit": 0}, {}),
    "dst_zero": (HANDLE, {"dst": 0}, {}),
    "src_unknown": (HANDLE, {"src": 987654}, {}), "motion_unknown": (HANDLE, {"motion": 987654}, {}), "hit_unknown": (HANDLE, {"hit": 987654}, {}),
    "dst_unknown": (HANDLE, {"dst": 987654}, {}),
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
        tex = {n: RenderTexture(ctx, W, H) for n in ("src", "motion", "hit", "dst", "sky")}
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
    d = {"ctx": ctx._h, **{n: tex[n].handle for n in ("src", "motion", "hit", "dst")}}
    for n, v in changes.items():
        d[n] = gone_h if v == "gone" else tex[v].handle if isinstance(v, str) else v
    p = None if params == "null" else C.byref(_lib.MotionBlurParams(*({**MB_OK, **params}[k] for k in MB_OK)))
    return ctx.lib.urt_motion_blur(d["ctx"], d["src"], d["motion"], d["hit"], d["dst"], p)


@pytest.mark.parametrize("case", sorted(MB_ERRORS))
def test_errors_write_nothing_and_allocate_nothing(error_rig, case):
    code, changes, params = MB_ERRORS[case]
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
    assert_bits(tex["dst"].GetPixels(), motion_blur_ref(snap["src"], snap["motion"], snap["hit"]), "defaults")
    assert live_resources()["device_bytes"] - held == scratch_bytes(16, 8)
    assert error_call(error_rig, {"hit": "src", "motion": "src"}, {"flags": 1, "shutter": 1.0}) == 0   # the inputs are only read
    assert_bits(tex["dst"].GetPixels(), motion_blur_ref(snap["src"], snap["src"], snap["src"], shutter=1.0, flags=1), "hit == motion == src")
    assert error_call(error_rig, {"src": "sky"}, {"shutter": 1.0, "max_radius": 4.0}) == 0   # the sky may be read
    assert_bits(tex["dst"].GetPixels(), motion_blur_ref(snap["sky"], snap["motion"], snap["hit"], shutter=1.0, max_radius=4.0), "from the sky")
    for n in ("src", "motion", "hit", "sky", "odd"):
        assert tex[n].GetPixels().tobytes() == snap[n].tobytes(), n              # the inputs are only read
    assert ctx.counters() == counters


# the height limit of the 16-row tiles (65535 rows of workgroups): textures of their own, 16 MB each
TALLEST = 16 * 65535


def test_textures_taller_than_the_grid_are_refused_and_the_tallest_are_served(gpu_ctx):
    """1 x 1048561 is an error like the others: nothing written, nothing allocated.  1 x 1048560 is served: a pan along x on an image one
    pixel wide has every tap but the own one outside the image, w = 1 / l_p with l_p = 0.25 * 16 = 4, and (c / 4) / (1 / 4) = c exactly
    (powers of two) — a closed form that needs no restatement at this size."""
    rng = np.random.default_rng(8)
    with Context(gpu_ctx.device) as ctx:
        for height, code in ((TALLEST + 1, ARG), (TALLEST, 0)):
            src_px = np.exp2(rng.uniform(-6, 6, (height, 1, 4))).astype(F)
            hit_px = np.exp2(rng.uniform(-2, 6, (height, 1, 4))).astype(F)
            motion_px = np.zeros((height, 1, 4), F)
            motion_px[..., 0], motion_px[..., 2] = 16.0, 1.0
            sentinel = np.full((height, 1, 4), SENTINEL, U).view(F)
            with Quad(ctx, 1, height, src_px, motion_px, hit_px) as (src, motion, hit, dst):
                dst.SetPixels(sentinel)
                for t in (src, motion, hit, dst):
                    t.GetPixels()                                                # (whatever a readback keeps is held from here on)
                held = live_resources()["device_bytes"]
                assert ctx.lib.urt_motion_blur(ctx._h, src.handle, motion.handle, hit.handle, dst.handle, None) == code
                ctx.synchronize()
                grown = live_resources()["device_bytes"] - held
                if code:
                    assert dst.GetPixels().tobytes() == sentinel.tobytes() and grown == 0
                else:
                    assert_bits(dst.GetPixels(), src_px, "1 x 1048560, a pan across the only column")
                    assert grown == scratch_bytes(1, height)
