"""GPU: temporal reprojection (include/urt.h urt_reproject, urt_blit_add_history) — bit for bit against the float32 restatement of
tests/reproject_ref.py on analytic feature buffers with injected bad texels and on real renders, the blend against urt_blit_add and the
reference, deferred and fused blends against submitted ones, ordering with read-backs, counters and unrelated textures, the temporal-off
camera move, argument errors, and the quality gain over a fresh frame after a small camera move."""
import ctypes as C

import numpy as np
import pytest

from reproject_ref import analytic_aovs, blit_add_history_ref, reproject_ref
from unityraytracer_amd import Context, RayTraceMaster, _lib, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, ref, what):
    g, r = u32(got), u32(ref)
    bad = g != r
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} texels differ, first at {np.argwhere(bad)[0]}: {got[tuple(np.argwhere(bad)[0][:2])]} " \
                          f"vs {ref[tuple(np.argwhere(bad)[0][:2])]}"


# ---- 1. random inputs ------------------------------------------------------------------------------------------------------------------
POSES = {"move": (dict(), dict(position=(0.35, 1.2, -9.6), yaw_deg=4.0)),
         "behind": (dict(position=(0.0, 1.0, 4.0)), dict()),                   # most surface points lie behind the previous camera
         "still": (dict(), dict())}


def random_case(seed, w, h, pose):
    rng = np.random.default_rng(seed)
    pa, pb = POSES[pose]
    cam_a, cam_b = scenes.camera_matrices(w, h, **pa), scenes.camera_matrices(w, h, **pb)
    prev = [a.copy() for a in analytic_aovs(w, h, *cam_a)]
    cur = [a.copy() for a in analytic_aovs(w, h, *cam_b)]
    color = (10.0 ** rng.uniform(-3, 2, (h, w, 4))).astype(F)
    count = np.zeros((h, w, 4), F)
    count[..., 0] = rng.choice([0.0, 1.0, 3.5, 17.0, 64.0, 200.0], (h, w))
    count[..., 1:] = rng.uniform(-1, 1, (h, w, 3))                        # the reserved components are ignored
    def inject(a, p, vals, comps):
        m = rng.random(a.shape[:2]) < p
        a[m, rng.choice(comps, m.sum())] = rng.choice(vals, m.sum())
    bad = [np.nan, np.inf, -np.inf]
    inject(color, 0.02, bad, [0, 1, 2, 3])
    inject(count, 0.02, bad + [-2.0], [0])
    for hit, normal, ids in (prev, cur):
        inject(hit, 0.02, bad + [-1.0, 0.0], [0, 1, 2, 3])
        inject(normal, 0.02, bad, [0, 1, 2])
        inject(normal, 0.02, [1.0, 2.0, 3.0, 0.0, np.nan], [3])             # kind mismatches
        iv = ids.view(np.int32)
        m = rng.random(iv.shape[:2]) < 0.03
        iv[m, 0] += 1                                                     # id mismatches
    return color, count, prev, cur, cam_a, cam_b


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (67, 33), (200, 120)])
@pytest.mark.parametrize("pose", sorted(POSES))
def test_random_inputs_match_reference_bit_for_bit(gpu_ctx, size, pose):
    w, h = size
    for k, (mh, motion, nt, pt) in enumerate([(0.0, True, 0.9, 0.02), (1.0, False, 0.5, 0.2), (64.0, True, -1.0, 1e3),
                                              (64.0, False, 0.99, 0.001)]):
        color, count, prev, cur, cam_a, cam_b = random_case(100 * w + 10 * k + len(pose), w, h, pose)
        M = scenes.world_to_clip(*cam_a)
        params = dict(max_history=mh, normal_threshold=nt, plane_threshold=pt)
        got = gpu_ctx.reproject_arrays(color, count, *prev, *cur, M, *cam_b, motion=motion, **params)
        ref = reproject_ref(color, count, *prev, *cur, M, *cam_b, **params)
        what = f"{w}x{h} {pose} mh={mh} motion={motion}"
        assert_bits(got["color"], ref["color"], what + " color")
        assert_bits(got["count"], ref["count"], what + " count")
        if motion:
            assert_bits(got["motion"], ref["motion"], what + " motion")
        if w * h > 100 and pose != "behind":
            assert (ref["count"][..., 0] > 0).mean() > 0.3, what           # the case does exercise history


# ---- 2. real renders -------------------------------------------------------------------------------------------------------------------
def pose_b(sc):
    c2w, invp = scenes.camera_matrices(sc.width, sc.height, position=(0.25, 1.05, -9.8), yaw_deg=3.0)
    return c2w, invp


@pytest.mark.parametrize("cfg", ["mixed", "C1"])
def test_real_renders_match_reference_bit_for_bit(gpu_ctx, cfg):
    sc = scenes.mixed_test_scene(96, 64) if cfg == "mixed" else scenes.config1(256, 256)
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, sc)
        m.EnableTemporalAccumulation()
        for _ in range(16):
            m.OnRenderImage()
        cam_a = (sc.camera_to_world.copy(), sc.camera_inverse_projection.copy())
        hist_color, hist_count = m._converged.GetPixels(), m._tcount.GetPixels()
        assert (hist_count[..., 0] == 16).all()
        c2w_b, invp_b = pose_b(sc)
        m.MoveCamera(c2w_b, invp_b)
        prev = [t.GetPixels() for t in m._taov[0]]
        cur = [t.GetPixels() for t in m._taov[1]]
        got_c, got_n = m._converged.GetPixels(), m._tcount.GetPixels()
        ref = reproject_ref(hist_color, hist_count, *prev, *cur, scenes.world_to_clip(*cam_a), c2w_b, invp_b,
                            **{k: v for k, v in m._temporal.items()})
        assert_bits(got_c, ref["color"], cfg + " color")
        assert_bits(got_n, ref["count"], cfg + " count")
        kept = (ref["count"][..., 0] > 0).mean()
        assert kept > 0.8, kept
        m.OnDisable()


# ---- 3. the blend --------------------------------------------------------------------------------------------------------------------
def test_uniform_count_blend_is_blit_add(gpu_ctx):
    w, h = 37, 23
    rng = np.random.default_rng(3)
    with Context(gpu_ctx.device) as ctx:
        src, a, b, cnt = (RenderTexture(ctx, w, h) for _ in range(4))
        start = rng.uniform(0, 1, (h, w, 4)).astype(F)
        a.SetPixels(start); b.SetPixels(start)
        cnt.SetPixels(np.zeros((h, w, 4), F))
        for k in range(8):
            src.SetPixels(rng.uniform(0, 4, (h, w, 4)).astype(F))
            ctx.blit_add_history(src, a, cnt, 0.0)
            ctx.check(ctx.lib.urt_blit_add(ctx._h, src.handle, b.handle, float(k)))
        assert_bits(a.GetPixels(), b.GetPixels(), "history blend vs blit_add")
        c = cnt.GetPixels()
        assert (c[..., 0] == 8).all() and (c[..., 1:] == 0).all()
        for t in (src, a, b, cnt):
            t.Release()


def test_random_counts_match_reference(gpu_ctx):
    w, h = 53, 31
    rng = np.random.default_rng(4)
    with Context(gpu_ctx.device) as ctx:
        src, dst, cnt = (RenderTexture(ctx, w, h) for _ in range(3))
        for mh in (0.0, 1.0, 2.5, 8.0, 64.0):
            s = rng.uniform(0, 4, (h, w, 4)).astype(F)
            d = rng.uniform(0, 4, (h, w, 4)).astype(F)
            n = np.zeros((h, w, 4), F)
            n[..., 0] = rng.choice([0.0, 0.25, 1.0, 5.5, 7.0, 63.0, 100.0, 1e30, np.nan, np.inf, -np.inf, -1.0, -0.0], (h, w))
            n[..., 1:] = 9.0
            src.SetPixels(s); dst.SetPixels(d); cnt.SetPixels(n)
            ctx.blit_add_history(src, dst, cnt, mh)
            rd, rn = blit_add_history_ref(s, d, n, mh)
            assert_bits(dst.GetPixels(), rd, f"mh={mh} dst")
            assert_bits(cnt.GetPixels(), rn, f"mh={mh} count")
        for t in (src, dst, cnt):
            t.Release()


def temporal_run(device, sc, fused, frames=20, max_history=8.0, observe=False):
    with Context(device) as ctx:
        if not fused:
            ctx.set_option("frames_per_launch", 1)
        m = RayTraceMaster(ctx, sc)
        m.EnableTemporalAccumulation(max_history=max_history)
        present = RenderTexture(ctx, sc.width, sc.height)
        seen = []
        for k in range(frames):
            m.OnRenderImage(present)
            if not fused:
                ctx.flush()
            if observe and k in (4, 11):                                  # read-backs straight after deferred frames
                seen.append((m._tcount.GetPixels(), present.GetPixels(), m._converged.GetPixels()))
        out = (m._converged.GetPixels(), m._tcount.GetPixels(), present.GetPixels(), ctx.launch_info(), seen)
        present.Release()
        m.OnDisable()
        return out


def test_fused_deferred_blends_equal_submitted_ones(gpu_ctx):
    sc = scenes.mixed_test_scene(64, 48)
    for mh in (8.0, 0.0):
        a = temporal_run(gpu_ctx.device, sc, True, max_history=mh)
        b = temporal_run(gpu_ctx.device, sc, False, max_history=mh)
        assert a[3]["n_frames"] > 1, a[3]                                  # the fused path was taken
        for x, y, what in zip(a[:3], b[:3], ("colour", "count", "present")):
            assert_bits(x, y, f"mh={mh} {what}")
        assert (a[1][..., 0] == (min(20.0, mh) if mh else 20.0)).all()
        assert_bits(a[2], a[0], "present = converged")


def test_readbacks_see_deferred_blends(gpu_ctx):
    sc = scenes.mixed_test_scene(64, 48)
    seen = temporal_run(gpu_ctx.device, sc, True, frames=12, max_history=0.0, observe=True)[4]
    for (count, present, conv), n in zip(seen, (5, 12)):
        assert (count[..., 0] == n).all(), n
        assert_bits(present, conv, f"present after {n} frames")


# ---- 4. nothing else moves -------------------------------------------------------------------------------------------------------------
def test_counters_and_unrelated_textures_unchanged(gpu_ctx):
    sc = scenes.mixed_test_scene(48, 32)
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        m = RayTraceMaster(ctx, sc)
        m.EnableTemporalAccumulation()
        bystander = RenderTexture(ctx, 48, 32)
        marks = np.random.default_rng(5).uniform(0, 1, (32, 48, 4)).astype(F)
        bystander.SetPixels(marks)
        for _ in range(3):
            m.OnRenderImage()
        m.MoveCamera(*pose_b(sc))
        c0 = ctx.counters()
        spare = RenderTexture(ctx, 48, 32)
        ctx.blit_add_history(m._target, m._converged, m._tcount, 8.0)     # not deferred (no pending frame): enqueued
        prev, cur = m._taov
        ctx.reproject(m._converged, m._tcount, *prev, *cur, m._tspare[0], m._tspare[1], scenes.world_to_clip(*pose_b(sc)), motion=spare)
        ctx.synchronize()
        assert ctx.counters() == c0
        assert bystander.GetPixels().tobytes() == marks.tobytes()
        for t in (bystander, spare):
            t.Release()
        m.OnDisable()


def test_temporal_off_move_is_the_reference_reset(gpu_ctx):
    sc_a, sc_b = scenes.mixed_test_scene(64, 48), scenes.mixed_test_scene(64, 48)
    c2w, invp = pose_b(sc_a)
    out = []
    for use_move, sc in ((True, sc_a), (False, sc_b)):
        with Context(gpu_ctx.device) as ctx:
            m = RayTraceMaster(ctx, sc)
            for _ in range(5):
                m.OnRenderImage()
            if use_move:
                m.MoveCamera(c2w, invp)
            else:
                sc.camera_to_world, sc.camera_inverse_projection = c2w, invp
                m.ResetAccumulation()
            for _ in range(3):
                m.OnRenderImage()
            out.append((m._target.GetPixels(), m._converged.GetPixels()))
            m.OnDisable()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(gpu_ctx):
    w, h = 16, 8
    rng = np.random.default_rng(6)
    with Context(gpu_ctx.device) as ctx:
        lib, hd = ctx.lib, ctx._h
        names = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color", "count", "motion")
        tex = {n: RenderTexture(ctx, w, h) for n in names}
        small, sky, extra = RenderTexture(ctx, 8, 8), RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
        snap = {}
        for n, t in list(tex.items()) + [("sky", sky), ("extra", extra)]:
            a = rng.uniform(-2, 2, (h, w, 4)).astype(F)
            t.SetPixels(a)
            snap[n] = a
        gone = RenderTexture(ctx, w, h)
        gone_h = gone.handle
        gone.Release()
        H = {n: t.handle for n, t in tex.items()}

        def images(**ch):
            d = dict(H)
            d.update(ch)
            return C.byref(_lib.ReprojectImages(*(d[n] for n in names)))

        M = (C.c_float * 16)(*np.eye(4, dtype=F).reshape(16).tolist())

        def params(mh=64.0, nt=0.9, pt=0.02, flags=0):
            return C.byref(_lib.ReprojectParams(M, mh, nt, pt, flags))

        nan = float("nan")
        # no camera matrices bound yet
        assert lib.urt_reproject(hd, images(), params()) == 5                               # URT_ERR_UNBOUND
        c2w, invp = scenes.camera_matrices(w, h)
        sh = ComputeShader(ctx)
        sh.SetMatrix("_CameraToWorld", c2w)
        sh.SetMatrix("_CameraInverseProjection", invp)
        sh.SetTexture(0, "_SkyboxTexture", sky)
        cases = [
            ((None, params()), 1), ((images(), None), 1),
            ((images(), params(flags=1)), 1), ((images(), params(nt=nan)), 1), ((images(), params(pt=nan)), 1),
            ((images(), params(mh=nan)), 1), ((images(), params(mh=-1.0)), 1), ((images(), params(mh=0.5)), 1),
            ((images(prev_hit=small.handle), params()), 1), ((images(motion=small.handle), params()), 1),
            ((images(color=H["prev_color"]), params()), 1), ((images(count=H["id"]), params()), 1),
            ((images(motion=H["color"]), params()), 1), ((images(count=H["color"]), params()), 1),
            ((images(color=sky.handle), params()), 1), ((images(motion=sky.handle), params()), 1),
            ((images(prev_color=0), params()), 2), ((images(id=0), params()), 2), ((images(count=0), params()), 2),
            ((images(normal=987654), params()), 2), ((images(motion=987654), params()), 2), ((images(color=gone_h), params()), 2),
        ]
        for args, code in cases:
            assert lib.urt_reproject(hd, *args) == code, (args, code)
        s, d, c = H["prev_color"], H["color"], H["count"]
        for args, code in [((s, d, c, nan), 1), ((s, d, c, -1.0), 1), ((s, d, c, 0.5), 1), ((s, s, c, 0.0), 1), ((s, d, s, 0.0), 1),
                           ((s, d, d, 0.0), 1), ((s, small.handle, c, 0.0), 1), ((s, d, small.handle, 0.0), 1), ((s, sky.handle, c, 0.0), 1),
                           ((s, d, sky.handle, 0.0), 1), ((0, d, c, 0.0), 2), ((s, 0, c, 0.0), 2), ((s, d, 0, 0.0), 2),
                           ((s, d, gone_h, 0.0), 2), ((987654, d, c, 0.0), 2)]:
            assert lib.urt_blit_add_history(hd, *args) == code, (args, code)
        assert lib.urt_reproject(None, images(), params()) == 1
        assert lib.urt_blit_add_history(None, s, d, c, 0.0) == 1
        for n, t in list(tex.items()) + [("sky", sky), ("extra", extra)]:
            assert t.GetPixels().tobytes() == snap[n].tobytes(), n
        assert lib.urt_reproject(hd, images(), params()) == 0                               # and valid calls do write
        assert lib.urt_blit_add_history(hd, H["prev_color"], extra.handle, H["motion"], 0.0) == 0
        assert tex["color"].GetPixels().tobytes() != snap["color"].tobytes()
        assert extra.GetPixels().tobytes() != snap["extra"].tobytes()
        sh.SetTexture(0, "_SkyboxTexture", None)
        for t in list(tex.values()) + [small, sky, extra]:
            t.Release()


# ---- 6. quality ------------------------------------------------------------------------------------------------------------------------
def quality(ctx, frames=64, ref_frames=1024):
    """(surface MSE of the reprojected history plus one frame, that of a fresh one-frame image, surface mask, counts before / after the
    frame), against a ref_frames accumulation at the new pose, mixed scene at 128 x 96, a 0.1-unit move plus 1 degree of yaw."""
    w, h = 128, 96
    c2w_b, invp_b = scenes.camera_matrices(w, h, position=(0.1, 1.0, -10.0), yaw_deg=1.0)
    ref_sc = scenes.mixed_test_scene(w, h)
    ref_sc.camera_to_world, ref_sc.camera_inverse_projection = c2w_b, invp_b
    ref_m = RayTraceMaster(ctx, ref_sc, frame_seed=0xBEEF)
    for _ in range(ref_frames):
        ref_m.OnRenderImage()
    ref = ref_m._converged.GetPixels()[..., :3].astype(np.float64)
    normal = ref_m.RenderFeatureBuffers()[1].GetPixels()
    ref_m.OnDisable()
    fresh_sc = scenes.mixed_test_scene(w, h)
    fresh_sc.camera_to_world, fresh_sc.camera_inverse_projection = c2w_b, invp_b
    fresh_m = RayTraceMaster(ctx, fresh_sc, frame_seed=0x0F1E)
    fresh_m.OnRenderImage()
    fresh = fresh_m._converged.GetPixels()[..., :3].astype(np.float64)
    fresh_m.OnDisable()
    sc = scenes.mixed_test_scene(w, h)
    m = RayTraceMaster(ctx, sc)
    m.EnableTemporalAccumulation()
    for _ in range(frames):
        m.OnRenderImage()
    m.MoveCamera(c2w_b, invp_b)
    before = m._tcount.GetPixels()[..., 0]
    m.OnRenderImage()
    after = m._tcount.GetPixels()[..., 0]
    temporal = m._converged.GetPixels()[..., :3].astype(np.float64)
    m.OnDisable()
    surf = normal[..., 3] != 0
    mse = lambda a: float(((a - ref)[surf] ** 2).mean())  # noqa: E731
    return mse(temporal), mse(fresh), surf, before, after


def test_quality_after_a_small_camera_move(gpu_ctx):
    with Context(gpu_ctx.device) as ctx:
        t, f, surf, before, after = quality(ctx)
    print(f"temporal quality: surface MSE reprojected+1 {t:.4e}, fresh 1-frame {f:.4e}, ratio {f / t:.1f}x; "
          f"pixels with history {float((before > 0).mean()):.3f}")
    assert surf.mean() > 0.3
    assert f >= 10.0 * t, (t, f)                                         # measured 35x (DESIGN.md "Temporal reprojection")
    assert (after[before == 0] == 1).all()                               # disoccluded pixels start over
    assert (before > 0).mean() > 0.8
    assert (after[before > 0] == np.minimum(before[before > 0], 63.0) + 1).all()
