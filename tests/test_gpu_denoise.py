"""GPU: the edge-aware a-trous denoiser (include/urt.h urt_denoise) — against the float64 restatement of tests/denoise_ref.py on random
inputs (pass-through texels and alpha bit for bit), no bleed across normal edges, quality on real renders against a 1024-frame
accumulation, ordering with deferred frames, determinism, in-place use, unchanged frames and counters, external textures, scratch
regrowth and argument errors."""
import numpy as np
import pytest

from denoise_ref import denoise_ref, surface_mask
from unityraytracer_amd import Context, RayTraceMaster, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

pytestmark = pytest.mark.gpu

F = np.float32


def random_inputs(seed, w, h, miss=0.1, bad_color=0.02):
    """HDR colours up to 1e3 (log-uniform), random unit normals, depths 0.5..50, albedos with a few NaN channels, ~10 % miss pixels
    (the urt_render_aov miss texels) and a few NaN / inf colours."""
    rng = np.random.default_rng(seed)
    color = np.empty((h, w, 4), F)
    color[..., :3] = 10.0 ** rng.uniform(-3, 3, (h, w, 3))
    color[..., 3] = rng.uniform(0, 1, (h, w))
    bad = rng.random((h, w)) < bad_color
    color[bad, rng.integers(0, 3, bad.sum())] = rng.choice([np.nan, np.inf, -np.inf], bad.sum())
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normal = np.concatenate([n, rng.integers(1, 4, (h, w, 1))], -1).astype(F)
    hit = np.concatenate([rng.uniform(-10, 10, (h, w, 3)), rng.uniform(0.5, 50, (h, w, 1))], -1).astype(F)
    albedo = np.concatenate([rng.uniform(0, 1, (h, w, 3)), rng.uniform(0, 1, (h, w, 1))], -1).astype(F)
    albedo[..., :3][rng.random((h, w, 3)) < 0.01] = 0
    nan_alb = rng.random((h, w)) < 0.01
    albedo[nan_alb, 0] = np.nan
    m = rng.random((h, w)) < miss
    normal[m] = 0.0
    hit[m] = (0, 0, 0, np.inf)
    albedo[m, :3] = rng.uniform(0, 5, (m.sum(), 3))                    # a miss's albedo texel is the sky radiance
    return color, hit, normal, albedo


def assert_matches_reference(got, color, hit, normal, albedo, what, **params):
    ref = denoise_ref(color, hit, normal, albedo, **params)
    surf = surface_mask(color, hit, normal, albedo)
    assert got.view(np.uint32)[~surf].tobytes() == color.view(np.uint32)[~surf].tobytes(), f"{what}: pass-through texels"
    assert got[..., 3].view(np.uint32).tobytes() == color[..., 3].view(np.uint32).tobytes(), f"{what}: alpha"
    g, r = got[..., :3][surf].astype(np.float64), ref[..., :3][surf]
    err = np.abs(g - r) / (1 + np.abs(r))
    assert np.isfinite(g).all() and err.max(initial=0) <= 1e-4, f"{what}: max relative error {err.max(initial=0):.3e}"


SIGMAS = {"all": dict(sigma_color=50.0, sigma_normal=0.5, sigma_depth=0.3),
          "color_only": dict(sigma_color=20.0, sigma_normal=0.0, sigma_depth=0.0),
          "normal_only": dict(sigma_color=0.0, sigma_normal=0.3, sigma_depth=-1.0),
          "depth_only": dict(sigma_color=-2.0, sigma_normal=0.0, sigma_depth=0.1),
          "none": dict(sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0)}


# ---- 1. against the float64 reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (7, 5), (67, 33)])
@pytest.mark.parametrize("sig", sorted(SIGMAS))
def test_matches_reference_small(gpu_ctx, size, sig):
    w, h = size
    for it in range(1, 6):
        color, hit, normal, albedo = random_inputs(1000 * w + 10 * it + len(sig), w, h)
        for alb in (None, albedo):
            got = gpu_ctx.denoise_arrays(color, hit, normal, alb, iterations=it, **SIGMAS[sig])
            assert_matches_reference(got, color, hit, normal, alb, f"{w}x{h} it={it} {sig} albedo={alb is not None}", iterations=it,
                                     **SIGMAS[sig])


@pytest.mark.parametrize("case", [(5, "all", True), (1, "color_only", False)])
def test_matches_reference_1080p(gpu_ctx, case):
    it, sig, with_albedo = case
    color, hit, normal, albedo = random_inputs(7 + it, 1920, 1080)
    alb = albedo if with_albedo else None
    got = gpu_ctx.denoise_arrays(color, hit, normal, alb, iterations=it, **SIGMAS[sig])
    assert_matches_reference(got, color, hit, normal, alb, f"1080p it={it} {sig}", iterations=it, **SIGMAS[sig])


def test_defaults_are_the_documented_ones(gpu_ctx):
    """params == NULL and Context.denoise's defaults are the same filter."""
    color, hit, normal, albedo = random_inputs(3, 40, 24)
    h, w = color.shape[:2]
    tex = [RenderTexture(gpu_ctx, w, h) for _ in range(6)]
    for t, a in zip(tex, (color, hit, normal, albedo)):
        t.SetPixels(a)
    gpu_ctx.denoise(tex[0], tex[4], tex[1], tex[2], tex[3])
    assert gpu_ctx.lib.urt_denoise(gpu_ctx._h, tex[0].handle, tex[5].handle, tex[1].handle, tex[2].handle, tex[3].handle, None) == 0
    a, b = tex[4].GetPixels(), tex[5].GetPixels()
    assert a.tobytes() == b.tobytes()
    assert_matches_reference(a, color, hit, normal, albedo, "defaults")
    for t in tex:
        t.Release()


# ---- 2. no bleed across an edge ------------------------------------------------------------------------------------------------------
def test_no_bleed_across_normal_edges(gpu_ctx):
    w, h = 48, 40
    rng = np.random.default_rng(5)
    color = np.concatenate([rng.uniform(0, 1, (h, w, 3)), np.ones((h, w, 1))], -1).astype(F)
    left = np.zeros((h, w), bool)
    left[:, : w // 2 - 3] = True
    left[h // 3:, : w // 2 + 5] = True                                    # an L-shaped region, so the edge has a corner
    color[left, :3] += 10.0                                               # a bright region beside a dark one
    normal = np.where(left[..., None], np.array([0, 1, 0, 3], F), np.array([1, 0, 0, 3], F)).astype(F)
    hit = np.concatenate([rng.uniform(-1, 1, (h, w, 3)), np.full((h, w, 1), 4.0)], -1).astype(F)
    params = dict(iterations=5, sigma_color=0.0, sigma_normal=0.1, sigma_depth=0.0)
    both = gpu_ctx.denoise_arrays(color, hit, normal, **params)
    for region in (left, ~left):
        alone_normal = normal.copy()
        alone_normal[~region, 3] = 0                                      # the other region passes through: never a tap
        alone = gpu_ctx.denoise_arrays(color, hit, alone_normal, **params)
        g, r = both[region][:, :3].astype(np.float64), alone[region][:, :3].astype(np.float64)
        assert (np.abs(g - r) <= 1e-4 * (1 + np.abs(r))).all()
    assert (both[left][:, :3] > 9.0).all() and (both[~left][:, :3] < 2.0).all()


# ---- 3. quality on real renders ------------------------------------------------------------------------------------------------------
def quality_ratio(ctx, sc, frames=4, ref_frames=1024, **params):
    """(surface-pixel MSE of Denoise() after `frames` frames, that of the `frames`-frame mean), both against a `ref_frames` accumulation
    of the same camera."""
    ref_m = RayTraceMaster(ctx, sc, frame_seed=0xBEEF)
    for _ in range(ref_frames):
        ref_m.OnRenderImage()
    ref = ref_m._converged.GetPixels()[..., :3].astype(np.float64)
    ref_m.OnDisable()
    m = RayTraceMaster(ctx, sc)
    for _ in range(frames):
        m.OnRenderImage()
    noisy = m._converged.GetPixels()[..., :3].astype(np.float64)
    den = m.Denoise(**params).GetPixels()[..., :3].astype(np.float64)
    hit, normal = m._aov[0].GetPixels(), m._aov[1].GetPixels()
    surf = surface_mask(m._converged.GetPixels(), hit, normal)
    m.OnDisable()
    assert surf.mean() > 0.3
    mse = lambda a: float(((a - ref)[surf] ** 2).mean())  # noqa: E731
    return mse(den), mse(noisy)


@pytest.mark.parametrize("cfg", ["mixed", "C4"])
def test_quality_against_a_long_accumulation(gpu_ctx, cfg):
    sc = scenes.mixed_test_scene(256, 144) if cfg == "mixed" else scenes.config4(480, 270)
    with Context(gpu_ctx.device) as ctx:
        den, noisy = quality_ratio(ctx, sc)
    print(f"denoise quality {cfg}: surface MSE denoised {den:.4e}, 4-frame mean {noisy:.4e}, ratio {den / noisy:.3f}")
    assert den <= 0.5 * noisy, (cfg, den, noisy, den / noisy)


# ---- 4. ordering and determinism ------------------------------------------------------------------------------------------------------
def test_ordering_determinism_in_place_and_counters(gpu_ctx):
    sc = scenes.mixed_test_scene(96, 64)

    def run(sync_first):
        with Context(gpu_ctx.device) as ctx:
            m = RayTraceMaster(ctx, sc)
            m.OnRenderImage()
            hit, normal, albedo, _ = m.RenderFeatureBuffers()
            for _ in range(3):                                             # deferred Dispatch + Blit frames
                m.OnRenderImage()
            if sync_first:
                ctx.synchronize()
            c0 = ctx.counters() if sync_first else None
            out = RenderTexture(ctx, sc.width, sc.height)
            ctx.denoise(m._converged, out, hit, normal, albedo)
            first = out.GetPixels()
            ctx.denoise(m._converged, out, hit, normal, albedo)            # a second call gives the same bits
            second = out.GetPixels()
            if sync_first:
                ctx.synchronize()
                assert ctx.counters() == c0                               # counters untouched
            conv = m._converged.GetPixels()
            ctx.denoise(m._converged, m._converged, hit, normal, albedo)   # in place
            in_place = m._converged.GetPixels()
            out.Release()
            m.OnDisable()
            return first, second, in_place, conv

    a1, a2, a3, conv = run(False)
    b1, b2, b3, _ = run(True)
    assert a1.tobytes() == b1.tobytes(), "denoise after deferred frames differs from denoise after a synchronize"
    assert a1.tobytes() == a2.tobytes() and b1.tobytes() == b2.tobytes(), "two calls differ"
    assert a3.tobytes() == a1.tobytes() and b3.tobytes() == b1.tobytes(), "in place differs from out of place"
    assert a1.tobytes() != conv.tobytes()


def test_frames_unchanged_by_denoise_calls(gpu_ctx):
    sc = scenes.config3(96, 54, slices=60, stacks=47, sky=scenes.make_sky(64, 32))

    def run(with_denoise):
        with Context(gpu_ctx.device) as ctx:
            ctx.set_option("count_stats", 1)
            m = RayTraceMaster(ctx, sc)
            for k in range(6):
                m.OnRenderImage()
                if with_denoise:
                    m.Denoise(iterations=k % 5 + 1)
            img, conv = m._target.GetPixels(), m._converged.GetPixels()
            c = ctx.counters()
            m.OnDisable()
            return img, conv, c

    img0, conv0, c0 = run(False)
    img1, conv1, c1 = run(True)
    assert img0.tobytes() == img1.tobytes() and conv0.tobytes() == conv1.tobytes()
    for k in ("rays", "pixels", "dispatches", "tlas_nodes", "blas_nodes", "hit_sky"):
        assert c0[k] == c1[k], (k, c0[k], c1[k])


def test_counters_unchanged(gpu_ctx):
    sc = scenes.mixed_test_scene(48, 32)
    with Context(gpu_ctx.device) as ctx:
        ctx.set_option("count_stats", 1)
        m = RayTraceMaster(ctx, sc)
        for _ in range(3):
            m.OnRenderImage()
        m.RenderFeatureBuffers()
        c0 = ctx.counters()                                                # submits the deferred frames
        for it in range(1, 6):
            m.Denoise(iterations=it)
        ctx.synchronize()
        assert ctx.counters() == c0
        m.OnDisable()


# ---- 5. external textures and scratch -------------------------------------------------------------------------------------------------
def test_external_dst_and_scratch_regrowth(gpu_ctx):
    import torch
    with Context(gpu_ctx.device) as ctx:
        dev = torch.device("cuda", ctx.device)
        sizes = [(7, 5), (640, 360), (9, 4), (640, 360)]
        for k, (w, h) in enumerate(sizes):                                 # small, large, small again, large again: one scratch grows
            color, hit, normal, albedo = random_inputs(40 + k, w, h)
            tex = [RenderTexture(ctx, w, h) for _ in range(4)]
            for t, a in zip(tex, (color, hit, normal, albedo)):
                t.SetPixels(a)
            ext = torch.full((h, w, 4), -3.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            et = RenderTexture(ctx, w, h, external_ptr=ext.data_ptr())
            own = RenderTexture(ctx, w, h)
            ctx.denoise(tex[0], et, tex[1], tex[2], tex[3], iterations=4, **SIGMAS["all"])
            ctx.denoise(tex[0], own, tex[1], tex[2], tex[3], iterations=4, **SIGMAS["all"])
            ctx.synchronize()
            got = ext.cpu().numpy()
            assert got.tobytes() == own.GetPixels().tobytes(), (w, h)
            assert_matches_reference(got, color, hit, normal, albedo, f"external {w}x{h}", iterations=4, **SIGMAS["all"])
            for t in tex + [et, own]:
                t.Release()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(gpu_ctx):
    from unityraytracer_amd._lib import DenoiseParams
    import ctypes as C
    w, h = 16, 8
    with Context(gpu_ctx.device) as ctx:
        lib, hd = ctx.lib, ctx._h
        color, hit, normal, albedo = random_inputs(9, w, h)
        src, ht, nt, at, dst, small, sky = (RenderTexture(ctx, w, h) for _ in range(7))
        small.Release()
        small = RenderTexture(ctx, 8, 8)
        for t, a in zip((src, ht, nt, at), (color, hit, normal, albedo)):
            t.SetPixels(a)
        sentinel = np.full((h, w, 4), -5.5, F)
        dst.SetPixels(sentinel); sky.SetPixels(sentinel)
        sh = ComputeShader(ctx)
        sh.SetTexture(0, "_SkyboxTexture", sky)
        gone = RenderTexture(ctx, w, h)
        gone_handle = gone.handle
        gone.Release()
        P = lambda it=3, sc=1.0, sn=0.5, sz=0.1: C.byref(DenoiseParams(it, sc, sn, sz))  # noqa: E731
        s, d, hh, n, a = src.handle, dst.handle, ht.handle, nt.handle, at.handle
        for args, code in [
            ((s, hh, hh, n, a, P()), 1), ((s, n, hh, n, a, P()), 1), ((s, a, hh, n, a, P()), 1),     # dst is a guide
            ((s, sky.handle, hh, n, a, P()), 1),                                                     # dst is bound as _SkyboxTexture
            ((s, d, hh, small.handle, a, P()), 1), ((small.handle, d, hh, n, 0, P()), 1),             # sizes differ
            ((s, d, hh, n, a, P(it=0)), 1), ((s, d, hh, n, a, P(it=6)), 1), ((s, d, hh, n, a, P(it=-1)), 1),
            ((s, d, hh, n, a, P(sc=float("nan"))), 1), ((s, d, hh, n, a, P(sn=float("nan"))), 1),
            ((s, d, hh, n, a, P(sz=float("nan"))), 1),
            ((0, d, hh, n, a, P()), 2), ((s, 0, hh, n, a, P()), 2), ((s, d, 0, n, a, P()), 2), ((s, d, hh, 0, a, P()), 2),
            ((987654, d, hh, n, a, P()), 2), ((s, 987654, hh, n, a, P()), 2), ((s, d, 987654, n, a, P()), 2),
            ((s, d, hh, 987654, a, P()), 2), ((s, d, hh, n, 987654, P()), 2), ((s, gone_handle, hh, n, a, P()), 2), ((gone_handle, d, hh, n, a, P()), 2),
        ]:
            assert lib.urt_denoise(hd, *args) == code, (args[:5], code)
        assert lib.urt_denoise(None, s, d, hh, n, a, P()) == 1
        for t in (dst, sky):
            assert t.GetPixels().tobytes() == sentinel.tobytes()
        for t, v in zip((src, ht, nt, at), (color, hit, normal, albedo)):
            assert t.GetPixels().tobytes() == v.tobytes()
        assert lib.urt_denoise(hd, s, d, hh, n, a, P()) == 0                                  # and a valid call does write
        assert dst.GetPixels().tobytes() != sentinel.tobytes()
        sh.SetTexture(0, "_SkyboxTexture", None)
        for t in (src, ht, nt, at, dst, small, sky):
            t.Release()
