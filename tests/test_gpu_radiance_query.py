"""GPU: batched radiance queries (include/urt.h urt_radiance_query / urt_radiance_query_device), bit for bit — pixels mode against the
frame the default kernel renders and, independently of the frame kernels, against the oracle's literal render; rays mode against the
frame's own first rays; one bounce against urt_ray_query, urt_render_aov and the materials' emission; the two kernels (one query per
thread / resident grid with a work counter) against each other; batch shapes, the device form, argument errors, no effect on the frames
and their counters, scene updates, the large-LDS launch, and the master's SampleRadiance / ResamplePixels."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from unityraytracer_amd import Context, RayTraceMaster, scenes
from unityraytracer_amd.unity_api import ComputeShader, RenderTexture

from test_gpu_aov import bind, camera_rays, material_index, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
POX, POY = 0.3125, 0.71875           # a non-zero _PixelOffset


def multi_mesh_scene(w, h):
    """C4 in small: Cornell box + 3 blobs = 9 MeshObjects, the masked object-level walk of the default frame kernel."""
    sc = scenes.config4(w, h, slices=24, stacks=19, sky=scenes.make_sky(64, 32))
    sc.num_bounces = 4
    return sc


SCENES = {"mixed": lambda w, h: scenes.mixed_test_scene(w, h), "multi_mesh": multi_mesh_scene}


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    """A context of this module's own: no buffers of another module's scene stay bound, and its options start at their defaults."""
    with Context(gpu_ctx.device) as c:
        yield c


def master(ctx, sc, rays=1, bounces=4, seed=0.5, offset=(POX, POY)):
    sc = copy.copy(sc)
    sc.num_rays, sc.num_bounces, sc.seed, sc.pixel_offset = rays, bounces, seed, offset
    m = RayTraceMaster(ctx, sc)
    m.numRays, m.numBounces = rays, bounces
    return m


def all_pixels(w, h):
    X, Y = np.meshgrid(np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32))
    return np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def emission_table(sc):
    """(n_spheres + n_meshes + 1, 3) float32 in the library's material order; the ground plane emits nothing."""
    return np.concatenate([sc.spheres["lighting"]["emission"].reshape(-1, 3), sc.mesh_objects["lighting"]["emission"].reshape(-1, 3),
                           np.zeros((1, 3))]).astype(F)


# ---- 1. pixels mode equals the frame ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mixed", "multi_mesh"])
def test_pixels_mode_equals_the_frame(ctx, scene):
    w, h = 40, 24                                                    # not a multiple of 8
    sc = SCENES[scene](w, h)
    rng = np.random.default_rng(11)
    xy = all_pixels(w, h)[rng.permutation(w * h)]
    xy = np.concatenate([xy, xy[rng.choice(w * h, 40)]])             # shuffled, with duplicates
    lit = 0
    for rays in (1, 3):
        for bounces in (1, 4, 8):
            for seed in (0.4375, 0.8125):
                m = master(ctx, sc, rays, bounces, seed)
                m.OnRenderImage()                                    # the default kernel (kernel_mode 3)
                img = m._target.GetPixels()
                got = ctx.radiance_query_pixels(xy, rays, bounces)   # the uniforms of that frame are still bound
                m.OnDisable()
                what = (scene, rays, bounces, seed)
                assert np.array_equal(bits(got), bits(img[xy[:, 1], xy[:, 0]])), what
                first = {tuple(p): k for k, p in enumerate(xy[:w * h].tolist())}
                dup = np.array([first[tuple(p)] for p in xy[w * h:].tolist()])
                assert np.array_equal(bits(got[w * h:]), bits(got[dup])), what
                assert (got[:, 3] == 1).all()
                lit += int((img[..., :3] > 0).any(axis=2).sum())
    assert lit > 12 * w * h // 4                                     # the frames are not black


# ---- 2. pixels mode equals the oracle, independently of the frame kernels -----------------------------------------------------------
@pytest.mark.parametrize("scene, rays, bounces", [("mixed", 1, 4), ("mixed", 3, 8), ("multi_mesh", 2, 4)])
def test_pixels_mode_equals_the_oracle(ctx, scene, rays, bounces):
    w, h = 40, 24
    sc = SCENES[scene](w, h)
    m = master(ctx, sc, rays, bounces, 0.4375)
    x0, y0 = 19, 11                                                  # a 16 x 8 crop that straddles tiles
    xy = all_pixels(16, 8) + np.array([x0, y0], np.int32)
    got = m.ResamplePixels(xy)                                       # frame 0's uniforms: the scene's own offset and seed; nothing is rendered
    orc = pyoracle.Oracle(m.scene)
    orc.set_frame((POX, POY), 0.4375)
    ref = orc.render(rect=(x0, y0, x0 + 16, y0 + 8), mode=0)         # the literal walk: no triangle BVH of the product's involved
    m.OnDisable()
    assert np.array_equal(bits(got), bits(ref.reshape(-1, 4))), (scene, rays, bounces)
    assert (ref[..., :3] > 0).any()


# ---- 3. rays mode equals the frame -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mixed", "multi_mesh"])
def test_rays_mode_equals_the_frame(ctx, scene):
    w, h = 40, 24
    sc = SCENES[scene](w, h)
    for bounces, seed in ((4, 0.4375), (8, 0.8125)):
        m = master(ctx, sc, 1, bounces, seed)
        m.OnRenderImage()
        img = m._target.GetPixels()
        O, D = camera_rays(m.scene, w, h, frame=(POX, POY, seed))    # each pixel's first (and only) ray, built on the host
        xy = all_pixels(w, h)
        seed_after = (F(F(seed) + F(0.5)) + F(0.5)).astype(F)        # the two jitter draws advanced the running seed
        got = ctx.radiance_query(O.reshape(-1, 3), D.reshape(-1, 3), xy.astype(F), float(seed_after), 1, bounces)
        m.OnDisable()
        assert np.array_equal(bits(got[:, :3]), bits(img.reshape(-1, 4)[:, :3])), (scene, bounces, seed)
        assert (got[:, 3] == 1).all()


# ---- 4. one bounce is the first hit's own light ---------------------------------------------------------------------------------
def test_one_bounce_is_the_first_hits_own_light(ctx):
    w, h = 40, 24
    sc = scenes.mixed_test_scene(w, h)
    m = bind(ctx, sc)
    aov = ctx.render_aov_arrays(w, h)                                # pixel centres
    O, D = camera_rays(sc, w, h)
    O, D = O.reshape(-1, 3), D.reshape(-1, 3)
    # and rays at the emissive quad (y = 3.5) from below and from above: one of the two sides faces them
    gx, gz = np.meshgrid(np.linspace(-1.3, 1.3, 4), np.linspace(-0.3, 2.3, 4))
    up = np.stack([gx.reshape(-1), np.full(16, 3.0), gz.reshape(-1)], axis=1)
    O = np.concatenate([O, up, up + np.array([0, 1.0, 0])]).astype(F)
    D = np.concatenate([D, np.tile([0, 1, 0], (16, 1)), np.tile([0, -1, 0], (16, 1))]).astype(F)
    q = ctx.ray_query(O, D)
    n = len(O)
    got = ctx.radiance_query(O, D, np.stack([np.arange(n) % 40, np.arange(n) // 40], axis=1).astype(F), 0.25, 1, 1)
    m.OnDisable()
    miss = q["kind"] == 0
    assert miss.sum() > 50 and (~miss).sum() > 50 and len(np.unique(q["kind"])) >= 3
    cam = np.arange(n) < w * h                                       # the camera rays: urt_render_aov traced the same ones
    assert np.array_equal(bits(got[miss & cam, :3]), bits(aov["albedo"].reshape(-1, 3)[miss[:w * h]]))      # the sky radiance Shade returns
    em = emission_table(sc)[material_index(sc, q["kind"], q["object"])]
    assert np.array_equal(bits(got[~miss, :3]), bits(em[~miss]))
    assert (em[~miss] > 0).any() and (got[:, 3] == 1).all()


# ---- 5. batch shape, device form, the two kernels -----------------------------------------------------------------------------------
@pytest.fixture
def shaped(ctx):
    w, h = 40, 24
    sc = scenes.mixed_test_scene(w, h)
    m = master(ctx, sc, 2, 4, 0.4375)
    m.ResamplePixels(np.zeros((1, 2), np.int32))                     # binds the scene, the uniforms and a Result texture
    rng = np.random.default_rng(5)
    xy = all_pixels(w, h)[rng.permutation(w * h)][:257]
    O, D = camera_rays(m.scene, w, h)
    O, D = O.reshape(-1, 3)[:257].copy(), D.reshape(-1, 3)[:257].copy()
    P = rng.random((257, 2)).astype(F) * 100
    S = rng.random(257).astype(F)
    yield m, xy, O, D, P, S
    m.OnDisable()


def rebind(ctx, m):
    m.SetShaderParameters()
    m.RayTraceShader.SetTexture(0, "Result", m._target)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 257])
def test_batch_shapes_and_the_device_form(ctx, shaped, n):
    import torch
    m, xy, O, D, P, S = shaped
    rebind(ctx, m)
    dev = torch.device("cuda", ctx.device)
    host_r = ctx.radiance_query(O[:n], D[:n], P[:n], S[:n], 2, 4)
    host_p = ctx.radiance_query_pixels(xy[:n], 2, 4)
    assert host_r.shape == (n, 4) and host_p.shape == (n, 4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dev_r = ctx.radiance_query(t(O[:n]), t(D[:n]), t(P[:n]), t(S[:n]), 2, 4).cpu().numpy()
    dev_p = ctx.radiance_query_pixels(t(xy[:n]), 2, 4).cpu().numpy()
    assert np.array_equal(bits(dev_r), bits(host_r)) and np.array_equal(bits(dev_p), bits(host_p))
    if n > 1:
        assert (host_r[:, :3] > 0).any() and (host_p[:, :3] > 0).any() and (host_r[:, 3] == 1).all()
        whole = ctx.radiance_query_pixels(xy, 2, 4)                  # a query's answer does not depend on its place in the batch
        assert np.array_equal(bits(whole[:n]), bits(host_p))
    zero = np.tile(np.array([0, 0, 0, 1], F), (n, 1))
    assert np.array_equal(ctx.radiance_query(O[:n], D[:n], P[:n], S[:n], 3, 0), zero)
    assert np.array_equal(ctx.radiance_query_pixels(xy[:n], 3, 0), zero)


def test_device_form_skips_pixels_outside_the_result(ctx, shaped):
    import torch
    m, xy, O, D, P, S = shaped
    rebind(ctx, m)
    dev = torch.device("cuda", ctx.device)
    ref = ctx.radiance_query_pixels(xy[:130], 2, 4)
    bad = {3: (-1, 5), 64: (40, 0), 65: (0, 24), 129: (7, -2147483648)}
    q = xy[:130].copy()
    for k, p in bad.items():
        q[k] = p
    for persist in (0, 1):
        ctx.set_option("radiance_persist", persist)
        try:
            got = ctx.radiance_query_pixels(torch.from_numpy(q).to(dev), 2, 4).cpu().numpy()
        finally:
            ctx.set_option("radiance_persist", -1)
        keep = np.array([k not in bad for k in range(130)])
        assert np.array_equal(bits(got[keep]), bits(ref[keep])), persist
        assert not got[~keep].view(np.uint32).any(), persist          # four zeros, not (0, 0, 0, 1)
    with pytest.raises(Exception) as e:                              # the host form refuses the batch
        ctx.radiance_query_pixels(q, 2, 4)
    assert getattr(e.value, "code", None) == 1


@pytest.mark.parametrize("scene", ["mixed", "multi_mesh"])
def test_the_two_kernels_agree(ctx, scene):
    """k_radiance (one query per thread) and k_radiance_persist (resident grid, work counter) run the same per-query steps."""
    w, h = 40, 24
    sc = SCENES[scene](w, h)
    m = master(ctx, sc, 3, 8, 0.8125)
    xy = all_pixels(w, h)[np.random.default_rng(7).permutation(w * h)]
    O, D = camera_rays(m.scene, w, h)
    out = {}
    try:
        for persist in (0, 1):
            ctx.set_option("radiance_persist", persist)
            pix = m.ResamplePixels(xy)
            ray = m.SampleRadiance(O.reshape(-1, 3), D.reshape(-1, 3), 5)
            one = m.ResamplePixels(xy[:1])
            out[persist] = (pix, ray, one)
    finally:
        ctx.set_option("radiance_persist", -1)
        m.OnDisable()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(bits(a), bits(b))
    assert (out[0][0][:, :3] > 0).any() and (out[0][1][:, :3] > 0).any()


# ---- 6. housekeeping ---------------------------------------------------------------------------------------------------------------
def test_queries_do_not_change_frames_or_counters(ctx):
    sc = scenes.config3(96, 54, slices=60, stacks=47, sky=scenes.make_sky(64, 32))
    xy = all_pixels(96, 54)[::7]
    O, D = camera_rays(sc, 96, 54)
    O, D = O.reshape(-1, 3)[::11].copy(), D.reshape(-1, 3)[::11].copy()
    P = all_pixels(96, 54)[::11].astype(F)

    def run(with_queries):
        ctx.set_option("kernel_mode", 3)
        ctx.set_option("count_stats", 1)
        ctx.reset_counters()
        m = RayTraceMaster(ctx, sc)
        answers = []
        for _ in range(8):
            m.OnRenderImage()
            if with_queries:
                answers.append(ctx.radiance_query(O, D, P, 0.25, 2, 4))
                answers.append(ctx.radiance_query_pixels(xy, 1, 4))
        img, conv = m._target.GetPixels(), m._converged.GetPixels()
        ctr = ctx.counters()
        m.OnDisable()
        ctx.set_option("count_stats", 0)
        return img, conv, ctr, answers

    img0, conv0, c0, _ = run(False)
    img1, conv1, c1, answers = run(True)
    assert img0.tobytes() == img1.tobytes() and conv0.tobytes() == conv1.tobytes()
    c0.pop("trace_ms"); c1.pop("trace_ms")
    assert c0 == c1, (c0, c1)
    assert c0["launches"] < 8                                        # the frames stayed batched
    assert all(a.tobytes() == answers[0].tobytes() for a in answers[0::2])       # rays mode does not read the frame's uniforms
    assert len({a.tobytes() for a in answers[1::2]}) == 8            # pixels mode does: every frame has its own seed and offset
    assert (answers[0][:, :3] > 0).any()


def test_queries_see_scene_updates(ctx):
    w, h = 40, 24
    sc = scenes.mixed_test_scene(w, h)
    m = master(ctx, sc, 1, 4, 0.4375)
    xy = all_pixels(w, h)
    try:
        before = m.ResamplePixels(xy)
        mo = m.scene.mesh_objects.copy()
        k = int(np.argmax(mo["indices_count"]))
        mo[k]["localToWorldMatrix"] = scenes.trs(translate=(0.7, 1.4, -0.3), scale=(1.2, 0.9, 1.1), yaw_deg=23)
        refits0 = ctx.refit_stats()
        m._meshObjectBuffer.SetData(mo)
        m._meshObjectBVHBuffer.SetData(scenes.build_object_bvh(*scenes.mesh_bounds(mo, sc.vertices, sc.indices)))
        after = m.ResamplePixels(xy)                                 # prepares the moved scene (in place) first
        assert ctx.refit_stats()[1] == refits0[1] + 1
        m.OnRenderImage()
        img = m._target.GetPixels()
        assert np.array_equal(bits(after), bits(img.reshape(-1, 4)))
        assert not np.array_equal(bits(after), bits(before))
    finally:
        m.OnDisable()


def test_large_lds_launch(ctx, shaped):
    m, xy, O, D, P, S = shaped
    rebind(ctx, m)
    ref_p, ref_r = ctx.radiance_query_pixels(xy, 2, 4), ctx.radiance_query(O, D, P, S, 2, 4)
    try:
        for persist in (0, 1):
            ctx.set_option("radiance_persist", persist)
            ctx.set_option("stack_pad", 96)                          # > 64 KiB of stacks per workgroup
            assert np.array_equal(bits(ctx.radiance_query_pixels(xy, 2, 4)), bits(ref_p)), persist
            assert np.array_equal(bits(ctx.radiance_query(O, D, P, S, 2, 4)), bits(ref_r)), persist
    finally:
        ctx.set_option("stack_pad", 0)
        ctx.set_option("radiance_persist", -1)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_large_lds_launch_of_ray_queries(ctx, shaped):
    """stack_pad reaches k_query's launch too: 257 rays = one full workgroup and a ragged one, closest hit and any hit."""
    m = shaped[0]
    rebind(ctx, m)
    O, D = camera_rays(m.scene, 40, 24)
    pick = np.random.default_rng(7).permutation(40 * 24)[:257]       # rays all over the image (the fixture's own 257 all end on the ground)
    O, D = O.reshape(-1, 3)[pick].copy(), D.reshape(-1, 3)[pick].copy()
    ref_c, ref_a = ctx.ray_query(O, D), ctx.ray_query(O, D, any_hit=True)
    assert len(np.unique(ref_c["kind"])) == 4 and 0 < ref_a.sum() < len(ref_a)      # misses, the ground, spheres and triangles
    try:
        ctx.set_option("stack_pad", 96)                              # > 64 KiB of stacks per workgroup
        assert same_bytes(ctx.ray_query(O, D), ref_c)
        assert same_bytes(ctx.ray_query(O, D, any_hit=True), ref_a)
    finally:
        ctx.set_option("stack_pad", 0)


def test_large_lds_launch_of_feature_buffers(ctx, shaped):
    """stack_pad reaches k_aov's launch too: 24 x 17 has ragged tiles on both edges; both camera-ray forms."""
    rebind(ctx, shaped[0])
    ref = [ctx.render_aov_arrays(24, 17, frame_ray=fr) for fr in (False, True)]
    assert len(np.unique(ref[0]["kind"])) == 4 and not same_bytes(ref[0]["position"], ref[1]["position"])
    try:
        ctx.set_option("stack_pad", 96)
        for fr in (False, True):
            got = ctx.render_aov_arrays(24, 17, frame_ray=fr)
            assert got.keys() == ref[fr].keys()
            for k in got:
                assert same_bytes(got[k], ref[fr][k]), (fr, k)
    finally:
        ctx.set_option("stack_pad", 0)


def test_argument_errors_write_nothing(gpu_ctx):
    import torch
    w, h = 40, 24
    sc = scenes.mixed_test_scene(w, h)
    with Context(gpu_ctx.device) as ctx:                             # a fresh context: nothing bound yet
        lib, hd = ctx.lib, ctx._h
        dev = torch.device("cuda", ctx.device)
        n = 4
        rays = np.zeros((n, 12), F); rays[:, 5] = 1
        pix = np.array([[0, 0], [1, 1], [2, 2], [3, 3]], np.int32)
        out = np.full((n, 4), 7.0, F)
        d_rays, d_pix = torch.from_numpy(rays).to(dev), torch.from_numpy(pix).to(dev)
        d_out = torch.full((n + 1, 4), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)         # noqa: E731
        host, devf = lib.urt_radiance_query, lib.urt_radiance_query_device

        def untouched():
            ctx.synchronize()
            torch.cuda.synchronize(dev)
            return (out == 7.0).all() and bool((d_out == 7.0).all())

        # pixels mode before anything is bound: no Result, no camera
        assert host(hd, p(pix), n, 1, 1, p(out), 1) == 5 and devf(hd, dp(d_pix), n, 1, 1, dp(d_out), 1) == 5      # URT_ERR_UNBOUND
        tex = RenderTexture(ctx, w, h)
        sh = ComputeShader(ctx)
        sh.SetTexture(0, "Result", tex)
        assert host(hd, p(pix), n, 1, 1, p(out), 1) == 5 and devf(hd, dp(d_pix), n, 1, 1, dp(d_out), 1) == 5      # a Result, still no camera
        sh.SetMatrix("_CameraToWorld", sc.camera_to_world)
        assert host(hd, p(pix), n, 1, 1, p(out), 1) == 5
        sh.SetMatrix("_CameraInverseProjection", sc.camera_inverse_projection)
        sh.SetTexture(0, "Result", None)
        assert host(hd, p(pix), n, 1, 1, p(out), 1) == 5                                                            # cameras, no Result
        sh.SetTexture(0, "Result", tex)
        assert untouched()
        m = bind(ctx, sc)
        m.RayTraceShader.SetTexture(0, "Result", tex)
        for flags, h_in, d_in in ((0, rays, d_rays), (1, pix, d_pix)):
            for fn, a, o in ((host, p(h_in), p(out)), (devf, dp(d_in), dp(d_out))):
                assert fn(hd, None, 0, 1, 1, None, flags) == 0                                   # n == 0: nothing to do
                assert fn(hd, a, -1, 1, 1, o, flags) == 1
                assert fn(hd, None, n, 1, 1, o, flags) == 1 and fn(hd, a, n, 1, 1, None, flags) == 1
                assert fn(hd, a, n, 1, 1, o, 2) == 1 and fn(hd, a, n, 1, 1, o, -1) == 1
                assert fn(hd, a, n, 0, 1, o, flags) == 1 and fn(hd, a, n, 4097, 1, o, flags) == 1
                assert fn(hd, a, n, 1, -1, o, flags) == 1 and fn(hd, a, n, 1, 65, o, flags) == 1
                assert fn(None, a, n, 1, 1, o, flags) == 1
        # alignment of the device form: rays and output 16 bytes, pixels 8
        assert devf(hd, dp(d_rays, 4), n - 1, 1, 1, dp(d_out), 0) == 1 and devf(hd, dp(d_rays), n, 1, 1, dp(d_out, 8), 0) == 1
        assert devf(hd, dp(d_pix, 4), n - 1, 1, 1, dp(d_out), 1) == 1 and devf(hd, dp(d_pix), n, 1, 1, dp(d_out, 4), 1) == 1
        # the host form looks at its pixels
        for bad in ((-1, 0), (w, 0), (0, h), (0, -1)):
            q = pix.copy(); q[2] = bad
            assert host(hd, p(q), n, 1, 1, p(out), 1) == 1, bad
        assert untouched()
        # and valid calls do write, at the limits of the ranges too
        assert host(hd, p(pix), n, 4096, 0, p(out), 1) == 0 and np.array_equal(out, np.tile(np.array([0, 0, 0, 1], F), (n, 1)))
        assert host(hd, p(rays), n, 1, 64, p(out), 0) == 0 and (out[:, 3] == 1).all()
        assert devf(hd, dp(d_pix, 8), n - 1, 1, 1, dp(d_out, 16), 1) == 0                           # 8-byte aligned pixels are enough
        ctx.synchronize()
        got = d_out.cpu().numpy()
        assert (got[0] == 7.0).all() and (got[1:4, 3] == 1).all() and (got[4] == 7.0).all()       # n - 1 texels from the second on
        m.OnDisable()
        tex.Release()


# ---- 7. master level: fresh samples for the pixels a reprojection left without history ----------------------------------------------
def test_resample_pixels_of_a_disocclusion_mask(gpu_ctx):
    w, h = 96, 64
    sc = scenes.mixed_test_scene(w, h)
    with Context(gpu_ctx.device) as ctx:
        m = RayTraceMaster(ctx, sc)
        m.numRays = 2
        m.EnableTemporalAccumulation()
        for _ in range(4):
            m.OnRenderImage()
        m.MoveCamera(*scenes.camera_matrices(w, h, position=(0.6, 1.0, -10.0), yaw_deg=3.0))
        count = m._tcount.GetPixels()[..., 0]
        ys, xs = np.nonzero(count == 0)
        assert 0 < len(xs) < w * h // 2                              # some pixels lost their history, most kept it
        xy = np.stack([xs, ys], axis=1).astype(np.int32)
        fresh = m.ResamplePixels(xy)
        m.OnRenderImage()                                            # the next frame: the same uniforms
        img = m._target.GetPixels()
        m.OnDisable()
        assert np.array_equal(bits(fresh), bits(img[ys, xs]))
        assert (fresh[:, :3] > 0).any() and (fresh[:, 3] == 1).all()


def test_sample_radiance_streams(ctx):
    """SampleRadiance: numBounces and the current _Seed of the master; the pixel of query i is (i mod 4096, i div 4096)."""
    sc = scenes.mixed_test_scene(40, 24)
    m = master(ctx, sc, 1, 4, 0.4375)
    n = 4100                                                         # crosses the 4096 wrap
    rng = np.random.default_rng(3)
    O = (rng.random((n, 3)) * np.array([6, 3, 6]) - np.array([3, -0.2, 3])).astype(F)
    D = rng.normal(size=(n, 3)).astype(F)
    got = m.SampleRadiance(O, D, 4)
    i = np.arange(n)
    P = np.stack([i % 4096, i // 4096], axis=1).astype(F)
    ref = ctx.radiance_query(O, D, P, 0.4375, 4, 4)
    same_ray = m.SampleRadiance(np.tile(O[:1], (64, 1)), np.tile(D[:1], (64, 1)), 4)
    m.OnDisable()
    assert np.array_equal(bits(got), bits(ref)) and (got[:, :3] > 0).any()
    assert P[4096].tolist() == [0, 1] and same_bits(got[:, 3], np.ones(n, F)).all()
    assert len({r.tobytes() for r in same_ray}) > 1                  # one ray, 64 random streams
