"""GPU: the image-space kernels (urt_reproject, urt_reproject_objects, urt_reproject_deformed, urt_upsample, urt_denoise, urt_bloom) and
urt_render_aov against the first-principles geometry of tests/registration_model.py: this pixel's history must come from THERE.  The
same checks tests/test_registration_model.py runs on the numpy restatements (with the negative controls that show each check can fail),
here on what the kernels wrote.  Feature buffers come from urt_render_aov on scenes.mixed_test_scene; the moved objects go through
MoveObjects (a refit), the deformed blob through DeformMeshes with a urt_buffer_copy snapshot of its vertices."""
import numpy as np
import pytest

import registration_model as R
from unityraytracer_amd import Context, RayTraceMaster, host_scene, scenes
from unityraytracer_amd.unity_api import ComputeBuffer, RenderTexture
from upsample_ref import low_grid_position

pytestmark = pytest.mark.gpu

F = np.float32
# px.  About eight float32 roundings scaled by W / 2 stay below 1e-4 px at these sizes; this is ten times that and 500 times below a
# half-pixel error.  Measured on one MI355X (pytest -s prints every figure; DESIGN.md "Temporal reprojection"): check 1 8.0e-6 .. 2.6e-5
# px, check 2 <= 1.1e-5 px, check 3 <= 2.4e-5: the figures of the restatements on the same guides.
TOL = 1e-3
TOL_MOVED = 1e-3                                                             # check 4: measured <= 1.7e-5 px (motion), <= 2.5e-5 (gather); the restatements too, under 2.5e-4: not raised
TOL_IDENTITY = 1e-4                                                          # world units; derivation in tests/test_registration_model.py; measured <= 8.1e-6
MIN_SHARE = 0.8                                                              # check 3: surface pixels checked (measured 0.859 at 67x45, 0.885 at 96x64, as the restatement alone)
MIN_SHARE_MOVED = 0.5                                                        # check 4: of each moved object's pixels (measured: mesh 0.67 / 0.72, sphere 0.90 / 0.93, blob 0.77 / 0.86)
TOL_UPSAMPLE = 1e-5                                                          # check 5a measured <= 2.4e-7
MIN_SHARE_UPSAMPLE = 0.75                                                    # check 5b (measured 0.815 and 0.868)
TOL_CENTROID, TOL_SUM = 1e-4, 1e-5                                           # check 7 (measured <= 8.1e-8 px, <= 4.9e-8 relative)
SIZE_IDS = dict(ids=lambda s: "%dx%d" % s)


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    with Context(gpu_ctx.device) as c:
        yield c


def read_guides(m):
    t = m.RenderFeatureBuffers()
    return t[0].GetPixels(), t[1].GetPixels(), t[3].GetPixels()


_rendered = {}


def guides(ctx, W, H, cam, aspect=None):
    """(hit, normal, id) of urt_render_aov(URT_AOV_PIXEL_CENTER) on the mixed scene under the pose `cam`, rendered once per module."""
    key = (id(ctx), W, H, tuple(sorted((k, tuple(np.ravel(v))) for k, v in cam.items())), aspect)
    if key not in _rendered:
        m = RayTraceMaster(ctx, R.posed(scenes, scenes.mixed_test_scene(W, H), dict(cam, aspect=aspect)))
        _rendered[key] = read_guides(m)
        m.OnDisable()
        for a in _rendered[key]:
            a.setflags(write=False)
    return _rendered[key]


def reproject(ctx, W, H, prev, cur, then, now, **kw):
    color, count = R.ramp_history(W, H)
    M = scenes.world_to_clip(*R.camera_of(scenes, W, H, then))
    return ctx.reproject_arrays(color, count, *prev, *cur, M, *R.camera_of(scenes, W, H, now), max_history=0.0, **kw)


# ---- 1. the model against traced geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["A", "B", "plane"])
@pytest.mark.parametrize("size", R.SIZES, **SIZE_IDS)
def test_hit_points_project_to_their_own_pixel(ctx, size, cam):
    pose = {"A": R.POSE_A, "B": R.POSE_B, "plane": R.PLANE_POSE}[cam]
    hit, normal, ids = guides(ctx, *size, pose)
    d = R.own_pixel_deviation(hit, normal, pose)
    r, n = R.identity_residual(hit, normal, ids, R.SceneData(scenes.mixed_test_scene(*size)))
    print(f"check 1 {size} {cam}: {d:.2e} px; identity {r:.2e} world units over {n} triangle pixels")
    assert d <= TOL and r <= TOL_IDENTITY
    if cam == "plane":
        assert (normal[..., 3] == 1).all()                                   # the view check 5a needs
    else:
        assert n > 20 and (normal[..., 3] == 0).any() and (normal[..., 3] == 2).any()


# ---- 2, 3. motion vectors and the gather, static scene ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(R.STATIC_PAIRS))
@pytest.mark.parametrize("size", R.SIZES, **SIZE_IDS)
def test_static_scene_motion_and_gather(ctx, size, pair):
    then, now = R.STATIC_PAIRS[pair]
    prev, cur = guides(ctx, *size, then), guides(ctx, *size, now)
    out = reproject(ctx, *size, prev, cur, then, now)
    q, depth, classed = R.model_positions(cur[0], cur[1], then, now)
    surface = R.classes(*cur[:2])[0]
    dev, n, n_out, bad = R.motion_deviation(out, q, depth, classed)
    gdev, share = R.gather_deviation(out, q, depth, classed, of=surface)
    gall, _ = R.gather_deviation(out, q, depth, classed)
    print(f"checks 2, 3 {size} {pair}: motion {dev:.2e} px over {n}; {n_out} outside, {bad} of them not zero; gather {max(gdev, gall):.2e}, "
          f"share of surface pixels {share:.3f}")
    assert dev <= TOL and n > 0.3 * classed.sum()
    assert bad == 0 and (n_out > 0.2 * surface.sum() if pair == "behind" else n_out > 0)
    assert gall <= TOL
    if pair == "move":                                                       # behind: the surface pixels are the ones without history
        assert gdev <= TOL and share >= MIN_SHARE


# ---- 4. moved objects and a deformed mesh --------------------------------------------------------------------------------------------------------------
def check_objects(out, cur, q, q_still, depth, classed, masks, what):
    for name, mask in masks.items():
        dev, n, _, bad = R.motion_deviation(out, q, depth, classed, only=mask)
        gdev, share = R.gather_deviation(out, q, depth, classed, of=mask)
        print(f"check 4 {what} {name}: {int(mask.sum())} pixels, motion {dev:.2e} px over {n}, gather {gdev:.2e}, share checked {share:.3f}")
        assert mask.sum() >= 60 and n >= 0.9 * mask.sum()
        assert dev <= TOL_MOVED and bad == 0
        assert gdev <= TOL_MOVED and share >= MIN_SHARE_MOVED
        assert np.abs(q - q_still)[mask].max() >= 1.0                        # the object does move by a pixel or more on its own
    dev, n, _, bad = R.motion_deviation(out, q, depth, classed)               # and everything else in the image stays right
    gdev, share = R.gather_deviation(out, q, depth, classed, of=R.classes(*cur[:2])[0])
    print(f"   whole image: motion {dev:.2e} px over {n}, gather {gdev:.2e}, share of surface pixels {share:.3f}")
    assert dev <= TOL_MOVED and bad == 0 and gdev <= TOL_MOVED and share > 0.5


@pytest.mark.parametrize("size", R.SIZES, **SIZE_IDS)
def test_moved_objects_come_from_where_identity_puts_them(ctx, size):
    rest = scenes.mixed_test_scene(*size)
    moved = R.moved_scene(scenes, rest)
    m = RayTraceMaster(ctx, R.posed(scenes, rest, R.MOVED_A))
    prev = read_guides(m)
    m.MoveObjects({R.MOVED_MESH: moved.mesh_objects[R.MOVED_MESH]["localToWorldMatrix"]},
                  {R.MOVED_SPHERE: (moved.spheres[R.MOVED_SPHERE]["position"], moved.spheres[R.MOVED_SPHERE]["radius"])},
                  *R.camera_of(scenes, *size, R.MOVED_B))                    # temporal accumulation off: the edits (a refit) and a reset
    cur = read_guides(m)
    m.OnDisable()
    r, n = R.identity_residual(*cur, R.SceneData(moved))
    print(f"check 4 {size} moved: identity {r:.2e} world units over {n} triangle pixels")
    assert r <= TOL_IDENTITY
    out = reproject(ctx, *size, prev, cur, R.MOVED_A, R.MOVED_B, mesh_motion=host_scene.mesh_motion(rest.mesh_objects, moved.mesh_objects),
                    sphere_motion=host_scene.sphere_motion(rest.spheres, moved.spheres))
    was = R.where_it_was(*cur, R.SceneData(moved), R.SceneData(rest))
    q, depth, classed = R.model_positions(cur[0], cur[1], R.MOVED_A, R.MOVED_B, was)
    k, o = cur[1][..., 3], R.bits(cur[2][..., 0])
    check_objects(out, cur, q, R.model_positions(cur[0], cur[1], R.MOVED_A, R.MOVED_B)[0], depth, classed,
                  {"mesh": (k == 3) & (o == R.MOVED_MESH), "sphere": (k == 2) & (o == R.MOVED_SPHERE)}, f"{size} moved")


@pytest.mark.parametrize("size", R.SIZES, **SIZE_IDS)
def test_a_deformed_mesh_comes_from_where_identity_puts_it(ctx, size):
    rest = scenes.mixed_test_scene(*size)
    deformed = R.deformed_scene(scenes, rest)
    m = RayTraceMaster(ctx, R.posed(scenes, rest, R.DEFORM_A))
    prev = read_guides(m)
    snapshot = ComputeBuffer(ctx, m._vertexBuffer.count, 12)
    snapshot.CopyFrom(m._vertexBuffer)                                       # urt_buffer_copy, before the edit
    m.DeformMeshes({R.DEFORMED_MESH: R.deformed_positions(rest)})             # temporal accumulation off: the edit (a refit) and a reset
    m.MoveCamera(*R.camera_of(scenes, *size, R.DEFORM_B))
    cur = read_guides(m)
    prev_vertices = snapshot.GetData().view(F).reshape(-1, 3)
    snapshot.Release()
    m.OnDisable()
    assert prev_vertices.tobytes() == np.ascontiguousarray(rest.vertices, F).tobytes()
    r, n = R.identity_residual(*cur, R.SceneData(deformed))
    print(f"check 4 {size} deformed: identity {r:.2e} world units over {n} triangle pixels")
    assert r <= TOL_IDENTITY
    flags = np.zeros(len(rest.mesh_objects), np.int32)
    flags[R.DEFORMED_MESH] = 1
    out = reproject(ctx, *size, prev, cur, R.DEFORM_A, R.DEFORM_B, deform=(prev_vertices, rest.indices, rest.mesh_objects, flags))
    was = R.where_it_was(*cur, R.SceneData(deformed), R.SceneData(rest))
    q, depth, classed = R.model_positions(cur[0], cur[1], R.DEFORM_A, R.DEFORM_B, was)
    k, o = cur[1][..., 3], R.bits(cur[2][..., 0])
    check_objects(out, cur, q, R.model_positions(cur[0], cur[1], R.DEFORM_A, R.DEFORM_B)[0], depth, classed,
                  {"blob": (k == 3) & (o == R.DEFORMED_MESH)}, f"{size} deformed")


# ---- 5. upsampling ------------------------------------------------------------------------------------------------------------------------------------
def upsample(ctx, low_color, low, full):
    h, w = low_color.shape[:2]
    H, W = full[0].shape[:2]
    tex = [RenderTexture(ctx, w, h) for _ in range(4)] + [RenderTexture(ctx, W, H) for _ in range(4)]
    try:
        for t, a in zip(tex, (low_color, *low, *full)):
            t.SetPixels(a)
        ctx.upsample(*tex[:4], *tex[4:7], tex[7], wide_fallback=False)       # flags = 0
        return tex[7].GetPixels()
    finally:
        for t in tex:
            t.Release()


@pytest.mark.parametrize("pair", R.UPSAMPLE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_upsampling_a_plane_reproduces_the_screen_ramp(ctx, pair):
    w, h, W, H = pair
    low, full = guides(ctx, w, h, R.PLANE_POSE), guides(ctx, W, H, R.PLANE_POSE)
    assert (low[1][..., 3] == 1).all() and (full[1][..., 3] == 1).all()      # every pixel of both grids sees the ground plane
    color = upsample(ctx, R.screen_ramp(w, h), low, full)
    inside = R.four_taps_inside(w, h, W, H)
    d = R.upsample_deviation(color, W, H)
    print(f"check 5a {pair}: {d[inside].max():.2e} over {int(inside.sum())} of {W * H} pixels")
    assert inside.mean() > 0.8 and d[inside].max() <= TOL_UPSAMPLE


@pytest.mark.parametrize("pair", R.MIXED_PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_upsampling_a_mixed_view(ctx, pair):
    """Both grids look through the full grid's camera (the low one keeps its width : height), as a host that upsamples renders them."""
    w, h, W, H = pair
    low_cam = dict(R.POSE_A, aspect=W / H)
    low, full = guides(ctx, w, h, R.POSE_A, aspect=W / H), guides(ctx, W, H, R.POSE_A)
    d1 = R.own_pixel_deviation(low[0], low[1], low_cam)
    color = upsample(ctx, R.screen_ramp(w, h), low, full)
    share = float((R.upsample_deviation(color, W, H) <= TOL_UPSAMPLE).mean())
    rel = R.grid_relation_deviation(full[0], full[1], w, h, low_cam, low_grid_position(W, w), low_grid_position(H, h))
    print(f"check 5b {pair}: share within {TOL_UPSAMPLE:g}: {share:.3f}; low grid check 1 {d1:.2e} px; 5c grid relation {rel:.2e} low px")
    assert share >= MIN_SHARE_UPSAMPLE
    assert d1 <= TOL and rel <= TOL


# ---- 6. denoiser ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_denoiser_leaves_a_ramp_on_uniform_guides_alone(ctx, iterations):
    W, H = 67, 45
    hit, normal = R.uniform_guides(W, H)
    src = R.denoise_ramp(W, H)
    out = ctx.denoise_arrays(src, hit, normal, iterations=iterations, sigma_color=0.0)
    inner = R.interior(W, H, 2 * (2 ** iterations - 1))
    err = np.abs(out[..., :3].astype(np.float64) - src[..., :3].astype(np.float64))
    bound = 1e-4 * (1.0 + np.abs(src[..., :3].astype(np.float64)))           # the header's own bound
    print(f"check 6 iterations {iterations}: interior {err[inner].max():.2e} over {int(inner.sum())} pixels, borders up to {err[~inner].max():.2f}")
    assert inner.sum() >= 100 and (err[inner] <= bound[inner]).all()
    assert err[~inner].max() > 0.1                                            # the borders do show what a lopsided footprint does


# ---- 7. bloom ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(97, 61, 48, 30, 3), (97, 61, 47, 31, 3), (131, 95, 65, 47, 4)], ids=lambda c: "%dx%d-at-%d-%d-levels-%d" % c)
def test_bloom_of_an_impulse_is_centred_on_it(ctx, case):
    W, H, x, y, levels = case
    src = R.impulse(W, H, x, y)
    a, b = RenderTexture(ctx, W, H), RenderTexture(ctx, W, H)
    try:
        a.SetPixels(src)
        ctx.bloom(a, b, threshold=0.0, soft_knee=0.0, intensity=1.0, levels=levels)
        dst = b.GetPixels()
    finally:
        a.Release()
        b.Release()
    cx, cy, s, edge = R.glow_moments(dst, src)
    print(f"check 7 {case}: centroid off by {np.abs(cx - x).max():.1e}, {np.abs(cy - y).max():.1e} px, sum off by "
          f"{np.abs(s / src[y, x, :3] - 1).max():.1e} relative")
    assert edge == 0.0                                                       # the support does not touch a border
    assert np.abs(cx - x).max() <= TOL_CENTROID and np.abs(cy - y).max() <= TOL_CENTROID
    assert (np.abs(s / src[y, x, :3].astype(np.float64) - 1.0) <= TOL_SUM).all()
