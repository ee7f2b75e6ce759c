"""CPU: the numpy restatements of the image-space stages (reproject_ref, reproject_objects_ref, reproject_deformed_ref, upsample_ref,
denoise_ref, bloom_ref) against the first-principles geometry of tests/registration_model.py, and the negative controls: every wrong
reading of where a texel sits, fed to a restatement as perturbed INPUTS, must fail its check by at least 100 times the tolerance.
tests/test_gpu_registration.py runs the same checks on the kernels' outputs.

Guides: the analytic scene of tests/reproject_ref.py and the mixed test scene traced by the oracle (aov_ref.render_aov_ref), the latter
also with one mesh and one sphere moved and with the blob deformed."""
import functools

import numpy as np
import pytest

import registration_model as R
from aov_ref import render_aov_ref
from bloom_ref import bloom_ref
from denoise_ref import denoise_ref, reach
from reproject_deform_ref import matrices_of, reproject_deformed_ref
from reproject_motion_ref import reproject_objects_ref
from reproject_ref import analytic_aovs, reproject_ref
from unityraytracer_amd import host_scene, scenes
from upsample_ref import low_grid_position, upsample_ref

F = np.float32
# px.  About eight float32 roundings scaled by W / 2 stay below 1e-4 px at these sizes; this is ten times that and 500 times below a
# half-pixel error.  Measured here (pytest -s prints every figure): check 1 2.4e-6 .. 2.6e-5 px at 67x45 and 96x64 (6.0e-5 at 200x120),
# check 2 <= 1.1e-5 px, check 3 <= 2.4e-5; the controls: 1.000 for a one-texel roll, 44 / 63 for flipped rows, 15 / 21 px for the wrong matrix.
TOL = 1e-3
# Moved and deformed pixels (check 4): the restatements measured against the model give <= 1.7e-5 px (motion) and <= 2.5e-5 (gather) for
# the moved mesh and sphere, <= 9.3e-6 / 1.9e-5 for the deformed blob: under 2.5e-4, so the tolerance stays at 1e-3.  The controls: an
# inverted table 1.5 .. 12 px, swapped barycentrics 4.8 / 7.6 px.
TOL_MOVED = 1e-3
CONTROL = 100.0                                                              # a control must miss by this many tolerances
# World units.  A hit point is origin + t * direction in float32: |P| <= 20 has an ulp of 2e-6 and t carries a few ulps of its own, so
# 1e-5 is reachable; float32 barycentrics add 1e-7 per unit of edge.  Measured <= 8.1e-6 (1.5e-5 at 200x120); a swapped u / v gives 2.6.
TOL_IDENTITY = 1e-4
MIN_SHARE_RESTATEMENT = 0.85                                                 # check 3: surface pixels checked; the kernels' test asks 0.8 (measured 0.859 .. 0.901)
MIN_SHARE_MOVED = 0.5                                                        # check 4: of each moved object's pixels (measured 0.67 .. 0.93)
TOL_UPSAMPLE = 1e-5                                                          # check 5a measured <= 2.4e-7
MIN_SHARE_UPSAMPLE = 0.75                                                    # check 5b (measured 0.815 .. 0.892; half a low pixel off: 0.000)
CAMS = {"A": R.POSE_A, "B": R.POSE_B, "behind": R.POSE_BEHIND, "movedA": R.MOVED_A, "movedB": R.MOVED_B, "deformA": R.DEFORM_A,
        "deformB": R.DEFORM_B, "plane": R.PLANE_POSE}
NEAR = {"moved": ("movedA", "movedB"), "deformed": ("deformA", "deformB")}


# ---- guides, rendered once and shared (nothing writes into them) -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed(W, H, state="rest"):
    sc = scenes.mixed_test_scene(W, H)
    return {"rest": lambda: sc, "moved": lambda: R.moved_scene(scenes, sc), "deformed": lambda: R.deformed_scene(scenes, sc)}[state]()


@functools.lru_cache(maxsize=None)
def guides(source, W, H, cam, state="rest", half_off=False, aspect=None):
    """(hit, normal, id) of the pixel-centre rays of CAMS[cam]; aspect: the width : height of the view when it is not W : H."""
    c2w, invp = R.camera_of(scenes, W, H, dict(CAMS[cam], aspect=aspect))
    if half_off:
        invp = R.half_pixel_off(invp, W, H)
    if source == "analytic":
        out = analytic_aovs(W, H, c2w, invp)
    else:
        sc = R.posed(scenes, mixed(W, H, state), dict(CAMS[cam], aspect=aspect))
        sc.camera_inverse_projection = invp
        hit, normal, _, ids = render_aov_ref(sc)
        out = (hit, normal, ids)
    for a in out:
        a.setflags(write=False)
    return out


def world_to_clip(W, H, cam):
    return scenes.world_to_clip(*R.camera_of(scenes, W, H, CAMS[cam]))


def reproject_inputs(source, W, H, then, now, state="rest"):
    """What one reprojection call takes: the ramp history, the guides of (rest scene, camera `then`) and of (`state`, camera `now`)."""
    color, count = R.ramp_history(W, H)
    prev, cur = guides(source, W, H, then), guides(source, W, H, now, state)
    return dict(images=(color, count, *prev, *cur), M=world_to_clip(W, H, then), cam=R.camera_of(scenes, W, H, CAMS[now]), cur=cur)


def static_model(c, then, now):
    return R.model_positions(c["cur"][0], c["cur"][1], CAMS[then], CAMS[now])


def run_static(c, images=None, M=None):
    return reproject_ref(*(c["images"] if images is None else images), c["M"] if M is None else M, *c["cam"], max_history=0.0)


# ---- 1. the model against traced geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["A", "B", "movedA", "deformB", "plane"])
@pytest.mark.parametrize("size", R.SIZES + [(200, 120)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("source", ["analytic", "mixed"])
def test_hit_points_project_to_their_own_pixel(source, size, cam):
    hit, normal, ids = guides(source, *size, cam)
    d = R.own_pixel_deviation(hit, normal, CAMS[cam])
    print(f"check 1 {source} {size} {cam}: {d:.2e} px")
    assert d <= TOL
    if source == "mixed":
        r, n = R.identity_residual(hit, normal, ids, R.SceneData(mixed(*size)))
        print(f"   identity: {r:.2e} world units over {n} triangle pixels")
        assert r <= TOL_IDENTITY and (n > 20 or cam == "plane")


def test_the_plane_pose_sees_only_the_ground():
    for w, h in sorted({p[:2] for p in R.UPSAMPLE_PAIRS} | {p[2:] for p in R.UPSAMPLE_PAIRS}):
        assert (guides("mixed", w, h, "plane")[1][..., 3] == 1).all(), (w, h)


# ---- 2, 3. motion vectors and the gather, static scene ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["move", "behind"])
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("source", ["analytic", "mixed"])
def test_static_scene_motion_and_gather(source, size, pair):
    then, now = ("A", "B") if pair == "move" else ("behind", "A")
    c = reproject_inputs(source, *size, then, now)
    q, depth, classed = static_model(c, then, now)
    out = run_static(c)
    surface = R.classes(*c["cur"][:2])[0]
    dev, n, n_out, bad = R.motion_deviation(out, q, depth, classed)
    gdev, share = R.gather_deviation(out, q, depth, classed, of=surface)
    gall, _ = R.gather_deviation(out, q, depth, classed)
    print(f"checks 2, 3 {source} {size} {pair}: motion {dev:.2e} px over {n}; {n_out} outside, {bad} of them not zero; gather {max(gdev, gall):.2e}, "
          f"share of surface pixels {share:.3f}")
    assert dev <= TOL and n > 0.3 * classed.sum()
    assert bad == 0 and (n_out > 0.2 * surface.sum() if pair == "behind" else n_out > 0)
    assert gall <= TOL
    if pair == "move":                                                       # behind: the surface pixels are the ones without history
        assert gdev <= TOL and share >= MIN_SHARE_RESTATEMENT


CONTROLS = {"rolled one texel in x": lambda im, M, Mb: ((np.roll(im[0], 1, 1), np.roll(im[1], 1, 1)) + im[2:], M),
            "rolled one texel in y": lambda im, M, Mb: ((np.roll(im[0], 1, 0), np.roll(im[1], 1, 0)) + im[2:], M),
            "rows flipped": lambda im, M, Mb: ((im[0][::-1], im[1][::-1]) + im[2:], M),
            "prev_world_to_clip of the current camera": lambda im, M, Mb: (im, Mb)}


@pytest.mark.parametrize("control", sorted(CONTROLS))
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_static_controls_fail(size, control):
    """The history images (colour and count) moved against the guides, or the wrong camera's matrix: checks 2 and 3 must notice."""
    c = reproject_inputs("mixed", *size, "A", "B")
    q, depth, classed = static_model(c, "A", "B")
    images, M = CONTROLS[control](c["images"], c["M"], world_to_clip(*size, "B"))
    out = run_static(c, images, M)
    dev = R.motion_deviation(out, q, depth, classed)[0]
    gdev, share = R.gather_deviation(out, q, depth, classed)
    print(f"control {size} {control}: motion {dev:.3f} px, gather {gdev:.3f} (share {share:.3f})")
    assert max(dev, gdev) >= CONTROL * TOL and share > 0.5


# ---- 4. moved objects and a deformed mesh --------------------------------------------------------------------------------------------------------------
def object_masks(cur, state):
    k, o = cur[1][..., 3], R.bits(cur[2][..., 0])
    if state == "moved":
        return {"mesh": (k == 3) & (o == R.MOVED_MESH), "sphere": (k == 2) & (o == R.MOVED_SPHERE)}
    return {"blob": (k == 3) & (o == R.DEFORMED_MESH)}


def moved_case(W, H, state, tables=None, swap_uv=False):
    """(outputs of the restatement, model q, depth, classed, masks of the moved objects, the images given, q without the objects' own
    motion) for the state's pair of nearby cameras."""
    then, new = NEAR[state]
    c = reproject_inputs("mixed", W, H, then, new, state)
    rest, now = mixed(W, H), mixed(W, H, state)
    was = R.where_it_was(*c["cur"], R.SceneData(now), R.SceneData(rest))
    q, depth, classed = R.model_positions(c["cur"][0], c["cur"][1], CAMS[then], CAMS[new], was)
    q_still = R.model_positions(c["cur"][0], c["cur"][1], CAMS[then], CAMS[new])[0]
    images = c["images"]
    if swap_uv:
        ids = np.array(images[7])
        ids[..., 2], ids[..., 3] = images[7][..., 3], images[7][..., 2]
        images = images[:7] + (ids,)
    if state == "moved":
        if tables is None:
            tables = (host_scene.mesh_motion(rest.mesh_objects, now.mesh_objects), host_scene.sphere_motion(rest.spheres, now.spheres))
        out = reproject_objects_ref(*images, c["M"], *c["cam"], max_history=0.0, mesh_motion=tables[0], sphere_motion=tables[1])
    else:
        flags = np.zeros(len(rest.mesh_objects), np.int32)
        flags[R.DEFORMED_MESH] = 1
        out = reproject_deformed_ref(*images, c["M"], *c["cam"], max_history=0.0, deform=(rest.vertices, rest.indices, matrices_of(rest.mesh_objects), flags))
    return out, q, depth, classed, object_masks(c["cur"], state), images, q_still


@pytest.mark.parametrize("state", ["moved", "deformed"])
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_moved_and_deformed_pixels_come_from_where_identity_puts_them(size, state):
    out, q, depth, classed, masks, images, q_still = moved_case(*size, state)
    r, n = R.identity_residual(*images[5:8], R.SceneData(mixed(*size, state)))
    print(f"check 4 {size} {state}: identity {r:.2e} world units over {n} triangle pixels")
    assert r <= TOL_IDENTITY
    for name, mask in masks.items():
        dev, n, _, bad = R.motion_deviation(out, q, depth, classed, only=mask)
        gdev, share = R.gather_deviation(out, q, depth, classed, of=mask)
        print(f"   {name}: {int(mask.sum())} pixels, motion {dev:.2e} px over {n}, gather {gdev:.2e}, share checked {share:.3f}")
        assert mask.sum() >= 60 and n >= 0.9 * mask.sum()
        assert dev <= TOL_MOVED and bad == 0
        assert gdev <= TOL_MOVED and share >= MIN_SHARE_MOVED
        assert np.abs(q - q_still)[mask].max() >= 1.0                        # the case does move the object by a pixel or more on its own
    dev, n, _, bad = R.motion_deviation(out, q, depth, classed)               # and everything else in the image stays right
    gdev, share = R.gather_deviation(out, q, depth, classed, of=R.classes(*images[5:7])[0])
    print(f"   whole image: motion {dev:.2e} px over {n}, gather {gdev:.2e}, share of surface pixels {share:.3f}")
    assert dev <= TOL_MOVED and bad == 0 and gdev <= TOL_MOVED and share > 0.5


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_inverted_motion_table_fails(size):
    rest, now = mixed(*size), mixed(*size, "moved")
    tables = (R.inverted_table(host_scene.mesh_motion(rest.mesh_objects, now.mesh_objects)),
              R.inverted_table(host_scene.sphere_motion(rest.spheres, now.spheres)))
    out, q, depth, classed, masks = moved_case(*size, "moved", tables=tables)[:5]
    for name, mask in masks.items():
        dev = R.motion_deviation(out, q, depth, classed, only=mask)[0]
        print(f"control {size} inverted table, {name}: motion {dev:.3f} px")
        assert dev >= CONTROL * TOL_MOVED


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_swapped_barycentrics_fail(size):
    out, q, depth, classed, masks, images = moved_case(*size, "deformed", swap_uv=True)[:6]
    dev = R.motion_deviation(out, q, depth, classed, only=masks["blob"])[0]
    r, _ = R.identity_residual(*images[5:8], R.SceneData(mixed(*size, "deformed")))
    print(f"control {size} u and v swapped: motion {dev:.3f} px, identity {r:.3f} world units")
    assert dev >= CONTROL * TOL_MOVED and r >= CONTROL * TOL_IDENTITY


# ---- 5. upsampling ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", R.UPSAMPLE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_upsampling_a_plane_reproduces_the_screen_ramp(pair):
    w, h, W, H = pair
    out = upsample_ref(R.screen_ramp(w, h), *guides("mixed", w, h, "plane"), *guides("mixed", W, H, "plane"), flags=0)
    inside = R.four_taps_inside(w, h, W, H)
    d = R.upsample_deviation(out["color"], W, H)
    print(f"check 5a {pair}: {d[inside].max():.2e} over {int(inside.sum())} of {W * H} pixels")
    assert inside.mean() > 0.8 and d[inside].max() <= TOL_UPSAMPLE


@pytest.mark.parametrize("source,pair", [("analytic", p) for p in R.MIXED_PAIRS] + [("mixed", p) for p in R.MIXED_PAIRS],
                         ids=lambda p: p if isinstance(p, str) else "%dx%d-%dx%d" % p)
def test_upsampling_a_mixed_view(source, pair):
    """Both grids look through the full grid's camera (the low one keeps its width : height), as a host that upsamples renders them."""
    w, h, W, H = pair
    full = guides(source, W, H, "A")
    low_cam = dict(CAMS["A"], aspect=W / H)
    low = guides(source, w, h, "A", aspect=W / H)
    d1 = R.own_pixel_deviation(low[0], low[1], low_cam)
    out = upsample_ref(R.screen_ramp(w, h), *low, *full, flags=0)
    share = float((R.upsample_deviation(out["color"], W, H) <= TOL_UPSAMPLE).mean())
    rel = R.grid_relation_deviation(full[0], full[1], w, h, low_cam, low_grid_position(W, w), low_grid_position(H, h))
    print(f"check 5b {source} {pair}: share within {TOL_UPSAMPLE:g}: {share:.3f}; low grid check 1 {d1:.2e} px; 5c grid relation {rel:.2e} low px")
    assert share >= MIN_SHARE_UPSAMPLE
    assert d1 <= TOL and rel <= TOL


@pytest.mark.parametrize("pair", R.MIXED_PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_low_grid_half_a_pixel_off_fails(pair):
    """A low grid whose pixel-centre rays pass half a low pixel off: its guides miss check 1, and its colours, which show what those rays
    see, land half a low pixel off on the full grid (a sky texel has no hit point to tell where it looked and keeps its centre's colour,
    so the share is taken over the full grid's surface pixels)."""
    w, h, W, H = pair
    low_cam = dict(CAMS["A"], aspect=W / H)
    full = guides("mixed", W, H, "A")
    surface = R.classes(*full[:2])[0]
    shares = {}
    for half_off in (True, False):
        low = guides("mixed", w, h, "A", half_off=half_off, aspect=W / H)
        out = upsample_ref(R.seen_ramp(low[0], low[1], low_cam), *low, *full, flags=0)
        d = R.upsample_deviation(out["color"], W, H)
        shares[half_off] = float((d[surface] <= TOL_UPSAMPLE).mean())
        if half_off:
            d1, median = R.own_pixel_deviation(low[0], low[1], low_cam), float(np.median(d[surface & out["result"]]))
    print(f"control {pair} half a low pixel off: check 1 {d1:.3f} px; surface pixels within {TOL_UPSAMPLE:g}: {shares[True]:.3f} (median deviation "
          f"{median:.2e}); the same on the right grid: {shares[False]:.3f}")
    assert d1 >= CONTROL * TOL
    assert shares[True] <= 0.05 and median >= CONTROL * TOL_UPSAMPLE
    assert shares[False] >= 0.5


# ---- 6. denoiser ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_denoiser_leaves_a_ramp_on_uniform_guides_alone(iterations):
    W, H = 67, 45
    hit, normal = R.uniform_guides(W, H)
    src = R.denoise_ramp(W, H)
    out = denoise_ref(src, hit, normal, iterations=iterations, sigma_color=0.0)
    assert reach(iterations) == 2 * (2 ** iterations - 1)
    inner = R.interior(W, H, reach(iterations))
    err = np.abs(out[..., :3] - src[..., :3].astype(np.float64))
    bound = 1e-4 * (1.0 + np.abs(src[..., :3].astype(np.float64)))
    print(f"check 6 iterations {iterations}: interior {err[inner].max():.2e} over {int(inner.sum())} pixels, borders up to {err[~inner].max():.2f}")
    assert inner.sum() >= 100 and (err[inner] <= bound[inner]).all()
    assert err[~inner].max() > 0.1                                            # the borders do show what a lopsided footprint does


# ---- 7. bloom ------------------------------------------------------------------------------------------------------------------------------------------------
BLOOM_CASES = [(97, 61, 48, 30, 3), (97, 61, 47, 31, 3), (131, 95, 65, 47, 4)]
BLOOM_PARAMS = dict(threshold=0.0, soft_knee=0.0, intensity=1.0)
TOL_CENTROID, TOL_SUM = 1e-4, 1e-5                                           # measured <= 8e-8 px and <= 4e-8 relative


@pytest.mark.parametrize("case", BLOOM_CASES, ids=lambda c: "%dx%d-at-%d-%d-levels-%d" % c)
def test_bloom_of_an_impulse_is_centred_on_it(case):
    W, H, x, y, levels = case
    src = R.impulse(W, H, x, y)
    dst, _ = bloom_ref(src, levels=levels, **BLOOM_PARAMS)
    cx, cy, s, edge = R.glow_moments(dst, src)
    print(f"check 7 {case}: centroid off by {np.abs(cx - x).max():.1e}, {np.abs(cy - y).max():.1e} px, sum off by "
          f"{np.abs(s / src[y, x, :3] - 1).max():.1e} relative")
    assert edge == 0.0                                                       # the support does not touch a border
    assert np.abs(cx - x).max() <= TOL_CENTROID and np.abs(cy - y).max() <= TOL_CENTROID
    assert (np.abs(s / src[y, x, :3].astype(np.float64) - 1.0) <= TOL_SUM).all()
